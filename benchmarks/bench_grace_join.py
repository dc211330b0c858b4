"""Native partitioner and the out-of-core (grace) join.

  python benchmarks/bench_grace_join.py [--part-rows-log2 26]
      [--build-rows-log2 25] [--probe-rows-log2 27] [--out FILE.json]

(a) `rowops.partition_by_hash` on int64 keys for P in {8, 64, 256}: the
    one-pass native partitioner against the path it replaces (u64_mod +
    bincount + full radix argsort, which is still what P > 256 runs), the
    two alternating, each the median of `--reps` device-synchronised calls
    after a warm-up, with their outputs compared.
(b) An inner join, unique int64 build keys, every probe key hits: once with
    no memory limit and once with `memory_limit_bytes` at a quarter of the
    build side, which takes the grace path.  Prints both times, their ratio
    (the price of spilling) and the operator's grace_stats.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import daft_amd as daft  # noqa: E402
from daft_amd import execution_config_ctx  # noqa: E402
from daft_amd.kernels import native_required, rowops  # noqa: E402
from daft_amd.physical import ops  # noqa: E402
from daft_amd.schema import DataType  # noqa: E402
from daft_amd.series import Series  # noqa: E402

DEV = "cuda:0"


def _sync_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def radix_sort_partition(keys, parts):
    """The three-step path: ids to memory, bincount, full radix argsort."""
    h = rowops.hash_columns(keys)
    part = native_required().u64_mod(h, parts)
    counts = torch.bincount(part, minlength=parts)
    return rowops._stable_sort_perm_by(part), counts


def bench_partition(n, reps, emit):
    g = torch.Generator(device=DEV).manual_seed(0)
    data = torch.randint(-(1 << 62), 1 << 62, (n,), device=DEV, generator=g)
    keys = [Series("k", DataType.int64(), data=data)]
    hash_ms = _median([_sync_ms(lambda: rowops.hash_columns(keys))[0]
                       for _ in range(reps + 1)][1:])
    for parts in (8, 64, 256):
        old = lambda: radix_sort_partition(keys, parts)      # noqa: E731
        new = lambda: rowops.partition_by_hash(keys, parts)  # noqa: E731
        _, (po, co) = _sync_ms(old)        # warm-up, and the outputs
        _, (pn, cn) = _sync_ms(new)
        same = bool(torch.equal(po, pn) and torch.equal(co, cn))
        del po, co, pn, cn
        t_old, t_new = [], []
        for _ in range(reps):              # alternate the two
            t_old.append(_sync_ms(old)[0])
            t_new.append(_sync_ms(new)[0])
        emit({"bench": "partition_by_hash", "rows": n, "P": parts,
              "radix_sort_path_ms": round(_median(t_old), 3),
              "native_ms": round(_median(t_new), 3),
              "radix_sort_path_all_ms": [round(t, 3) for t in t_old],
              "native_all_ms": [round(t, 3) for t in t_new],
              "hash_columns_ms_included": round(hash_ms, 3),
              "speedup": round(_median(t_old) / _median(t_new), 2),
              "outputs_equal": same})


def bench_join(n_build, n_probe, batch_rows, reps, emit):
    g = torch.Generator(device=DEV).manual_seed(1)
    bk = torch.randperm(n_build, device=DEV, generator=g)
    pk = torch.randint(0, n_build, (n_probe,), device=DEV, generator=g)
    build = daft.from_pydict(
        {"k": bk, "bv": torch.arange(n_build, device=DEV)}, device=DEV)
    probe = daft.from_pydict(
        {"k": pk, "pv": torch.arange(n_probe, device=DEV)}, device=DEV) \
        .into_batches(batch_rows)
    build_bytes = n_build * 16
    build = build.into_batches(batch_rows)
    del bk, pk

    seen = []
    orig = ops.JoinOp.execute

    def execute(self, ectx):
        seen.append(self)
        return orig(self, ectx)
    ops.JoinOp.execute = execute

    def run(limit):
        def go():
            rows = ksum = 0
            with execution_config_ctx(memory_limit_bytes=limit):
                for part in probe.join(build, on="k").iter_partitions():
                    rows += len(part)
                    ksum += int(part.column("bv").data.sum().item())
            return rows, ksum
        return go

    limit = build_bytes // 4
    res = {}
    for name, lim in (("in_memory", None), ("grace", limit)):
        times = []
        for _ in range(reps + 1):          # first run is the warm-up
            seen.clear()
            ms, (rows, ksum) = _sync_ms(run(lim))
            times.append(ms)
        res[name] = {"ms": round(_median(times[1:]), 1),
                     "all_ms": [round(t, 1) for t in times[1:]],
                     "warmup_ms": round(times[0], 1),
                     "rows_out": rows, "sum_bv": ksum,
                     "grace_stats": seen[-1].grace_stats}
    ops.JoinOp.execute = orig
    assert res["in_memory"]["grace_stats"] is None
    assert res["grace"]["grace_stats"] is not None
    emit({"bench": "inner_join", "build_rows": n_build,
          "probe_rows": n_probe, "batch_rows": batch_rows,
          "build_bytes": build_bytes, "memory_limit_bytes": limit,
          "in_memory": res["in_memory"], "grace": res["grace"],
          "grace_over_in_memory": round(
              res["grace"]["ms"] / res["in_memory"]["ms"], 2),
          "outputs_equal": (res["grace"]["rows_out"], res["grace"]["sum_bv"])
          == (res["in_memory"]["rows_out"], res["in_memory"]["sum_bv"])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part-rows-log2", type=int, default=26)
    ap.add_argument("--build-rows-log2", type=int, default=25)
    ap.add_argument("--probe-rows-log2", type=int, default=27)
    ap.add_argument("--batch-rows-log2", type=int, default=23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--join-reps", type=int, default=3)
    ap.add_argument("--skip", choices=("partition", "join"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    native_required()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.skip != "partition":
        bench_partition(1 << args.part_rows_log2, args.reps, emit)
    if args.skip != "join":
        bench_join(1 << args.build_rows_log2, 1 << args.probe_rows_log2,
                   1 << args.batch_rows_log2, args.join_reps, emit)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

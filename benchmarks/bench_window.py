"""Framed window aggregates: the native scan kernels (csrc/window.hip)
against the torch prefix-sum / sparse-table path they replace on the device.

  python benchmarks/bench_window.py [--rows-log2 24]
      [--partitions 1 1000 1000000] [--reps 5] [--out FILE.json]

Data is made on the device with a fixed seed: float64 values in [0, 1), a
random partition id per row and a random int64 order key.  Three queries per
partition count: a running sum, a mean over rows_between(-99, 0) and a min
over rows_between(-99, 0).

The sort is shared: partition ids, permutation and offsets are built once per
partition count, and each measurement times `_framed_agg` alone, without
`seg` (the torch path, still the CPU implementation) and with it (native).
The two alternate, each time the median of `--reps` device-synchronised
calls after a warm-up, and their outputs are compared.  For the min query the
peak of torch.cuda.max_memory_allocated above the resident inputs is
reported for both paths.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from daft_amd import col  # noqa: E402
from daft_amd.kernels import native_required, rowops  # noqa: E402
from daft_amd.physical import window as win  # noqa: E402
from daft_amd.recordbatch import RecordBatch  # noqa: E402
from daft_amd.schema import DataType  # noqa: E402
from daft_amd.series import Series  # noqa: E402
from daft_amd.window import Window  # noqa: E402

DEV = "cuda:0"
QUERIES = [
    ("running_sum", lambda c: c.sum(),
     (Window.unbounded_preceding, Window.current_row)),
    ("mean_100", lambda c: c.mean(), (-99, 0)),
    ("min_100", lambda c: c.min(), (-99, 0)),
]


def _sync_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _peak_mib(fn):
    """Peak device memory of one call above what is resident before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def make_batch(n, partitions, gen):
    """(batch, gids, sorted_pos, order_by nodes, seg), as run_window has them
    after its sort."""
    v = torch.rand(n, dtype=torch.float64, device=DEV, generator=gen)
    o = torch.randint(0, 1 << 62, (n,), device=DEV, generator=gen)
    g = torch.randint(0, partitions, (n,), device=DEV, generator=gen)
    batch = RecordBatch([Series("g", DataType.int64(), data=g),
                         Series("o", DataType.int64(), data=o),
                         Series("v", DataType.float64(), data=v)],
                        num_rows=n)
    if partitions > 1:
        gids, reps = rowops.groupby([batch.columns[0]])
        num_groups = int(reps.shape[0])
    else:
        gids, num_groups = torch.zeros_like(g), 1
    perm = rowops.argsort_multi(
        [Series("__g", DataType.int64(), data=gids), batch.columns[1]],
        [False, False], [False, False])
    pos = torch.empty_like(perm)
    pos[perm] = torch.arange(n, dtype=torch.int64, device=DEV)
    part_start = win._partition_starts(gids[perm], num_groups)
    seg = win._seg_offsets(gids, num_groups)
    order_by = Window().order_by("o").order_by_exprs
    return batch, gids, (perm, pos, part_start), order_by, seg, num_groups


def bench_partitions(n, partitions, reps, emit):
    gen = torch.Generator(device=DEV).manual_seed(42)
    batch, gids, sorted_pos, order_by, seg, num_groups = \
        make_batch(n, partitions, gen)
    base = {"bench": "window", "rows": n, "partitions": num_groups}
    for name, make_agg, frame in QUERIES:
        a = make_agg(col("v"))._node
        torch_fn = lambda: win._framed_agg(          # noqa: E731
            batch, a, "w", gids, sorted_pos, order_by, frame)
        native_fn = lambda: win._framed_agg(         # noqa: E731
            batch, a, "w", gids, sorted_pos, order_by, frame, seg)
        _, x = _sync_ms(torch_fn)          # warm-up, and the outputs
        _, y = _sync_ms(native_fn)
        # min is exact; the sums differ by the order of the additions, and
        # the torch path's whole-batch prefix carries an absolute error of
        # about an ulp of the grand total
        diff = float((x.data - y.data).abs().max().item())
        scale = float(x.data.abs().max().item())
        same_valid = (x.validity is None) == (y.validity is None)
        del x, y
        t_old, t_new = [], []
        for _ in range(reps):              # alternate the two
            t_old.append(_sync_ms(torch_fn)[0])
            t_new.append(_sync_ms(native_fn)[0])
        row = dict(base, query=name,
                   torch_ms=round(_median(t_old), 3),
                   native_ms=round(_median(t_new), 3),
                   torch_all_ms=[round(t, 3) for t in t_old],
                   native_all_ms=[round(t, 3) for t in t_new],
                   speedup=round(_median(t_old) / _median(t_new), 2),
                   max_abs_diff=diff, max_abs_value=scale,
                   validity_agrees=same_valid)
        if name == "min_100":
            row["torch_peak_mib"] = _peak_mib(torch_fn)
            row["native_peak_mib"] = _peak_mib(native_fn)
        emit(row)
        assert same_valid and diff <= 1e-6 * max(scale, 1.0), \
            f"torch and native outputs differ ({name})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=24)
    ap.add_argument("--partitions", type=int, nargs="+",
                    default=[1, 1000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    native_required()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for partitions in args.partitions:
        bench_partitions(1 << args.rows_log2, partitions, args.reps, emit)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

"""Top-k: rowops.topk_multi (radix select on the leading key, then a sort of
the candidates) against the full sort it replaces.

  python benchmarks/bench_topn.py [--min-log2 18] [--max-log2 27]
      [--ks 10 100 10000] [--k-fractions 2 8 32] [--shapes int64 q3 string]
      [--reps 5] [--out FILE.json]

Data is made on the device with a fixed seed.  Three key shapes:
  int64   one uniform int64 key, ascending;
  q3      (float64 revenue descending, int32 date ascending), TPC-H Q3's order;
  string  one key of 16..24 random lowercase bytes (about 20), ascending.
`--k-fractions F` adds k = n // F per row count, which is how the k/n end of
the gate is found.  The gate constants are forced open while measuring, so
every (n, k) runs the select path.

Old is `argsort_multi(...)[:k]`, new is `topk_multi`; they run alternately,
each the median of `--reps` device-synchronised calls after a warm-up, and
their outputs are compared.  A further line per row count splits the new path
(at the first k) into select, take and residual sort.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from daft_amd.kernels import native_required, rowops  # noqa: E402
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


def make_keys(shape, n, gen):
    """(keys, descending, nulls_first)"""
    if shape == "int64":
        k = torch.randint(-(1 << 62), 1 << 62, (n,), device=DEV, generator=gen)
        return [Series("k", DataType.int64(), data=k)], [False], [False]
    if shape == "q3":
        rev = torch.rand(n, device=DEV, dtype=torch.float64,
                         generator=gen) * 5e5
        day = torch.randint(8036, 10592, (n,), device=DEV, generator=gen,
                            dtype=torch.int32)
        return ([Series("revenue", DataType.float64(), data=rev),
                 Series("o_orderdate", DataType.date(), data=day)],
                [True, False], [False, False])
    lens = torch.randint(16, 25, (n,), device=DEV, generator=gen)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(lens, 0, out=offsets[1:])
    data = torch.randint(97, 123, (int(offsets[-1].item()),), device=DEV,
                         generator=gen, dtype=torch.uint8)
    return ([Series("s", DataType.string(), data=data, offsets=offsets,
                    length=n)], [False], [False])


def bench_split(keys, desc, nf, k, reps):
    """Median ms of the three stages of the select path, one after another."""
    t_sel, t_take, t_sort = [], [], []
    for _ in range(reps + 1):
        ms, (rows, _stats) = _sync_ms(lambda: rowops.topk_candidates(
            rowops._leading_image(keys[0], desc[0], nf[0]), k))
        t_sel.append(ms)
        ms, sub = _sync_ms(lambda: [s.take(rows, has_neg=False)
                                    for s in keys])
        t_take.append(ms)
        ms, _ = _sync_ms(lambda: rows[rowops.argsort_multi(sub, desc,
                                                           nf)[:k]])
        t_sort.append(ms)
    return {"select_ms": round(_median(t_sel[1:]), 3),
            "take_ms": round(_median(t_take[1:]), 3),
            "residual_sort_ms": round(_median(t_sort[1:]), 3),
            "candidates": int(rows.numel())}


def bench_shape(shape, n, ks, reps, emit):
    gen = torch.Generator(device=DEV).manual_seed(42)
    keys, desc, nf = make_keys(shape, n, gen)
    base = {"bench": "topn", "shape": shape, "rows": n}
    for k in ks:
        old = lambda: rowops.argsort_multi(keys, desc, nf)[:k]   # noqa: E731
        new = lambda: rowops.topk_multi(keys, desc, nf, k)       # noqa: E731
        _, a = _sync_ms(old)               # warm-up, and the outputs
        _, b = _sync_ms(new)
        same = bool(torch.equal(a, b))
        del a, b
        assert same, f"full sort and top-k outputs differ ({shape}, {n}, {k})"
        t_old, t_new = [], []
        for _ in range(reps):              # alternate the two
            t_old.append(_sync_ms(old)[0])
            t_new.append(_sync_ms(new)[0])
        emit(dict(base, k=k, sort_ms=round(_median(t_old), 3),
                  topk_ms=round(_median(t_new), 3),
                  sort_all_ms=[round(t, 3) for t in t_old],
                  topk_all_ms=[round(t, 3) for t in t_new],
                  speedup=round(_median(t_old) / _median(t_new), 2),
                  topk_wins=max(t_new) < min(t_old), outputs_equal=same))
    emit(dict(base, k=ks[0], split=bench_split(keys, desc, nf, ks[0], reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log2", type=int, default=18)
    ap.add_argument("--max-log2", type=int, default=27)
    ap.add_argument("--ks", type=int, nargs="*", default=[10, 100, 10_000])
    ap.add_argument("--k-fractions", type=int, nargs="*", default=[])
    ap.add_argument("--shapes", nargs="+", default=["int64", "q3", "string"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    native_required()
    rowops._TOPK_MIN_ROWS = 1          # measure the select path everywhere
    rowops._TOPK_MAX_FRACTION = 1
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for log2 in range(args.min_log2, args.max_log2 + 1):
        n = 1 << log2
        ks = sorted({k for k in args.ks if k <= n} |
                    {n // f for f in args.k_fractions if n // f >= 1})
        for shape in args.shapes:
            bench_shape(shape, n, ks, args.reps, emit)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

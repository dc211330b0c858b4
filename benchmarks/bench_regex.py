"""Regex / LIKE predicates over a device column of per-row text.

  python benchmarks/bench_regex.py [--rows N] [--reps R] [--out FILE.json]

The column is built on the device by concatenating randomly drawn words
(`concat_str`), so it is plain offsets + bytes, not dictionary-encoded: a
predicate that leaves the device pays one interpreter call per row.  Four
predicates are timed through the wrappers in daft_amd/kernels/strings.py,
each as the median of `--reps` calls after one warm-up call, with the device
synchronised around every call.  Prints ms, rows/s and bytes/s per predicate,
and the hit count plus a position checksum so that two builds can be checked
for equal answers.  The script only uses calls that exist on older trees too:
run it on two commits to compare them."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from daft_amd.kernels import native_required  # noqa: E402
from daft_amd.kernels import strings as strk  # noqa: E402
from daft_amd.schema import DataType  # noqa: E402
from daft_amd.series import Series  # noqa: E402

FIRST = ["Special", "Pending", "Order", "Regular", "special", "final",
         "ironic", "express", "abc", "quick", "Deposit", "carefully"]
SECOND = [" requests", " 2024", " 17", " 123456", " packages", " accounts",
          " a-c", " theodolites", " deposits", " 999"]
REST = [" special", " requests", " sleep", " furiously", " among", " the",
        " SPECIAL", " pinto", " beans", " axc", " blithely", " even"]

QUERIES = [
    ("regexp_match special.*requests",
     lambda s: strk.regexp_match(s, r"special.*requests")),
    ("regexp_match ^[A-Z][a-z]+ \\d{2,4}$",
     lambda s: strk.regexp_match(s, r"^[A-Z][a-z]+ \d{2,4}$")),
    ("LIKE %a_c%", lambda s: strk.like(s, "%a_c%")),
    ("ILIKE %SPECIAL%",
     lambda s: strk.like(s, "%SPECIAL%", case_insensitive=True)),
]


def build_column(n: int, dev: str) -> Series:
    """Rows of two words; nine in ten carry four more."""
    g = torch.Generator(device=dev).manual_seed(0)

    def draw(words, keep=None):
        vocab = Series.from_pylist("w", words + [""], DataType.string(),
                                   device=dev)
        idx = torch.randint(0, len(words), (n,), device=dev, generator=g)
        if keep is not None:
            idx = torch.where(keep, idx, torch.full_like(idx, len(words)))
        return vocab.take(idx)

    long_row = torch.rand(n, device=dev, generator=g) < 0.9
    parts = [draw(FIRST), draw(SECOND)] + \
        [draw(REST, long_row) for _ in range(4)]
    s = strk.concat_str(parts)
    assert not s.is_dict() and s.is_gpu() and len(s) == n
    return s


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_regex.py needs a GPU"
    native_required()
    dev = "cuda:0"
    s = build_column(args.rows, dev)
    nbytes = int(s.data.numel())
    engine = "dfa kernel" if hasattr(strk, "_device_dfa_pred") else "host re"
    print(f"rows={args.rows} bytes={nbytes} "
          f"({nbytes / args.rows:.1f}/row) engine={engine}")
    weights = torch.arange(1, args.rows + 1, device=dev)
    rows = []
    for name, fn in QUERIES:
        res = fn(s)
        assert res.data.is_cuda and res.data.dtype == torch.bool
        hits = int(res.data.sum())
        checksum = int((res.data.to(torch.int64) * weights).sum())
        med, lo, hi = timed(lambda: fn(s), args.reps)
        row = {"query": name, "ms": med, "ms_min": lo, "ms_max": hi,
               "rows_per_s": args.rows / (med * 1e-3),
               "bytes_per_s": nbytes / (med * 1e-3),
               "hits": hits, "checksum": checksum}
        rows.append(row)
        print(f"{name:40s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]  "
              f"{row['rows_per_s']:.3e} rows/s  "
              f"{row['bytes_per_s']:.3e} B/s  hits={hits} "
              f"checksum={checksum}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": args.rows, "bytes": nbytes, "engine": engine,
                       "reps": args.reps, "queries": rows}, f, indent=1)


if __name__ == "__main__":
    main()

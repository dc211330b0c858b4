"""Regex functions that need match positions (count, extract, extract_all,
replace, split) over a device column of per-row text.

  python benchmarks/bench_regex_spans.py [--rows N] [--reps R] [--out FILE.json]

The column is the one bench_regex.py builds on the device: plain offsets +
bytes, not dictionary-encoded, so a function that leaves the device pays one
interpreter call per row.  The five functions are timed through the public
free functions of daft_amd.functions, each as the median of `--reps` calls
after one warm-up call, with the device synchronised around every call.
Prints ms and rows/s per function, and a checksum (the sum of the counts; for
strings the rows, items and bytes of the output) so that two builds can be
checked for equal answers.  The script only uses calls that exist on older
trees too: run it on two commits to compare them."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_regex import build_column  # noqa: E402
from daft_amd import col  # noqa: E402
from daft_amd import functions as F  # noqa: E402
from daft_amd.kernels import native_required  # noqa: E402
from daft_amd.kernels import regex_dfa  # noqa: E402

QUERIES = [
    ("regexp_count \\d+", F.regexp_count(col("s"), r"\d+")),
    ("regexp_extract [A-Z][a-z]+", F.regexp_extract(col("s"), r"[A-Z][a-z]+")),
    ("regexp_extract_all [a-z]+ly",
     F.regexp_extract_all(col("s"), r"[a-z]+ly")),
    ("regexp_replace special|SPECIAL -> X",
     F.regexp_replace(col("s"), r"special|SPECIAL", "X")),
    ("regexp_split ' +'", F.regexp_split(col("s"), r" +")),
]


def run(expr, s):
    node = expr._node
    return node.fn(s, *node.literal_args, **node.kwargs)


def checksum(res) -> dict:
    """Figures that are equal exactly when two builds gave equal shapes."""
    assert res.is_gpu()
    if res.offsets is not None and res.children:        # list<string>
        child = res.children[0].dict_decode()
        return {"rows": len(res), "items": len(child),
                "bytes": int(child.data.numel()),
                "offsets_sum": int(res.offsets.sum())}
    if res.offsets is not None or res.is_dict():        # string
        res = res.dict_decode()
        valid = len(res) if res.validity is None else int(res.validity.sum())
        lens = res.offsets[1:] - res.offsets[:-1]
        if res.validity is not None:
            lens = lens * res.validity
        return {"rows": len(res), "valid": valid, "bytes": int(lens.sum())}
    data = res.data if res.validity is None else res.data * res.validity
    return {"rows": len(res), "sum": int(data.sum())}


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
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_regex_spans.py needs a GPU"
    native_required()
    dev = "cuda:0"
    s = build_column(args.rows, dev)
    nbytes = int(s.data.numel())
    engine = "span kernels" if hasattr(regex_dfa, "compile_spans") \
        else "host re"
    print(f"rows={args.rows} bytes={nbytes} "
          f"({nbytes / args.rows:.1f}/row) engine={engine}", flush=True)
    rows = []
    for name, expr in QUERIES:
        check = checksum(run(expr, s))
        med, lo, hi = timed(lambda: run(expr, s), args.reps)
        row = {"query": name, "ms": med, "ms_min": lo, "ms_max": hi,
               "rows_per_s": args.rows / (med * 1e-3), "checksum": check}
        rows.append(row)
        print(f"{name:38s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]  "
              f"{row['rows_per_s']:.3e} rows/s  {check}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": args.rows, "bytes": nbytes, "engine": engine,
                       "reps": args.reps, "queries": rows}, f, indent=1)


if __name__ == "__main__":
    main()

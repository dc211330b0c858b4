"""Text cleanup in front of dedup: `normalize` with its defaults and `strip`
over a device column of web-like documents.

  python benchmarks/bench_normalize.py [--rows N] [--non-ascii SHARE]
                                       [--reps R] [--out FILE.json]

Each document is about 50 words in mixed case with stray punctuation and runs
of mixed whitespace, padded with whitespace on both sides; `--non-ascii` is
the share of documents that also hold accented and CJK words.  The column is
plain offsets + bytes on cuda:0, not dictionary-encoded, so a function that
leaves the device pays one interpreter call per row.  Both functions are
timed through the public API, each as the median of `--reps` calls after one
warm-up call, with the device synchronised around every call.  Prints one
JSON line: ms, rows/s and input GB/s per function, and a checksum (rows,
valid rows and bytes of the output) so that two builds can be checked for
equal answers.  The script only uses calls that exist on older trees too: run
it on two commits to compare them."""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from daft_amd import DataType, Series, col  # noqa: E402
from daft_amd import functions as F  # noqa: E402
from daft_amd.kernels import native_required  # noqa: E402

WORDS = ("the quick brown fox jumps over lazy dog data center model text "
         "clean token near duplicate page web crawl filter hash bucket "
         "signature shingle band row column stream kernel wave").split()
ACCENTED = ["café", "naïve", "straße", "señor", "漢字", "über", "€uro"]
PUNCT = [",", ".", "!", "?", ";", ":", " -", "...", ")", "\""]
GAPS = [" ", " ", " ", "  ", "\t", "\n", " \n ", "\r\n", "   "]


def make_doc(rng, non_ascii: bool) -> str:
    parts = [rng.choice(GAPS)]
    for k in range(rng.randrange(40, 61)):
        # a non-ASCII document: its first word, and every tenth after it
        w = rng.choice(ACCENTED) \
            if non_ascii and (k == 0 or rng.random() < 0.1) \
            else rng.choice(WORDS)
        r = rng.random()
        if r < 0.15:
            w = w.capitalize()
        elif r < 0.20:
            w = w.upper()
        if rng.random() < 0.2:
            w += rng.choice(PUNCT)
        parts.append(w)
        parts.append(rng.choice(GAPS))
    return "".join(parts)


def build_column(rows: int, share: float, device) -> Series:
    """`rows` documents drawn from pools of 4096 distinct ones."""
    rng = random.Random(0)
    plain = [make_doc(rng, False) for _ in range(4096)]
    mixed = [make_doc(rng, True) for _ in range(4096)]
    assert all(d.isascii() for d in plain)
    assert all(not d.isascii() for d in mixed)
    vals = [rng.choice(mixed) if rng.random() < share else rng.choice(plain)
            for _ in range(rows)]
    return Series.from_pylist("s", vals, DataType.string(), device=device)


def run(expr, s):
    node = expr._node
    return node.fn(s, *node.literal_args, **node.kwargs)


def checksum(res) -> dict:
    assert res.is_gpu()
    res = res.dict_decode()
    valid = len(res) if res.validity is None else int(res.validity.sum())
    lens = res.offsets[1:] - res.offsets[:-1]
    if res.validity is not None:
        lens = lens * res.validity
    return {"rows": len(res), "valid": valid, "bytes": int(lens.sum()),
            "byte_sum": int(res.data.sum(dtype=torch.int64))}


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
    ap.add_argument("--non-ascii", type=float, default=0.0,
                    help="share of documents with non-ASCII words")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_normalize.py needs a GPU"
    native_required()
    s = build_column(args.rows, args.non_ascii, "cuda:0")
    nbytes = int(s.data.numel())
    queries = [("normalize", F.normalize(col("s"))),
               ("strip", col("s").str.strip())]
    result = {"rows": args.rows, "bytes": nbytes,
              "non_ascii_share": args.non_ascii, "reps": args.reps,
              "queries": []}
    for name, expr in queries:
        check = checksum(run(expr, s))
        med, lo, hi = timed(lambda: run(expr, s), args.reps)
        result["queries"].append({
            "query": name, "ms": med, "ms_min": lo, "ms_max": hi,
            "rows_per_s": args.rows / (med * 1e-3),
            "input_gb_per_s": nbytes / (med * 1e-3) / 1e9,
            "checksum": check})
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

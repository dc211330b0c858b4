"""Text -> values after ingest: casts of device string columns to integers,
decimals, floats and dates, `str.to_date`, and integers and dates cast back
to text.

  python benchmarks/bench_parse.py [--rows N] [--reps R] [--out FILE.json]

The columns hold `--rows` rows each: integers of 1-18 digits, prices with two
decimals, `repr` of random doubles, and ISO dates, as plain offsets + bytes on
cuda:0.  Every query runs through the public API (`Series.cast`,
`str.to_date`) and is timed as the median of `--reps` calls after one warm-up
call, with the device synchronised around every call.  Prints one JSON line:
per query ms, rows/s, input GB/s, the share of rows that went to the host
(null where the tree has no such path), and a checksum (rows, valid rows and
a sum over the output) so that two builds can be checked for equal answers.
Where the build can switch the LDS staging of the parse kernels, the parse
queries are timed both ways (`ms_staged`, `ms_direct`).  The script only uses
calls that exist on older trees too: run it on two commits to compare them."""
import argparse
import json
import os
import random
import struct
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from daft_amd import DataType, Series, col  # noqa: E402
from daft_amd.kernels import native_required  # noqa: E402

POOL = 1 << 16   # distinct rows per column; the columns draw from them


def build_columns(rows: int, device) -> dict:
    rng = random.Random(0)
    ints = [str(rng.randrange(-10**d, 10**d))
            for d in (rng.randint(1, 18) for _ in range(POOL))]
    prices = ["%d.%02d" % (rng.randrange(10**6), rng.randrange(100))
              for _ in range(POOL)]
    floats = []
    while len(floats) < POOL:
        b = rng.getrandbits(64)
        if 0 < (b >> 52) & 0x7FF < 0x7FF:
            floats.append(repr(struct.unpack("<d", struct.pack("<Q", b))[0]))
    dates = ["%04d-%02d-%02d" % (rng.randint(1900, 2100), rng.randint(1, 12),
                                 rng.randint(1, 28)) for _ in range(POOL)]
    idx = torch.randint(0, POOL, (rows,),
                        generator=torch.Generator().manual_seed(0))
    out = {}
    for name, pool in (("int", ints), ("price", prices), ("float", floats),
                       ("date", dates)):
        s = Series.from_pylist("s", pool, DataType.string(), device=device)
        out[name] = s.take(idx.to(device))
    return out


def run(expr, s):
    node = expr._node
    return node.fn(s, *node.literal_args, **node.kwargs)


def checksum(res) -> dict:
    assert res.is_gpu()
    res = res.dict_decode()
    valid = len(res) if res.validity is None else int(res.validity.sum())
    d = res.data
    if res.offsets is None:
        d = d if res.validity is None else d[res.validity]
        d = d.view(torch.int64) if d.dtype == torch.float64 else d
    return {"rows": len(res), "valid": valid,
            "sum": int(d.sum(dtype=torch.int64))}


def host_share(fn, rows):
    """Share of rows handed to the host path, where the tree has one."""
    try:
        from daft_amd.kernels import parse
    except ImportError:
        return None
    sent = []
    real_p, real_s = parse._host_parse, parse._host_to_string
    parse._host_parse = lambda s, *a: sent.append(len(s)) or real_p(s, *a)
    parse._host_to_string = lambda s: sent.append(len(s)) or real_s(s)
    try:
        fn()
    finally:
        parse._host_parse, parse._host_to_string = real_p, real_s
    return sum(sent) / rows


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
    return out[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_parse.py needs a GPU"
    nat = native_required()
    cols = build_columns(args.rows, "cuda:0")
    as_int = cols["int"].cast(DataType.int64())
    as_date = cols["date"].cast(DataType.date())
    to_date = col("s").str.to_date("%Y-%m-%d")
    queries = [
        ("int64", cols["int"], lambda s: s.cast(DataType.int64())),
        ("decimal(12,2)", cols["price"],
         lambda s: s.cast(DataType.decimal128(12, 2))),
        ("float64", cols["float"], lambda s: s.cast(DataType.float64())),
        ("date", cols["date"], lambda s: s.cast(DataType.date())),
        ("to_date", cols["date"], lambda s: run(to_date, s)),
        ("int64->string", as_int, lambda s: s.cast(DataType.string())),
        ("date->string", as_date, lambda s: s.cast(DataType.string())),
    ]
    staging = getattr(nat, "strparse_staging", None)
    result = {"rows": args.rows, "reps": args.reps, "queries": []}
    for name, s, fn in queries:
        call = lambda: fn(s)   # noqa: E731
        nbytes = int(s.data.numel()) * s.data.element_size()
        med = timed(call, args.reps)
        q = {"query": name, "ms": med, "rows_per_s": args.rows / (med * 1e-3),
             "input_gb_per_s": nbytes / (med * 1e-3) / 1e9,
             "host_share": host_share(call, args.rows),
             "checksum": checksum(call())}
        if staging is not None and s.offsets is not None:
            was = staging(True)
            q["ms_staged"] = timed(call, args.reps)
            staging(False)
            q["ms_direct"] = timed(call, args.reps)
            staging(was)
        result["queries"].append(q)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

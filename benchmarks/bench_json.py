"""JSON-lines scan: host decode (pyarrow, `device_decode=False`) against device
decode (csrc/json.hip, `device_decode=True`) of the same file, in the same
run.

  python benchmarks/bench_json.py [--rows N] [--reps R] [--out FILE.json]

A lineitem-shaped file of `--rows` records and 16 keys in a fixed order
(integers, floats with two digits, dates as strings, flags, and a comment
that in a fraction of the rows holds `\\"`, `\\n` and `\\u00e9` escapes) is
written to a temporary directory.  Each query reads it through
`daft.read_json` on cuda:0 and keeps the batches on the device: all 16
columns, and 3 of them.  Host and device paths alternate, `--reps` times each
after one warm-up, the device synchronised before the clock stops; the
medians are end-to-end seconds, file read included.  `decode` is the device
path's stage alone: `decode_chunk` over the file's bytes already in HBM, in
GB/s of input.  The checksum (rows, and the sum of an integer and of a float
column in hundredths) must be the same for both paths.  Prints one JSON
line."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import daft_amd as daft  # noqa: E402
from daft_amd.kernels import jsonl as device_json, native_required  # noqa: E402
from daft_amd.kernels.csv import _upload  # noqa: E402

NAMES = ["l_orderkey", "l_partkey", "l_suppkey", "l_linenumber",
         "l_quantity", "l_extendedprice", "l_discount", "l_tax",
         "l_returnflag", "l_linestatus", "l_shipdate", "l_commitdate",
         "l_receiptdate", "l_shipinstruct", "l_shipmode", "l_comment"]
THREE = ["l_quantity", "l_extendedprice", "l_shipdate"]
POOL = 1 << 14   # distinct records; the file draws from them


def write_file(path: str, rows: int) -> int:
    rng = random.Random(0)

    def date():
        return '"%04d/%02d/%02d"' % (rng.randint(1992, 1998),
                                     rng.randint(1, 12), rng.randint(1, 28))
    words = ["carefully", "final, deposits", 'the \\"quick\\" fox',
             "packages", "sleep\\n", "furiously: {bold}", "caf\\u00e9"]
    plain = [w for w in words if "\\" not in w]
    pool = []
    for i in range(POOL):
        src = words if i % 4 == 0 else plain      # escapes in a quarter
        comment = " ".join(rng.choice(src) for _ in range(rng.randint(2, 5)))
        vals = [str(rng.randrange(1, 6 * 10**8)),
                str(rng.randrange(1, 2 * 10**7)),
                str(rng.randrange(1, 10**6)), str(rng.randint(1, 7)),
                "%d.25" % rng.randint(1, 50),
                "%d.%02d" % (rng.randrange(900, 105000), rng.randrange(100)),
                "0.%02d" % rng.randint(1, 10), "0.%02d" % rng.randint(1, 8),
                '"%s"' % rng.choice("ARN"), '"%s"' % rng.choice("OF"),
                date(), date(), date(),
                '"%s"' % rng.choice(["DELIVER IN PERSON", "COLLECT COD",
                                     "NONE"]),
                '"%s"' % rng.choice(["TRUCK", "MAIL", "REG AIR", "SHIP"]),
                '"%s"' % comment]
        pool.append("{" + ",".join('"%s":%s' % kv
                                   for kv in zip(NAMES, vals)) + "}\n")
    idx = torch.randint(0, POOL, (rows,),
                        generator=torch.Generator().manual_seed(0)).tolist()
    with open(path, "w") as f:
        for a in range(0, rows, 1 << 16):
            f.write("".join(pool[i] for i in idx[a:a + (1 << 16)]))
    return os.path.getsize(path)


def scan(path, columns, device_decode):
    df = daft.read_json(path, device_decode=device_decode)
    if columns:
        df = df.select(*columns)
    parts = df.collect()
    torch.cuda.synchronize()
    return parts


def checksum(parts) -> dict:
    out = parts.to_pydict()
    return {"rows": len(out["l_quantity"]),
            "quantity": sum(round(v * 100) for v in out["l_quantity"]),
            "price": sum(round(v * 100) for v in out["l_extendedprice"])}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_200_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_json.py needs a GPU"
    native_required()
    result = {"rows": args.rows, "reps": args.reps, "queries": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lineitem.jsonl")
        result["file_bytes"] = nbytes = write_file(path, args.rows)
        for name, columns in (("all 16 columns", None),
                              ("3 of 16 columns", THREE)):
            times = {False: [], True: []}
            sums = {}
            for rep in range(args.reps + 1):       # the first is the warm-up
                for dev in (False, True):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    parts = scan(path, columns, dev)
                    dt = time.perf_counter() - t
                    if rep:
                        times[dev].append(dt)
                    elif columns:
                        sums[dev] = checksum(parts)
                    del parts
            host, device = median(times[False]), median(times[True])
            q = {"query": name, "host_s": host, "device_s": device,
                 "ratio": host / device}
            if sums:
                assert sums[False] == sums[True], sums
                q["checksum"] = sums[True]
            result["queries"].append(q)
        # the decode stage alone, over bytes that are in HBM already
        schema = {f.name: f.dtype for f in daft.read_json(path).schema}
        with open(path, "rb") as f:
            buf = f.read()
        assert len(buf) <= device_json.MAX_CHUNK, "lower --rows: one chunk only"
        dev_bytes = _upload(buf, "cuda:0")
        names = list(schema)
        for name, columns in (("decode, all 16 columns", None),
                              ("decode, 3 of 16 columns", THREE)):
            times = []
            for rep in range(args.reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                device_json.decode_chunk(dev_bytes, names, schema, columns,
                                         True)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t)
            result["queries"].append({
                "query": name, "device_s": median(times),
                "input_gb_per_s": nbytes / median(times) / 1e9})
    result["stats"] = {k: v if isinstance(v, int) else len(v)
                       for k, v in device_json.STATS.items()}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Parquet scan: host decode (pyarrow, `device_decode=False`) against device
decode (csrc/parquet.hip) of the same file, in the same run.

  python benchmarks/bench_parquet.py [--rows N] [--reps R] [--out FILE.json]

A lineitem-shaped table of `--rows` rows is written with Snappy in row groups
of 2^21 rows: the 12 fixed-width columns (keys, decimals of two digits, dates),
the 3 low-cardinality strings and a comment column.  Each query reads it
through `daft.read_parquet` on cuda:0 and keeps the batches on the device: all
16 columns, and 3 of them.  Host and device paths alternate, `--reps` times
each after one warm-up, the device synchronised before the clock stops; the
medians are end-to-end seconds, file read included.  `decode` is the device
path's stage alone: `decode` of row-group plans whose bytes are staged in
pinned memory already (the upload is in it, the file read and the page-header
walk are not), in GB/s of compressed input.  The checksum (rows, and the sum
of an integer and of a decimal column) must be the same for both paths.
`stats` counts the column chunks decoded on the device and left to pyarrow
over the whole run.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import daft_amd as daft  # noqa: E402
from daft_amd.kernels import native_required, parquet as device_parquet  # noqa: E402

THREE = ["l_quantity", "l_extendedprice", "l_shipdate"]
ROW_GROUP = 1 << 21


def write_file(path: str, rows: int) -> int:
    import numpy as np
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(0)

    def dec(lo, hi):
        # decimal128 is a little-endian int128: the low limb, and a zero
        limbs = np.stack([rng.integers(lo, hi, rows),
                          np.zeros(rows, np.int64)], axis=1)
        return pa.Array.from_buffers(pa.decimal128(12, 2), rows,
                                     [None, pa.py_buffer(limbs.tobytes())])

    def date():
        return pa.array(rng.integers(8036, 10591, rows).astype(np.int32)) \
            .cast(pa.date32())

    def pick(words):
        return pa.array(np.array(words, dtype=object)[
            rng.integers(0, len(words), rows)])
    words = np.array(["carefully", "final deposits", "the quick fox",
                      "packages", "sleep", "furiously bold", "requests"],
                     dtype=object)
    comment = words[rng.integers(0, 7, rows)] + " " + \
        words[rng.integers(0, 7, rows)] + " " + \
        rng.integers(0, 1 << 20, rows).astype(str).astype(object)
    table = pa.table({
        "l_orderkey": pa.array(np.sort(rng.integers(1, 6 * 10**8, rows))),
        "l_partkey": pa.array(rng.integers(1, 2 * 10**7, rows)),
        "l_suppkey": pa.array(rng.integers(1, 10**6, rows)),
        "l_linenumber": pa.array(rng.integers(1, 8, rows).astype(np.int32)),
        "l_quantity": dec(100, 5001),
        "l_extendedprice": dec(90000, 10500000),
        "l_discount": dec(0, 11),
        "l_tax": dec(0, 9),
        "l_returnflag": pick(["A", "R", "N"]),
        "l_linestatus": pick(["O", "F"]),
        "l_shipdate": date(), "l_commitdate": date(), "l_receiptdate": date(),
        "l_shipinstruct": pick(["DELIVER IN PERSON", "COLLECT COD", "NONE",
                                "TAKE BACK RETURN"]),
        "l_shipmode": pick(["TRUCK", "MAIL", "REG AIR", "SHIP", "AIR", "FOB",
                            "RAIL"]),
        "l_comment": pa.array(comment),
    })
    pq.write_table(table, path, compression="snappy",
                   row_group_size=ROW_GROUP)
    return os.path.getsize(path)


def scan(path, columns, device_decode):
    df = daft.read_parquet(path, device_decode=device_decode)
    if columns:
        df = df.select(*columns)
    parts = df.collect()
    torch.cuda.synchronize()
    return parts


def checksum(parts) -> dict:
    out = parts.to_pydict()
    return {"rows": len(out["l_quantity"]),
            "quantity": sum(int(v * 100) for v in out["l_quantity"]),
            "price": sum(int(v * 100) for v in out["l_extendedprice"])}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_parquet.py needs a GPU"
    native_required()
    device_parquet.STATS.update(device_chunks=0, host_chunks=0, reasons=[])
    result = {"rows": args.rows, "reps": args.reps, "queries": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lineitem.parquet")
        result["file_bytes"] = write_file(path, args.rows)
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
        # the decode stage alone, over bytes that are staged already
        for name, columns in (("decode, all 16 columns", None),
                              ("decode, 3 of 16 columns", THREE)):
            plans = list(device_parquet.host_stage(path, columns))
            nbytes = sum(p.src_bytes for p in plans)
            times = []
            for rep in range(args.reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for p in plans:
                    device_parquet.decode(path, p, "cuda:0")
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t)
            result["queries"].append({
                "query": name, "device_s": median(times),
                "compressed_bytes": nbytes,
                "input_gb_per_s": nbytes / median(times) / 1e9})
    st = device_parquet.STATS
    result["stats"] = {"device_chunks": st["device_chunks"],
                       "host_chunks": st["host_chunks"],
                       "reasons": sorted(set(st["reasons"]))}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

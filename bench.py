"""Flagship benchmark: TPC-H (22 queries) on daft_amd, per BASELINE.json.

  python bench.py --gpus N --steps K --warmup W [--sf SF] [--queries 1,6,...]
                  [--dump-outputs DIR] [--full]

One step = one full pass over the query set on dbgen-equivalent synthetic
data resident in HBM (no network on the bench boxes; generation follows the
TPC-H spec distributions — see benchmarks/tpch/datagen.py).  For N>1 the
driver launches this under torch.distributed.run with one rank per GPU; the
tables are sharded across ranks and exchanges run over RCCL/xGMI.

A plain run sets up, warms up, times the K steps and prints one JSON result
line.  --dump-outputs DIR additionally writes the query results of the last
timed step as DIR/q<NN>__<column>.npy (float64) so two builds can be compared
output for output; the generated tables are a pure function of (sf, world),
so the same arguments give the same inputs on every run.  --full is reserved
for measurements beyond the headline figure; today there are none, so it
changes nothing.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

DUMP_BUDGET_BYTES = 64 << 20    # cap on everything --dump-outputs writes
DUMP_SAMPLE_SEED = 0


def _column_to_f64(values):
    """One to_pydict() column as float64: numbers as they are, dates as days
    since 1970-01-01, strings as the CRC-32 of their UTF-8 bytes, nulls as
    NaN."""
    import datetime as dt
    import zlib
    import numpy as np
    epoch = dt.date(1970, 1, 1)
    out = np.empty(len(values), dtype=np.float64)
    for i, v in enumerate(values):
        if v is None:
            out[i] = np.nan
        elif isinstance(v, (bool, int, float)):
            out[i] = float(v)
        elif isinstance(v, dt.datetime):
            out[i] = v.timestamp()
        elif isinstance(v, dt.date):
            out[i] = float((v - epoch).days)
        elif isinstance(v, str):
            out[i] = float(zlib.crc32(v.encode("utf-8")))
        elif isinstance(v, (bytes, bytearray)):
            out[i] = float(zlib.crc32(bytes(v)))
        else:
            out[i] = float(v)
    return out


def dump_outputs(outputs, out_dir) -> None:
    """Write {qid: collected DataFrame} as out_dir/q<NN>__<column>.npy.  Rows
    stay in the order the query returned them.  If everything together would
    exceed DUMP_BUDGET_BYTES every array is cut to the same fixed, seeded row
    sample (sorted row indices, so order is preserved)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}
    for qi, df in outputs.items():
        for name, values in df.to_pydict().items():
            safe = "".join(c if c.isalnum() or c in "_-" else "_"
                           for c in name)
            arrays["q%02d__%s" % (qi, safe)] = _column_to_f64(values)
    total = sum(a.nbytes for a in arrays.values())
    budget = DUMP_BUDGET_BYTES - 256 * len(arrays)   # room for .npy headers
    if total > budget:
        keep = budget / float(total)
        for key in sorted(arrays):
            a = arrays[key]
            n = int(len(a) * keep)
            # seeded per row count: all columns of one query share the rows
            rng = np.random.default_rng([DUMP_SAMPLE_SEED, len(a)])
            arrays[key] = a[np.sort(rng.choice(len(a), n, replace=False))]
    for key, a in arrays.items():
        np.save(os.path.join(out_dir, key + ".npy"), a)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sf", type=float, default=None,
                    help="TPC-H scale factor (default: 100 on GPU, 0.1 on CPU)")
    ap.add_argument("--queries", type=str, default="all")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write the last timed step's query results as "
                         "DIR/q<NN>__<column>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also run measurements beyond the headline figure "
                         "(none today)")
    args = ap.parse_args()

    import torch
    world = int(os.environ.get("WORLD_SIZE", args.gpus if args.gpus > 1 else 1))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    on_gpu = torch.cuda.is_available()

    dist = None
    if world > 1:
        import torch.distributed as tdist
        dist = tdist
        backend = "nccl" if on_gpu else "gloo"
        if on_gpu:
            local_rank = local_rank % torch.cuda.device_count()
            torch.cuda.set_device(local_rank)
        tdist.init_process_group(backend=backend, rank=rank,
                                 world_size=world)

    sf = args.sf
    if sf is None:
        sf = 100.0 if on_gpu else 0.1
    device = args.device or (f"cuda:{local_rank}" if on_gpu else "cpu")

    import daft_amd
    from daft_amd.kernels import load_native, native_required
    if on_gpu:
        native_required()  # HIP extension is mandatory on GPU

    if world > 1:
        from daft_amd.context import get_context
        from daft_amd.distributed.runner import DistributedRunner
        get_context().set_runner(DistributedRunner(get_context()))

    from benchmarks.tpch import datagen, queries as Q

    if args.queries == "all":
        qids = list(range(1, 23))
    else:
        qids = [int(x) for x in args.queries.split(",")]

    def log(msg):
        if rank == 0:
            print(msg, file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    tables = datagen.dataframes(sf, device=device, rank=rank, world=world)
    if on_gpu:
        torch.cuda.synchronize()
    log(f"[bench] datagen sf={sf} world={world} took "
        f"{time.perf_counter() - t0:.1f}s")

    last_outputs = {}   # qid -> collected result of the most recent pass

    def run_suite():
        per_q = {}
        for qi in qids:
            tq = time.perf_counter()
            out = Q.run_query(qi, tables, sf=sf)
            # force full materialization on-device
            for part in out._result:
                pass
            if on_gpu:
                torch.cuda.synchronize()
            per_q[qi] = time.perf_counter() - tq
            if args.dump_outputs:
                last_outputs[qi] = out
        return per_q

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    for w in range(args.warmup):
        barrier_sync()
        pq = run_suite()
        barrier_sync()
        log(f"[bench] warmup {w}: {sum(pq.values()):.2f}s")

    times = []
    all_per_q = None
    for s in range(args.steps):
        barrier_sync()
        t1 = time.perf_counter()
        per_q = run_suite()
        barrier_sync()
        dt_s = time.perf_counter() - t1
        # max over ranks
        if dist is not None:
            t = torch.tensor([dt_s], dtype=torch.float64,
                             device=device if on_gpu else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_s = float(t.item())
        times.append(dt_s)
        all_per_q = per_q
        log(f"[bench] step {s}: {dt_s:.2f}s")

    if args.dump_outputs:
        # to_pydict() gathers across ranks, so every rank calls it
        if rank == 0:
            dump_outputs(last_outputs, args.dump_outputs)
        else:
            for df in last_outputs.values():
                df.to_pydict()

    value = sum(times) / len(times)
    baseline_s = 785.0  # reference SF100 published total (other hardware)
    result = {
        "metric": "tpch_sf%g_total_runtime_s" % sf,
        "value": round(value, 3),
        "unit": "s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(value * 1000.0, 1),
        "higher_is_better": False,
        "scaling": "strong",
        "vs_baseline": round(value / baseline_s, 4) if sf == 100.0 else None,
        "dtype": "fp64",
        "data": "synthetic (dbgen-equivalent TPC-H, generated in HBM)",
        "config": {
            "model": "TPC-H",
            "queries": qids,
            "scale_factor": sf,
            "global_batch": None,
            "seq_len": None,
            "parallelism": f"dp{world} (sharded tables, RCCL exchanges)"
            if world > 1 else "single-gpu",
            "per_query_s": {f"q{k}": round(v, 3)
                            for k, v in (all_per_q or {}).items()},
        },
    }
    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

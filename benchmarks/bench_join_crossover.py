"""Direct-address join against the hash join as the key range grows.

  python benchmarks/bench_join_crossover.py [--out FILE.json]

The probe side is fixed and the build side is a unique key set spread over
a range of `factor` x probe rows; half the probe keys hit.  Prints one line
per (shape, factor): milliseconds of the hash join and, where the tree has
it, of the native direct-address join (each the median of 5 calls, device
synchronised).  Run it on two builds to compare their hash paths."""
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

SHAPES = [(100_000_000, 100_000), (100_000_000, 10_000_000),
          (20_000_000, 1_000_000)]
FACTORS = [0.25, 1, 2, 4, 8, 16]


def timed(fn, reps=5):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    native_required()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    has_dense = hasattr(rowops, "_dense_key_join_native")
    rows = []
    for n_l, n_r in SHAPES:
        for f in FACTORS:
            rng = int(f * n_l)
            if rng < n_r or rng > rowops._DENSE_JOIN_LIMIT:
                continue
            # unique build keys: a strided walk over the range, shuffled
            step = rng // n_r
            build = torch.arange(n_r, device=dev) * step
            build = build[torch.randperm(n_r, device=dev, generator=g)]
            probe = torch.randint(0, rng, (n_l,), device=dev, generator=g)
            pick = torch.randint(0, n_r, (n_l // 2,), device=dev, generator=g)
            probe[::2][:n_l // 2] = build[pick]
            lk = [Series("k", DataType.int64(), data=probe)]
            rk = [Series("k", DataType.int64(), data=build)]
            row = {"n_l": n_l, "n_r": n_r, "factor": f, "rng": rng,
                   "hash_ms": timed(lambda: rowops._gpu_join(lk, rk, "inner"))}
            if has_dense:
                row["dense_ms"] = timed(lambda: rowops._dense_key_join_native(
                    lk[0], rk[0], "inner", 0, int(build.max().item()) + 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del probe, build, pick, lk, rk
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

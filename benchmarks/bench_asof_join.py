"""As-of join: the native probe path against the per-group host loop it
replaces.

  python benchmarks/bench_asof_join.py [--right-rows-log2 23]
      [--left-rows-log2 20] [--entities 1 100 10000] [--reps 5]
      [--out FILE.json]

Data is made on the device with a fixed seed, shaped like the reference's
as-of benchmark: int64 timestamps clustered around 1,000 centres, and an
entity per row drawn from a Zipf(1.0) distribution (int64 ids here, where the
reference has strings).  `--entities 1` joins without `by`.

For backward and forward, the old loop (kept below as `asof_match_loop`) and
`asof_match` run alternately, each the median of `--reps` device-synchronised
calls after a warm-up, and their outputs are compared.  Nearest has no
counterpart in the loop, so only the new time is printed.  A further line per
entity count splits the new path into group ids, right sort and probe kernel.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from daft_amd.kernels import native_required, rowops  # noqa: E402
from daft_amd.physical import asof  # noqa: E402
from daft_amd.schema import DataType  # noqa: E402
from daft_amd.series import Series  # noqa: E402

DEV = "cuda:0"
TS_MAX = 10 ** 12
N_CLUSTERS = 1000
CLUSTER_WIDTH = 10 ** 6


def _sync_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def make_table(n, entities, gen):
    """(timestamp Series, [entity Series] or [])."""
    centers = torch.randint(0, TS_MAX, (N_CLUSTERS,), device=DEV,
                            generator=gen)
    which = torch.randint(0, N_CLUSTERS, (n,), device=DEV, generator=gen)
    jitter = torch.randint(-CLUSTER_WIDTH, CLUSTER_WIDTH, (n,), device=DEV,
                           generator=gen)
    ts = (centers[which] + jitter).clamp_(0, TS_MAX - 1)
    on = Series("ts", DataType.int64(), data=ts)
    if entities == 1:
        return on, []
    # Zipf(1.0): P(rank r) ~ 1 / r, drawn through the inverse CDF
    w = 1.0 / torch.arange(1, entities + 1, device=DEV, dtype=torch.float64)
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(n, device=DEV, dtype=torch.float64, generator=gen)
    ent = torch.searchsorted(cdf, u).clamp_(max=entities - 1)
    return on, [Series("entity", DataType.int64(), data=ent)]


def asof_match_loop(left_keys, right_keys, left_by, right_by,
                    strategy="backward", allow_exact=True):
    """The path asof_match had before the native probe: sort the right side
    on the device, then one searchsorted per `by` group from a host loop."""
    nl, nr = len(left_keys), len(right_keys)
    dev = left_keys.device
    lk = left_keys.data.to(torch.int64)
    rk = right_keys.data.to(torch.int64)
    if left_by:
        merged = [Series.concat([l, r]) for l, r in zip(left_by, right_by)]
        gids, _reps = rowops.groupby(merged)
        lg, rg = gids[:nl], gids[nl:]
    else:
        lg = torch.zeros(nl, dtype=torch.int64, device=dev)
        rg = torch.zeros(nr, dtype=torch.int64, device=dev)
    rg_series = Series("__g", DataType.int64(), data=rg)
    rperm = rowops.argsort_multi([rg_series, right_keys], [False, False],
                                 [False, False])
    rg_s = rg[rperm]
    rk_s = rk[rperm]
    num_groups = int(torch.maximum(lg.max(), rg.max()).item()) + 1
    counts = torch.bincount(rg_s, minlength=num_groups)
    starts = torch.zeros(num_groups + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=starts[1:])
    out = torch.full((nl,), -1, dtype=torch.int64, device=dev)
    for g in torch.unique(lg).tolist():
        lsel = torch.nonzero(lg == g).reshape(-1)
        a, b = int(starts[g].item()), int(starts[g + 1].item())
        if a == b:
            continue
        seg = rk_s[a:b]
        vals = lk[lsel]
        if strategy == "backward":
            pos = torch.searchsorted(seg, vals, right=allow_exact) - 1
            ok = pos >= 0
        else:
            pos = torch.searchsorted(seg, vals, right=not allow_exact)
            ok = pos < (b - a)
        pos = pos.clamp(0, b - a - 1)
        out[lsel] = torch.where(ok, rperm[a + pos], torch.full_like(pos, -1))
    return out


def bench_split(lk, rk, lb, rb, reps):
    """Median ms of the three stages of asof_match, run one after another."""
    nl, nr = len(lk), len(rk)
    t_gid, t_sort, t_probe = [], [], []
    for _ in range(reps + 1):
        ms, (lg, rg, ng) = _sync_ms(
            lambda: asof._group_ids(lb, rb, nl, nr, lk.device))
        t_gid.append(ms)
        ekl = rowops._order_key_u64(lk).contiguous()
        ekr = rowops._order_key_u64(rk)
        ms, (rk_s, rg_s, rows, seg) = _sync_ms(
            lambda: asof._sort_right(ekr, rg, None, ng))
        t_sort.append(ms)
        lg = lg.contiguous()
        ms, _ = _sync_ms(lambda: asof._probe(ekl, lg, rk_s, rg_s, rows, seg,
                                             0, True, False))
        t_probe.append(ms)
    return {"group_ids_ms": round(_median(t_gid[1:]), 3),
            "right_sort_ms": round(_median(t_sort[1:]), 3),
            "probe_kernel_ms": round(_median(t_probe[1:]), 3)}


def bench_entities(entities, n_left, n_right, reps, emit):
    gen = torch.Generator(device=DEV).manual_seed(42)
    rk, rb = make_table(n_right, entities, gen)
    lk, lb = make_table(n_left, entities, gen)
    base = {"bench": "asof_match", "entities": entities,
            "left_rows": n_left, "right_rows": n_right}
    for strategy in ("backward", "forward"):
        old = lambda: asof_match_loop(lk, rk, lb, rb, strategy)   # noqa: E731
        new = lambda: asof.asof_match(lk, rk, lb, rb, strategy)   # noqa: E731
        _, a = _sync_ms(old)               # warm-up, and the outputs
        _, b = _sync_ms(new)
        same = bool(torch.equal(a, b))
        matched = int((b >= 0).sum().item())
        del a, b
        assert same, f"loop and native outputs differ ({strategy})"
        t_old, t_new = [], []
        for _ in range(reps):              # alternate the two
            t_old.append(_sync_ms(old)[0])
            t_new.append(_sync_ms(new)[0])
        emit(dict(base, strategy=strategy,
                  loop_ms=round(_median(t_old), 3),
                  native_ms=round(_median(t_new), 3),
                  loop_all_ms=[round(t, 3) for t in t_old],
                  native_all_ms=[round(t, 3) for t in t_new],
                  speedup=round(_median(t_old) / _median(t_new), 2),
                  native_within_loop_spread=_median(t_new) <= max(t_old),
                  matched_rows=matched, outputs_equal=same))
    new = lambda: asof.asof_match(lk, rk, lb, rb, "nearest")      # noqa: E731
    times = [_sync_ms(new)[0] for _ in range(reps + 1)][1:]
    emit(dict(base, strategy="nearest", native_ms=round(_median(times), 3),
              native_all_ms=[round(t, 3) for t in times]))
    emit(dict(base, strategy="backward", split=bench_split(lk, rk, lb, rb,
                                                           reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--right-rows-log2", type=int, default=23)
    ap.add_argument("--left-rows-log2", type=int, default=20)
    ap.add_argument("--entities", type=int, nargs="+",
                    default=[1, 100, 10_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    native_required()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for entities in args.entities:
        bench_entities(entities, 1 << args.left_rows_log2,
                       1 << args.right_rows_log2, args.reps, emit)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

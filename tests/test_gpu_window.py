"""Native window frames (csrc/window.hip) against a plain Python loop: for
each partition and row, clamp the frame, collect the non-null inputs and
aggregate them with Python ints and Fractions.  Values are integers within
+-1000 held as int64 or float64, so every partial sum is exact in both and
sum, count, mean, min, max and validity are compared with ==.

The scan works on tiles of T = 1024 sorted positions (WIN_TILE: 256 threads
x 4 positions, a wave covers 256); one block folds 256 tile aggregates per
trip, so 256 * T + 1 rows are the first size at which it loops."""
import functools
import math
import operator
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import col
from daft_amd.functions import dense_rank, rank
from daft_amd.kernels import native_required
from daft_amd.window import Window

DEV = "cuda:0"
T = 1024
UP, UF, CR = (Window.unbounded_preceding, Window.unbounded_following,
              Window.current_row)
# None is the RANGE default: order keys tie in runs of three (o // 3)
FRAMES = [(UP, CR), (CR, UF), (UP, UF), (-3, 0), (-1, 1), (0, 0), (2, 5),
          (-5, -2), (3, 1), (-(T + 1), 0), None]
OPS = ["sum", "count", "mean", "min", "max", "variance"]
OP_CODE = {"sum": 0, "count": 1, "mean": 2, "min": 3, "max": 4,
           "variance": 5}
EPS = 2.0 ** -53
# partition lengths, in sorted order
LAYOUTS = {
    "ones": (1,) * (T + 1),
    "wave-edge": (64, 192, 65),          # boundaries at lane and wave edges
    "tile-edge": (T, 5, T - 5, 1),       # boundaries at T and 2T
    "three-tiles": (3, 3 * T, 7),        # a carry crosses a headless tile
}


def make(lens, seed, nulls):
    """Rows in a shuffled order; sorted position p holds row perm[p]."""
    r = np.random.default_rng(seed)
    n = sum(lens)
    d = {"g": np.repeat(np.arange(len(lens)), lens),
         "o": np.concatenate([np.arange(L) for L in lens]),
         "v": r.integers(-1000, 1001, n),
         "ok": r.random(n) > 0.3 if nulls else np.ones(n, bool)}
    if nulls and len(lens) > 1:
        d["ok"][d["g"] == 1] = False     # a partition with no input at all
    perm = r.permutation(n)
    inv = np.argsort(perm)
    orig = {k: a[inv] for k, a in d.items()}
    return d, orig, perm


def bounds(frame, i, L):
    if frame is None:
        return 0, min(L - 1, i // 3 * 3 + 2)
    s, e = frame
    lo = 0 if s == UP else max(0, i + (0 if s == CR else s))
    hi = L - 1 if e == UF else min(L - 1, i + (0 if e == CR else e))
    return lo, hi


def aggs(xs):
    """Every op over the non-null inputs of one frame."""
    c = len(xs)
    if c == 0:
        return dict.fromkeys(OPS, None) | {"count": 0}
    s, sq = sum(xs), Fraction(sum(map(operator.mul, xs, xs)), c)
    # sumsq/cnt - mean*mean: three roundings, each below an ulp of sumsq/cnt
    var = float(sq - Fraction(s, c) ** 2), 4 * EPS * float(sq)
    return {"sum": s, "count": c, "mean": float(Fraction(s, c)),
            "min": min(xs), "max": max(xs), "variance": var}


@functools.lru_cache(maxsize=None)
def loop_ref(lens, seed, nulls, frame):
    """{op: expected per sorted position} for make(lens, seed, nulls)"""
    d = make(lens, seed, nulls)[0]
    out = {op: [] for op in OPS}
    base = 0
    for L in lens:
        vals = [int(v) if ok else None for v, ok in
                zip(d["v"][base:base + L], d["ok"][base:base + L])]
        for i in range(L):
            lo, hi = bounds(frame, i, L)
            r = aggs([x for x in vals[lo:max(hi + 1, lo)] if x is not None])
            for op in OPS:
                out[op].append(r[op])
        base += L
    return out


def check(got, want, op, what):
    if op != "variance":
        assert got == want, what
        return
    for g, w in zip(got, want):
        assert (g is None) == (w is None), what
        if w is not None:
            assert abs(g - w[0]) <= w[1], (what, g, w)


def native_call(orig, perm, lens, frame, op, dtype=torch.int64):
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)) \
        .to(DEV, dt)
    seg = np.concatenate([[0], np.cumsum(lens)])
    if frame is None:
        codes, peer = (0, 0, 2, 0), dev(orig["o"][perm] % 3 == 0)
    else:
        s, e = frame
        codes = (int(s != UP), 0 if s in (UP, CR) else s,
                 int(e != UF), 0 if e in (UF, CR) else e)
        peer = None
    value, count = native_required().window_agg(
        dev(orig["v"], dtype), dev(orig["ok"]), dev(perm), dev(orig["g"]),
        dev(seg), peer, *codes, OP_CODE[op])
    assert value.shape == count.shape == perm.shape
    assert count.dtype == torch.int64
    return value, count


@pytest.mark.parametrize("dtype", [torch.int64, torch.float64])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_native_layouts_equal_loop(layout, nulls, dtype):
    lens = LAYOUTS[layout]
    d, orig, perm = make(lens, 5, nulls)
    for frame in FRAMES:
        want = loop_ref(lens, 5, nulls, frame)
        for op in OPS:
            value, count = native_call(orig, perm, lens, frame, op, dtype)
            is_f = dtype == torch.float64 or op in ("mean", "variance")
            assert value.dtype == (torch.float64 if is_f and op != "count"
                                   else torch.int64), op
            v, c = value.cpu()[perm].tolist(), count.cpu()[perm].tolist()
            assert c == want["count"], (frame, op)
            got = c if op == "count" else \
                [x if k else None for x, k in zip(v, c)]
            check(got, want[op], op, (frame, op))


def frame_cols(w, frames):
    return {f"{op}{j}": getattr(col("v"), op)().over(
        w if fr is None else w.rows_between(*fr))
        for j, fr in enumerate(frames) for op in OPS}


def run_public(orig, order, frames, as_float):
    conv = float if as_float else int
    df = daft.from_pydict({
        "i": list(range(len(orig["v"]))), "g": orig["g"].tolist(),
        "o": orig["o"].tolist(), "k": (orig["o"] // 3).tolist(),
        "v": [conv(v) if ok else None
              for v, ok in zip(orig["v"], orig["ok"])]}, device=DEV)
    w = Window().partition_by("g").order_by(order)
    return df.with_window_columns(frame_cols(w, frames)).sort("i").to_pydict()


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("lens", [(1,), (63,), (64,), (65,), (T - 1,), (T,),
                                  (T + 1,), (2 * T + 1,), (70, 3, T, 200)],
                         ids=lambda l: "-".join(map(str, l)))
def test_dataframe_equals_loop(lens, as_float):
    nulls = sum(lens) % 2 == 1 and sum(lens) > 1
    d, orig, perm = make(lens, 9, nulls)
    inv = np.argsort(perm)
    for order, frames in (("o", FRAMES[:-1]), ("k", [None])):
        out = run_public(orig, order, frames, as_float)
        for j, fr in enumerate(frames):
            want = loop_ref(lens, 9, nulls, fr)
            for op in OPS:
                check(out[f"{op}{j}"], [want[op][p] for p in inv], op,
                      (fr, op))


def test_large_unbounded_frames():
    n = 256 * T + 1
    lens = [3, 100 * T + 5, 1, n - 100 * T - 9]
    d, orig, perm = make(lens, 3, True)
    v = np.where(d["ok"], d["v"], 0)
    big = np.iinfo(np.int64).max
    m = np.where(d["ok"], d["v"], big)
    c = d["ok"].astype(np.int64)
    want = {}
    for frame, view in (((UP, CR), slice(None)),
                        ((CR, UF), slice(None, None, -1))):
        parts = [(v[a:b][view], c[a:b][view], m[a:b][view]) for a, b in
                 zip(np.cumsum([0] + lens[:-1]), np.cumsum(lens))]
        for op, k, f in (("sum", 0, np.cumsum), ("count", 1, np.cumsum),
                         ("min", 2, np.minimum.accumulate)):
            want[frame, op] = np.concatenate([f(p[k])[view] for p in parts])
    for (frame, op), w in want.items():
        value, count = native_call(orig, perm, lens, frame, op)
        has = want[frame, "count"] > 0
        assert np.array_equal(count.cpu().numpy()[perm],
                              want[frame, "count"]), (frame, op)
        assert np.array_equal(value.cpu().numpy()[perm][has], w[has]), \
            (frame, op)


def test_float_sum_order_bound():
    lens = [T + 300, 77]
    d, orig, perm = make(lens, 4, False)
    x = np.random.default_rng(8).standard_normal(sum(lens))   # sorted space
    orig = dict(orig, v=x[np.argsort(perm)])
    for frame in [(UP, CR), (CR, UF), (-50, 49), (-(T + 1), 0)]:
        value, _ = native_call(orig, perm, lens, frame, "sum", torch.float64)
        got, base = value.cpu()[perm].tolist(), 0
        for L in lens:
            for i in range(L):
                lo, hi = bounds(frame, i, L)
                xs = x[base + lo:base + max(hi + 1, lo)].tolist()
                assert abs(got[base + i] - math.fsum(xs)) <= \
                    len(xs) * EPS * math.fsum(map(abs, xs)), (frame, i)
            base += L


@pytest.mark.parametrize("op", ["min", "max"])
def test_nan_propagates(op):
    v = [1.0, 5.0, float("nan"), 2.0, 7.0, 3.0, 4.0, 0.0]
    df = daft.from_pydict({"o": list(range(8)), "v": v}, device=DEV)
    w = Window().order_by("o").rows_between(-1, 1)
    out = df.with_window_columns(
        {"r": getattr(col("v"), op)().over(w)}).sort("o").to_pydict()["r"]
    pick = min if op == "min" else max
    for i, r in enumerate(out):
        xs = v[max(0, i - 1):i + 2]
        if any(x != x for x in xs):
            assert r != r, i
        else:
            assert r == pick(xs), i


def test_rank_and_dense_rank():
    lens = [T + 7, 3, T - 9]                      # 2T + 1 rows
    d, orig, perm = make(lens, 6, False)
    keys = d["v"] % 5                             # heavy ties
    df = daft.from_pydict({"i": list(range(len(perm))),
                           "g": orig["g"].tolist(),
                           "k": keys[np.argsort(perm)].tolist()}, device=DEV)
    w = Window().partition_by("g").order_by("k")
    out = df.with_window_columns({"r": rank().over(w),
                                  "d": dense_rank().over(w)}) \
        .sort("i").to_pydict()
    base = 0
    for L in lens:
        ks = keys[base:base + L].tolist()
        distinct = sorted(set(ks))
        for p in range(base, base + L):
            k, row = ks[p - base], perm[p]
            assert out["r"][row] == 1 + sum(x < k for x in ks), p
            assert out["d"][row] == 1 + distinct.index(k), p
        base += L


def test_int64_running_sum_is_exact():
    # three values near 2^58 per partition: exact in int64, not in float64
    n, per = 60, 3
    r = np.random.default_rng(2)
    v = ((1 << 58) + r.integers(1, 1000, n)).tolist()
    df = daft.from_pydict({"g": [i // per for i in range(n)],
                           "o": list(range(n)), "v": v}, device=DEV)
    w = Window().partition_by("g").order_by("o").rows_between(UP, CR)
    out = df.with_window_columns({"s": col("v").sum().over(w)}) \
        .sort("o").to_pydict()["s"]
    assert out == [sum(v[i // per * per:i + 1]) for i in range(n)]


def test_small_partition_after_huge_one_keeps_digits():
    parts, per = 12, 40
    vals = [1e18 if g % 2 == 0 else 0.1 for g in range(parts)
            for _ in range(per)]
    df = daft.from_pydict({"g": [i // per for i in range(parts * per)],
                           "o": list(range(parts * per)), "v": vals},
                          device=DEV)
    w = Window().partition_by("g").order_by("o").rows_between(UP, CR)
    out = df.with_window_columns({"s": col("v").sum().over(w)}) \
        .sort("o").to_pydict()["s"]
    for g in range(1, parts, 2):
        for i in range(per):
            xs = [0.1] * (i + 1)
            assert abs(out[g * per + i] - math.fsum(xs)) <= \
                len(xs) * EPS * math.fsum(xs), (g, i)


def test_argument_errors():
    lens = [5, 4]
    d, orig, perm = make(lens, 1, True)
    nat = native_required()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ok = dict(v=t(orig["v"]), ok=t(orig["ok"]), perm=t(perm), g=t(orig["g"]),
              seg=t(np.array([0, 5, 9])), peer=None, lk=0, lo=0, hk=1, ho=0,
              op=0)

    def call(**kw):
        a = dict(ok, **kw)
        return nat.window_agg(a["v"], a["ok"], a["perm"], a["g"], a["seg"],
                              a["peer"], a["lk"], a["lo"], a["hk"], a["ho"],
                              a["op"])
    assert call()[0].shape == (9,)
    for kw in [dict(v=ok["v"].to(torch.int32)), dict(v=ok["v"].cpu()),
               dict(v=ok["v"][:-1]), dict(ok=ok["ok"].to(torch.uint8)),
               dict(perm=ok["perm"].cpu()), dict(g=ok["g"][:-1]),
               dict(seg=ok["seg"].to(torch.int32)), dict(op=7), dict(lk=2),
               dict(hk=3), dict(hk=2), dict(lk=1, hk=2, peer=ok["ok"]),
               dict(v=None), dict(perm=ok["perm"].reshape(1, -1))]:
        with pytest.raises(RuntimeError, match="window_agg"):
            call(**kw)
    e = ok["perm"][:0]
    value, count = nat.window_agg(e, None, e, e, ok["seg"][:1], None, 0, 0, 1,
                                  0, 0)
    assert value.shape == count.shape == (0,) and value.is_cuda

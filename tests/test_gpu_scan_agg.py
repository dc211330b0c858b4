"""Filter -> Aggregate in one JIT kernel (fused_agg_jit) against an exact
host oracle and against the general path, with a spy on the binding telling
which of the two produced the result."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

from daft_amd import DataType, Series, col
from daft_amd.io import from_recordbatches
from daft_amd.kernels import native_required
from daft_amd.recordbatch import RecordBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG_N = 2048 * 1024 + 1025      # past the capped grid: grid-stride regime
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, BIG_N]
SPECIALS = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1.5, -2.5]


def _dict(name, card, codes):
    vocab = Series.from_pylist(name, [f"{name}{i}" for i in range(card)],
                               DataType.string())
    return Series.make_dict(name, vocab, codes.to(torch.int32))


@functools.lru_cache(maxsize=None)
def _corpus(n):
    """(device batch, numpy columns).  Built once per size and never
    changed."""
    g = torch.Generator().manual_seed(1000 + n)

    def ri(hi):
        return torch.randint(0, hi, (n,), generator=g)

    x = torch.rand(n, generator=g, dtype=torch.float64) * 200 - 100
    y = torch.rand(n, generator=g, dtype=torch.float64) * 1e6
    yv = torch.rand(n, generator=g) > 0.1
    f = (torch.rand(n, generator=g) * 8 - 4).to(torch.float32)
    z = torch.tensor(SPECIALS, dtype=torch.float64)[ri(len(SPECIALS))]
    p = torch.rand(n, generator=g, dtype=torch.float64)
    pv = torch.rand(n, generator=g) > 0.2
    i = ri(1000) - 500
    ku = torch.tensor([1, 3])[ri(2)]
    cols = [
        Series("x", DataType.float64(), data=x),
        Series("y", DataType.float64(), data=y, validity=yv),
        Series("f", DataType.float32(), data=f),
        Series("z", DataType.float64(), data=z),
        Series("p", DataType.float64(), data=p),
        Series("pn", DataType.float64(), data=p.clone(), validity=pv),
        Series("i", DataType.int64(), data=i),
        _dict("k1", 1, ri(1)), _dict("ka", 3, ri(3)), _dict("kb", 2, ri(2)),
        _dict("ku", 5, ku), _dict("kw", 1024, ri(1024)),
        _dict("kx", 683, ri(683)),
        Series("b", DataType.bool(), data=ri(2).to(torch.bool)),
    ]
    s = Series.from_pylist("s", [f"s{int(v)}" for v in ri(3)],
                           DataType.string())
    batch = RecordBatch(cols + [s], num_rows=n)
    host = {c.name: c.data.numpy() for c in cols}
    host["y_valid"] = yv.numpy()
    host["pn_valid"] = pv.numpy()
    return batch.to(DEV), host


class _Spy:
    def __init__(self, monkeypatch):
        native = native_required()
        self.calls = 0
        real = native.fused_agg_jit

        def call(*a):
            self.calls += 1
            return real(*a)
        monkeypatch.setattr(native, "fused_agg_jit", call)


def _collect(batch, pred, keys, aggs):
    df = from_recordbatches([batch])
    if pred is not None:
        df = df.where(pred)
    df = df.groupby(*keys).agg(*aggs) if keys else df.agg(*aggs)
    parts = df.collect()._result
    return RecordBatch.concat(parts) if len(parts) != 1 else parts[0]


def _both(n, pred, keys, aggs, monkeypatch, fused=True):
    """Result of the fused path (or of whatever runs when `fused` is False)
    and of the general path, checked equal in schema, row order, validity,
    and bit for bit in everything but sums and means."""
    batch, host = _corpus(n)
    spy = _Spy(monkeypatch)
    new = _collect(batch, pred, keys, aggs)
    assert spy.calls == (1 if fused else 0), spy.calls
    monkeypatch.setenv("DAFT_AMD_DISABLE_FUSED_AGG", "1")
    old = _collect(batch, pred, keys, aggs)
    monkeypatch.delenv("DAFT_AMD_DISABLE_FUSED_AGG")
    assert spy.calls == (1 if fused else 0), spy.calls
    assert len(new) == len(old)
    assert [(c.name, c.dtype) for c in new.columns] == \
        [(c.name, c.dtype) for c in old.columns]
    out = {}
    for cn, co in zip(new.columns, old.columns):
        a, b = cn.to_pylist(), co.to_pylist()
        assert [v is None for v in a] == [v is None for v in b], cn.name
        out[cn.name] = (a, b)
    return out, host


def _bits(v):
    return None if v is None else struct.pack("d", float(v))


def _same_bits(pair):
    a, b = pair
    assert [_bits(v) for v in a] == [_bits(v) for v in b], (a, b)


def _groups(host, n, keys, cards, passes):
    """Live groups in ascending packed-code order: [(codes, row mask)]."""
    packed = np.zeros(n, dtype=np.int64)
    for k, c in zip(keys, cards):
        packed = packed * c + host[k].astype(np.int64)
    live = np.unique(packed[passes]) if keys else [0]
    out = []
    for g in live:
        codes, rest = [], int(g)
        for c in reversed(cards):
            codes.append(rest % c)
            rest //= c
        out.append((codes[::-1], passes & (packed == g)))
    return out


def _check_sum(got, rows, vals):
    """|got - fsum| <= (m - 1) * 2^-53 * sum|x|: the a-priori bound for a
    sum of m terms in any order."""
    v = vals[rows].astype(np.float64)
    m = len(v)
    if m == 0:
        assert got is None
        return 0.0, 0
    bound = (m - 1) * 2.0 ** -53 * math.fsum(np.abs(v).tolist())
    exact = math.fsum(v.tolist())
    print("sum m=%d err=%.3e bound=%.3e" % (m, abs(got - exact), bound))
    assert abs(got - exact) <= bound, (got, exact, bound)
    return bound, m


Q1_AGGS = [col("x").sum().alias("sx"), col("y").sum().alias("sy"),
           (col("x") * (1 - col("p"))).sum().alias("sxp"),
           col("x").mean().alias("mx"), col("y").mean().alias("my"),
           col("x").count().alias("cx"), col("y").count().alias("cy"),
           col("x").min().alias("lo"), col("y").max().alias("hi")]

KEYSETS = {"none": ([], []), "card1": (["k1"], [1]),
           "3x2": (["ka", "kb"], [3, 2]), "unused": (["ku"], [5]),
           "bool": (["b"], [2])}
# "none" is a product so that no column statistic can prune the scan away
PREDS = {"absent": None, "all": col("p") >= 0.0,
         "none": col("p") * col("p") < 0.0,
         "2pct": col("p") < 0.02, "nulls": col("pn") < 0.5}


def _pass_mask(host, n, pname):
    if pname in ("absent", "all"):
        return np.ones(n, dtype=bool)
    if pname == "none":
        return np.zeros(n, dtype=bool)
    if pname == "2pct":
        return host["p"] < 0.02
    return (host["pn"] < 0.5) & host["pn_valid"]


def _check_q1_shape(n, kname, pname, monkeypatch):
    keys, cards = KEYSETS[kname]
    out, host = _both(n, PREDS[pname], keys, Q1_AGGS, monkeypatch)
    passes = _pass_mask(host, n, pname)
    groups = _groups(host, n, keys, cards, passes)
    if not keys and not passes.any():
        # empty global aggregate: one row, counts 0, the rest null
        assert out["cx"][0] == [0] and out["cy"][0] == [0]
        for name in ("sx", "sy", "sxp", "mx", "my", "lo", "hi"):
            assert out[name][0] == [None], name
        return
    assert len(out["cx"][0]) == len(groups)
    for r, (codes, rows) in enumerate(groups):
        for k, c in zip(keys, codes):
            want = bool(c) if k == "b" else f"{k}{c}"
            assert out[k][0][r] == want, (k, r)
        rows_y = rows & host["y_valid"]
        assert out["cx"][0][r] == int(rows.sum())
        assert out["cy"][0][r] == int(rows_y.sum())
        bx, mx_ = _check_sum(out["sx"][0][r], rows, host["x"])
        by, my_ = _check_sum(out["sy"][0][r], rows_y, host["y"])
        _check_sum(out["sxp"][0][r], rows, host["x"] * (1 - host["p"]))
        for name, vals, rws, b, m in (("mx", host["x"], rows, bx, mx_),
                                      ("my", host["y"], rows_y, by, my_)):
            got = out[name][0][r]
            if m == 0:
                assert got is None
                continue
            exact = math.fsum(vals[rws].tolist()) / m
            # the sum's bound over the count, plus one rounding
            assert abs(got - exact) <= b / m + abs(exact) * 2.0 ** -53, name
        assert out["lo"][0][r] == host["x"][rows].min()
        if my_:
            assert out["hi"][0][r] == host["y"][rows_y].max()
        else:
            assert out["hi"][0][r] is None
    _same_bits(out["lo"])
    _same_bits(out["hi"])
    for name in ["cx", "cy"] + keys:
        assert out[name][0] == out[name][1], name


@pytest.mark.parametrize("n", SIZES)
def test_sizes_two_keys_with_predicate(n, monkeypatch):
    _check_q1_shape(n, "3x2", "nulls", monkeypatch)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_global(n, monkeypatch):
    _check_q1_shape(n, "none", "2pct" if n > 4000 else "nulls", monkeypatch)


@pytest.mark.parametrize("kname", list(KEYSETS))
@pytest.mark.parametrize("pname", list(PREDS))
def test_keys_and_predicates(kname, pname, monkeypatch):
    _check_q1_shape(4097, kname, pname, monkeypatch)


def test_empty_batch_takes_the_general_path(monkeypatch):
    batch, _ = _corpus(63)
    spy = _Spy(monkeypatch)
    out = _collect(batch.slice(0, 0), col("p") < 0.5, ["ka"],
                   [col("x").sum().alias("sx")])
    assert spy.calls == 0 and len(out) == 0


@pytest.mark.parametrize("n", [257, BIG_N])
def test_specials_under_min_max(n, monkeypatch):
    """NaN, +-inf and -0.0: order-sensitive outcomes equal the general
    path's bit for bit."""
    aggs = [col("z").min().alias("lo"), col("z").max().alias("hi"),
            col("z").count().alias("c")]
    for keys in ([], ["ka", "kb"]):
        out, _ = _both(n, col("p") < 0.7, keys, aggs, monkeypatch)
        _same_bits(out["lo"])
        _same_bits(out["hi"])
        assert out["c"][0] == out["c"][1]
        if not keys:
            # IEEE total order: -inf lowest, NaN highest
            assert out["lo"][0] == [float("-inf")]
            assert math.isnan(out["hi"][0][0])


def test_float32_input_and_shared_expression(monkeypatch):
    n = 4097
    e = col("f") * col("f")
    aggs = [e.sum().alias("s"), e.mean().alias("m"), e.count().alias("c"),
            col("f").min().alias("lo")]
    out, host = _both(n, col("p") < 0.5, ["ka"], aggs, monkeypatch)
    passes = host["p"] < 0.5
    sq = (host["f"] * host["f"]).astype(np.float32)
    for r, (_codes, rows) in enumerate(_groups(host, n, ["ka"], [3], passes)):
        v = sq[rows].astype(np.float64)
        m = len(v)
        total = math.fsum(v.tolist())
        b = (m - 1) * 2.0 ** -53 * math.fsum(np.abs(v).tolist())
        # a float32 sum is accumulated in f64 and stored as float32: the
        # any-order bound plus that one rounding
        assert abs(out["s"][0][r] - total) <= b + abs(total) * 2.0 ** -24
        exact = total / m
        assert abs(out["m"][0][r] - exact) <= b / m + abs(exact) * 2.0 ** -53
        assert out["c"][0][r] == m
        assert out["lo"][0][r] == host["f"][rows].min()
    _same_bits(out["lo"])


def test_slot_bound(monkeypatch):
    """1024 groups x 2 aggregates = 2048 slots is fused (the LDS-atomic
    skeleton); 683 x 3 = 2049 is not."""
    n = BIG_N
    aggs = [col("x").sum().alias("s"), col("y").max().alias("hi")]
    out, host = _both(n, col("p") < 0.5, ["kw"], aggs, monkeypatch)
    passes = host["p"] < 0.5
    groups = _groups(host, n, ["kw"], [1024], passes)
    assert len(out["s"][0]) == len(groups) == 1024
    for r, (_codes, rows) in enumerate(groups):
        _check_sum(out["s"][0][r], rows, host["x"])
        rows_y = rows & host["y_valid"]
        assert out["hi"][0][r] == host["y"][rows_y].max()
    _same_bits(out["hi"])
    aggs3 = aggs + [col("x").count().alias("c")]
    out, _ = _both(n, col("p") < 0.5, ["kx"], aggs3, monkeypatch, fused=False)
    assert len(out["s"][0]) == 683


def test_medium_group_count_takes_the_lds_path(monkeypatch):
    """3 x 2 x 5 = 30 groups x 2 accumulators is past the register
    skeleton's 48 slots."""
    n = 4097
    aggs = [col("x").sum().alias("s"), col("y").sum().alias("sy"),
            col("y").count().alias("c")]
    keys, cards = ["ka", "kb", "ku"], [3, 2, 5]
    out, host = _both(n, col("pn") < 0.5, keys, aggs, monkeypatch)
    passes = _pass_mask(host, n, "nulls")
    groups = _groups(host, n, keys, cards, passes)
    assert len(out["s"][0]) == len(groups)
    for r, (_codes, rows) in enumerate(groups):
        _check_sum(out["s"][0][r], rows, host["x"])
        _check_sum(out["sy"][0][r], rows & host["y_valid"], host["y"])
        assert out["c"][0][r] == int((rows & host["y_valid"]).sum())


@pytest.mark.parametrize("keys,aggs", [
    (["ka"], [col("i").sum().alias("s"), col("x").sum().alias("sx")]),
    (["s"], [col("x").sum().alias("sx"), col("x").count().alias("c")]),
])
def test_ineligible_shapes_fall_back(keys, aggs, monkeypatch):
    n = 4097
    out, host = _both(n, col("p") < 0.5, keys, aggs, monkeypatch,
                      fused=False)
    # both runs are the general path, whose float sums depend on the order
    # its atomics land in: two any-order sums of one group's m <= n terms
    # differ by at most 2 (m - 1) 2^-53 sum|x|
    bound = 2 * n * 2.0 ** -53 * math.fsum(
        np.abs(host["x"][host["p"] < 0.5]).tolist())
    for name, (a, b) in out.items():
        if name == "sx":
            assert all(abs(u - v) <= bound for u, v in zip(a, b)), name
        else:
            assert a == b, name

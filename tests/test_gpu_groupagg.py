"""Native grouped-aggregation entry points (csrc/groupagg.hip) against a
numpy reference computed on the host.

Inputs are chosen so equality is exact and no tolerance is needed: f64
values are k/1024 with |k| < 2^20 and n <= 2^17, so every partial sum is
exactly representable and any atomic order gives the same bits (checked on
the host, forwards vs a random permutation, before anything is launched);
i64 sums use |v| < 2^40.  Min/max are compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from daft_amd.kernels import (AGG_COUNT, AGG_MAX, AGG_MIN, AGG_SUM,
                              native_required)

DEV = "cuda:0"
I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min
_SIGN = np.uint64(1 << 63)


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


# ---------------------------------------------------------------------------
# numpy reference
# ---------------------------------------------------------------------------

def _order_key(x):
    """f64 -> u64 key whose unsigned order is -NaN < -inf < -0.0 < +0.0 <
    +inf < +NaN: sign ? ~bits : bits | 1<<63."""
    b = x.view(np.uint64)
    return np.where((b & _SIGN) != 0, ~b, b | _SIGN)


def _from_order_key(k):
    return np.where((k & _SIGN) != 0, k ^ _SIGN, ~k).view(np.float64)


def _ref(gids, G, vals, valid, op):
    """(out[G] or None for count, cnt[G]) with the empty-group results:
    0 for sum, INT64_MAX/INT64_MIN for i64 min/max, 0.0 for f64 min/max."""
    keep = np.ones(len(gids), bool) if valid is None else valid
    g = gids[keep]
    cnt = np.zeros(G, np.int64)
    np.add.at(cnt, g, 1)
    if op == AGG_COUNT:
        return None, cnt
    v = vals[keep]
    if op == AGG_SUM:
        out = np.zeros(G, vals.dtype)
        np.add.at(out, g, v)
    elif vals.dtype == np.int64:
        out = np.full(G, I64_MAX if op == AGG_MIN else I64_MIN, np.int64)
        (np.minimum if op == AGG_MIN else np.maximum).at(out, g, v)
    else:
        key = np.full(G, ~np.uint64(0) if op == AGG_MIN else np.uint64(0))
        (np.minimum if op == AGG_MIN else np.maximum).at(
            key, g, _order_key(v))
        out = np.where(cnt > 0, _from_order_key(key), 0.0)
    return out, cnt


@functools.lru_cache(maxsize=None)
def _inputs(n, G, seed=0):
    """gids, a validity mask, and per dtype one value array for sums and
    one (with the extreme values) for min/max.  With G >= 3 group G-2 never
    occurs and every row of group 1 is invalid under the mask."""
    rng = np.random.default_rng(1000 * G + n + seed)
    gids = rng.integers(0, G, n)
    valid = rng.random(n) > 0.15
    if G >= 3:
        gids[gids == G - 2] = G - 1
        valid[gids == 1] = False
    f_sum = rng.integers(-(1 << 20) + 1, 1 << 20, n) / 1024.0
    f_mm = f_sum.copy()
    i_sum = rng.integers(-(1 << 40) + 1, 1 << 40, n)
    i_mm = rng.integers(-(1 << 62), 1 << 62, n)
    if n > 8:
        f_mm[np.flatnonzero(gids == 0)[0::2]] = -0.0   # group 0: only zeros
        f_mm[np.flatnonzero(gids == 0)[1::2]] = 0.0
        f_mm[3], f_mm[5] = np.inf, -np.inf
        i_mm[2], i_mm[7] = I64_MIN + 1, I64_MAX - 1
    # sums must not depend on accumulation order: forwards == permuted
    perm = rng.permutation(n)
    for v in (f_sum, i_sum):
        a, _ = _ref(gids, G, v, None, AGG_SUM)
        b, _ = _ref(gids[perm], G, v[perm], None, AGG_SUM)
        assert a.tobytes() == b.tobytes()
    vals = {"f64": {AGG_SUM: f_sum, AGG_MIN: f_mm, AGG_MAX: f_mm},
            "i64": {AGG_SUM: i_sum, AGG_MIN: i_mm, AGG_MAX: i_mm}}
    return gids, valid, vals


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mask_arg(valid):
    return _dev(valid) if valid is not None else \
        torch.empty(0, dtype=torch.bool, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------------------
# single-column sum/min/max/count
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [0, 1, 70_001])
@pytest.mark.parametrize("G", [1, 5, 4096, 4097])
@pytest.mark.parametrize("dt", ["f64", "i64"])
def test_grouped_agg_matches_numpy(dt, G, n, masked):
    nat = native_required()
    gids, valid, vals = _inputs(n, G)
    valid = valid if masked else None
    for op in (AGG_SUM, AGG_MIN, AGG_MAX):
        v = vals[dt][op]
        want, want_cnt = _ref(gids, G, v, valid, op)
        out, cnt = nat.grouped_agg(_dev(gids), G, _dev(v), _mask_arg(valid),
                                   op)
        assert out.dtype == (torch.float64 if dt == "f64" else torch.int64)
        assert np.array_equal(cnt.cpu().numpy(), want_cnt), op
        got = out.cpu().numpy()
        if op == AGG_SUM:
            assert np.array_equal(got, want), op
        else:
            assert np.array_equal(_bits(got), _bits(want)), op
    if G >= 3 and n > 8:
        # the never-seen group (and, masked, the all-invalid one) is empty
        assert want_cnt[G - 2] == 0 and (not masked or want_cnt[1] == 0)


def test_grouped_agg_f64_nan_orders_above_inf():
    nat = native_required()
    n, G = 70_001, 5
    gids, _, vals = _inputs(n, G)
    v = vals["f64"][AGG_MAX].copy()
    v[np.flatnonzero(gids == 2)[0]] = np.nan     # positive quiet NaN
    v[np.flatnonzero(gids == 2)[1]] = np.inf
    for op in (AGG_MIN, AGG_MAX):
        want, want_cnt = _ref(gids, G, v, None, op)
        out, cnt = nat.grouped_agg(_dev(gids), G, _dev(v), _mask_arg(None),
                                   op)
        assert np.array_equal(cnt.cpu().numpy(), want_cnt)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), op
    assert np.isnan(want[2])        # max of that group is the NaN


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [0, 1, 70_001])
@pytest.mark.parametrize("G", [8192, 8193])
def test_grouped_count_matches_numpy(G, n, masked):
    gids, valid, _ = _inputs(n, G)
    valid = valid if masked else None
    _, want = _ref(gids, G, None, valid, AGG_COUNT)
    got = native_required().grouped_count(_dev(gids), G, _mask_arg(valid))
    assert got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------
# multi-column: ops [sum, min, max, count], out[a*G + g]
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("count_masked", [False, True])
@pytest.mark.parametrize("G,n", [(512, 70_001), (513, 70_001), (1, 70_001),
                                 (512, 0), (513, 0)])
def test_grouped_multi_agg_matches_numpy(G, n, count_masked):
    nat = native_required()
    gids, valid, vals = _inputs(n, G)
    f_sum, f_mm = vals["f64"][AGG_SUM], vals["f64"][AGG_MIN]
    ops = [AGG_SUM, AGG_MIN, AGG_MAX, AGG_COUNT]
    cols = [(f_sum, valid), (f_mm, None), (f_mm, valid),
            (None, valid if count_masked else None)]
    datas = [_dev(d) if d is not None else
             torch.empty(0, dtype=torch.float64, device=DEV)
             for d, _ in cols]
    valids = [_dev(v) if v is not None else None for _, v in cols]
    out, cnt = nat.grouped_multi_agg(_dev(gids), G, datas, valids, ops)
    assert out.dtype == torch.float64 and cnt.dtype == torch.int64
    assert out.numel() == 4 * G and cnt.numel() == 4 * G
    out = out.cpu().numpy()
    cnt = cnt.cpu().numpy()
    for a, ((d, v), op) in enumerate(zip(cols, ops)):
        want, want_cnt = _ref(gids, G, d, v, op)
        assert np.array_equal(cnt[a * G:(a + 1) * G], want_cnt), a
        got = out[a * G:(a + 1) * G]
        if op == AGG_COUNT:
            assert not got.any(), a          # count slots carry no value
        elif op == AGG_SUM:
            assert np.array_equal(got, want), a
        else:
            assert np.array_equal(_bits(got), _bits(want)), a

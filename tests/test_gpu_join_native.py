"""Native join kernels (csrc/join.hip) against the host paths of rowops.

Direct-address joins must return element for element what the torch code of
`_dense_key_join` returns on the CPU.  Hash joins (forced with string keys)
must return the pairs of `_cpu_join` as a multiset, with lidx ascending."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from daft_amd.kernels import native_required, rowops
from daft_amd.schema import DataType
from daft_amd.series import Series

DEV = "cuda:0"
BIG = 2048 * 256 + 1   # many blocks, ragged last block
# The direct-address fill pass works in tiles of 4 x 256 rows and a block's
# chunk is ceil(n / 2048) rounded up to whole tiles: above 2048 * 1024 rows
# every chunk holds two tiles, so the running output base is carried from one
# tile to the next; the last block is ragged.
TWO_TILES = 2048 * 1024 + 1
DENSE_MODES = ("inner", "left", "semi", "anti")
KEY_TYPES = {
    "int64": (DataType.int64, torch.int64),
    "int32": (DataType.int32, torch.int32),
    "date": (DataType.date, torch.int32),
}


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    native_required()


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the joins that really went through the direct-address kernels."""
    calls = []
    orig = rowops._dense_key_join_native

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(rowops, "_dense_key_join_native", spy)
    return calls


def _series(kind, values, valid=None):
    mk, tdt = KEY_TYPES[kind]
    return Series("k", mk(), data=torch.as_tensor(values, dtype=tdt),
                  validity=None if valid is None else torch.as_tensor(valid))


def _check_dense(l, r, how, native_calls):
    want = rowops._dense_key_join([l], [r], how)
    assert want is not None
    before = len(native_calls)
    got = rowops._dense_key_join([l.to(DEV)], [r.to(DEV)], how)
    assert native_calls[before:] == [True]
    for g, w, name in zip(got, want, ("lidx", "ridx")):
        assert g.dtype == torch.int64 and g.is_cuda, name
        assert torch.equal(g.cpu(), w), (how, name)


@functools.lru_cache(maxsize=None)
def _dense_case(kind, n_l, n_r):
    """Sparse unique build keys over a range that starts below zero; probe
    keys spill over both ends, hit both ends exactly, ~10 % are null."""
    g = np.random.default_rng([n_l, n_r])
    if n_r == 1:
        build = np.array([-7])           # rng == 1
    else:
        build = g.permutation(np.arange(-500, 2500))[:n_r]
        build[:2] = (-500, 2499)
        build = np.unique(build)
        g.shuffle(build)
    mn, mx = int(build.min()), int(build.max())
    probe = g.integers(mn - 40, mx + 41, n_l)
    edge = (mn, mx, mn - 1, mx + 1)
    for j in range(min(n_l, 4)):
        probe[(j * 97) % n_l] = edge[j]
    valid = g.random(n_l) >= 0.1
    return _series(kind, probe, valid), _series(kind, build)


@pytest.mark.parametrize("n_r", [1, 1000])
@pytest.mark.parametrize("n_l", [1, 63, 64, 65, 255, 256, 257, BIG])
@pytest.mark.parametrize("kind", list(KEY_TYPES))
def test_dense_matches_cpu(kind, n_l, n_r, native_calls):
    l, r = _dense_case(kind, n_l, n_r)
    for how in DENSE_MODES:
        _check_dense(l, r, how, native_calls)


@pytest.mark.parametrize("kind", ["int64", "int32"])
def test_dense_two_tiles_per_chunk(kind, native_calls):
    l, r = _dense_case(kind, TWO_TILES, 1000)
    for how in DENSE_MODES:
        _check_dense(l, r, how, native_calls)


@pytest.mark.parametrize("n_l", [257, BIG])
@pytest.mark.parametrize("kind", ["int64", "int32"])
def test_dense_all_miss_and_all_hit(kind, n_l, native_calls):
    g = np.random.default_rng(n_l)
    r = _series(kind, g.permutation(np.arange(100, 1100)))
    hit = _series(kind, g.integers(100, 1100, n_l))
    miss = _series(kind, np.where(g.random(n_l) < 0.5, 99, 1100))
    for how in DENSE_MODES:
        _check_dense(hit, r, how, native_calls)
        _check_dense(miss, r, how, native_calls)
    li, _ = rowops._dense_key_join([miss.to(DEV)], [r.to(DEV)], "inner")
    assert li.numel() == 0
    li, _ = rowops._dense_key_join([hit.to(DEV)], [r.to(DEV)], "anti")
    assert li.numel() == 0


def test_dense_no_validity_and_right_outer(native_calls):
    """No probe validity at all, and the torch tail of right/outer joins on
    top of the native left join."""
    g = np.random.default_rng(5)
    r = _series("int64", g.permutation(np.arange(-50, 250))[:200])
    l = _series("int64", g.integers(-80, 280, 1000))
    for how in DENSE_MODES + ("right", "outer"):
        _check_dense(l, r, how, native_calls)


def _sorted_pairs(li, ri):
    li, ri = li.cpu().numpy(), ri.cpu().numpy()
    order = np.lexsort((ri, li))
    return li[order], ri[order]


def _check_pairs(got, want, how):
    if how in ("semi", "anti"):
        assert got[1].numel() == 0
        assert np.array_equal(np.sort(got[0].cpu().numpy()),
                              np.sort(want[0].numpy())), how
    else:
        for a, b in zip(_sorted_pairs(*got), _sorted_pairs(*want)):
            assert np.array_equal(a, b), how
    li = got[0].cpu().numpy()
    li = li[li >= 0]            # right/outer append their -1 rows at the end
    assert np.all(np.diff(li) >= 0), how


@pytest.mark.parametrize("kind", ["int64", "int32"])
def test_dense_duplicate_build_keys(kind, native_calls):
    g = np.random.default_rng(3)
    r = _series(kind, np.concatenate([np.arange(10, 200), [15, 15, 120]]))
    l = _series(kind, g.integers(0, 220, 5000), g.random(5000) >= 0.1)
    for how in ("semi", "anti"):
        _check_dense(l, r, how, native_calls)
    lg, rg = [l.to(DEV)], [r.to(DEV)]
    # inner: the build reports the duplicates, the join falls back to hashing
    before = len(native_calls)
    assert rowops._dense_key_join(lg, rg, "inner") is None
    assert native_calls[before:] == [False]
    _check_pairs(rowops.join(lg, rg, "inner"),
                 rowops._cpu_join([l], [r], "inner"), "inner")


# ---------------------------------------------------------------------------
# hash path
# ---------------------------------------------------------------------------

HASH_MODES = ("inner", "left", "semi", "anti", "right", "outer")


def _str_series(ids, valid):
    vals = [("key-%d" % i) if v else None for i, v in zip(ids, valid)]
    return Series.from_pylist("s", vals, DataType.string())


def _hash_keys(kind, ids, valid):
    """String key, or an (int, string) pair that together carries the id."""
    if kind == "str":
        return [_str_series(ids, valid)]
    return [Series("a", DataType.int64(), data=torch.as_tensor(ids % 7)),
            _str_series(ids // 7, valid)]


@functools.lru_cache(maxsize=None)
def _hash_case(kind, n_l, shape):
    g = np.random.default_rng([n_l, len(shape)])
    if shape == "fanout":      # every build key 1-5 times, nulls both sides
        bids = np.repeat(np.arange(0, 4000, 2), g.integers(1, 6, 2000))
        g.shuffle(bids)
        pids = g.integers(0, 4000, n_l)           # odd ids miss
    elif shape == "all_miss":
        bids = np.repeat(np.arange(0, 600, 2), 2)
        pids = g.integers(0, 300, n_l) * 2 + 1
    else:                      # "chain": one key 300 times among others
        bids = np.concatenate([np.full(300, 42), np.arange(100, 140)])
        g.shuffle(bids)
        pids = np.where(g.random(n_l) < 0.7, 42, g.integers(90, 150, n_l))
    rk = _hash_keys(kind, bids, g.random(len(bids)) >= 0.05)
    lk = _hash_keys(kind, pids, g.random(n_l) >= 0.1)
    return lk, rk, [s.to(DEV) for s in lk], [s.to(DEV) for s in rk]


@functools.lru_cache(maxsize=None)
def _hash_want(kind, n_l, shape, how):
    lk, rk, _, _ = _hash_case(kind, n_l, shape)
    return rowops._cpu_join(lk, rk, how)


@pytest.mark.parametrize("how", HASH_MODES)
@pytest.mark.parametrize("kind, n_l, shape", [
    ("str", 257, "fanout"), ("int_str", 257, "fanout"),
    ("str", BIG, "fanout"), ("int_str", BIG, "fanout"),
    ("str", 257, "all_miss"), ("int_str", BIG, "all_miss"),
    ("str", 257, "chain"), ("int_str", 257, "chain"),
])
def test_hash_join_matches_cpu(kind, n_l, shape, how):
    _, _, lg, rg = _hash_case(kind, n_l, shape)
    assert rowops._dense_key_join(lg, rg, how) is None
    got = rowops.join(lg, rg, how)
    want = _hash_want(kind, n_l, shape, how)
    _check_pairs(got, want, how)
    if shape == "all_miss" and how in ("inner", "semi"):
        assert got[0].numel() == 0

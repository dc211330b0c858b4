"""Radix select (csrc/topk.hip) and the top-k path built on it.

`topk_candidates(keys, k)` must return, exactly, the numpy oracle
T = np.partition(u, k - 1)[k - 1], np.flatnonzero(u <= T) and
[T, #(u < T), #(u == T)].  A block's chunk is max(512, ceil(n / 2048)) rows
rounded up to even and walked in 512-row tiles (two keys per thread), so
BIG = 2040 * 514 + 513 rows is the smallest count at which every block walks
two tiles and the last block is ragged: 2041 blocks, a 2-row second tile in
each, and a last block of 513 rows whose final key is loaded alone.
`topk_multi` must equal `argsort_multi(...)[:k]` element for element."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd.kernels import native_required, rowops

import topk_cases as tc

DEV = "cuda:0"
BIG = 2040 * 514 + 513
SIZES = (1, 63, 64, 65, 255, 256, 257, BIG)
PATTERNS = ("uniform", "all_equal", "bit0", "bit63", "narrow_int", "heavy_bin",
            "run") + tuple(f"span{b}" for b in (11, 12, 22, 23, 64))


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    native_required()


@functools.lru_cache(maxsize=None)
def _keys(pattern, n):
    """(u64 keys, extra ranks to try); read-only, shared by the cases."""
    rng = np.random.default_rng(100 * PATTERNS.index(pattern) + n % 997)
    u = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    extra = ()
    if pattern == "all_equal":
        u[:] = np.uint64(0xF123456789ABCDEF)
    elif pattern in ("bit0", "bit63"):
        bit = np.uint64(1) << np.uint64(0 if pattern == "bit0" else 63)
        u = np.uint64(0x0123456789ABCDE0) | (u & bit)
    elif pattern == "narrow_int":
        # sign-flipped ints in [-500, 500): the digit sits under a long prefix
        u = (rng.integers(-500, 500, size=n) ^ -(1 << 63)).view(np.uint64)
    elif pattern == "heavy_bin":
        heavy = rng.random(n) < 0.9
        u[heavy] = (u[heavy] >> np.uint64(11)) | np.uint64(0x5A5 << 53)
    elif pattern == "run":
        u = np.sort(u)
        lo, hi = n // 4, max(3 * n // 4, n // 4 + 1)
        u[lo:hi] = u[lo]
        u = u[rng.permutation(n)]
        extra = (lo + 1, hi)
    elif pattern.startswith("span"):
        bits = int(pattern[4:])
        if bits < 64:
            mask = np.uint64(((1 << bits) - 1) << 7)
            u = (u & mask) | (np.uint64(0xA5A5A5A5A5A5A5A5) & ~mask)
            # both ends present, so exactly `bits` bits vary (n >= 2)
            u[0] &= ~mask
            u[-1] |= mask
    u.setflags(write=False)
    return u, extra


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_topk_candidates_matches_numpy(pattern, n):
    u, extra = _keys(pattern, n)
    dev = torch.from_numpy(u.view(np.int64).copy()).to(DEV)
    ks = sorted({min(max(k, 1), n) for k in (1, 2, n // 2, n - 1, n) + extra})
    for k in ks:
        t = np.partition(u, k - 1)[k - 1]
        rows, stats = native_required().topk_candidates(dev, k)
        assert np.array_equal(rows.cpu().numpy(), np.flatnonzero(u <= t)), \
            (pattern, n, k)
        want = [int(t.view(np.int64)), int(np.count_nonzero(u < t)),
                int(np.count_nonzero(u == t))]
        assert stats.cpu().tolist() == want, (pattern, n, k)


def test_unaligned_slice_and_bad_arguments():
    nat = native_required()
    u, _ = _keys("uniform", BIG)
    dev = torch.from_numpy(u.view(np.int64).copy()).to(DEV)
    t = np.partition(u[1:], 99)[99]     # dev[1:] starts 8 bytes off 16
    rows = nat.topk_candidates(dev[1:], 100)[0].cpu().numpy()
    assert np.array_equal(rows, np.flatnonzero(u[1:] <= t))
    for bad, k in ((dev, 0), (dev, BIG + 1), (dev.to(torch.int32), 1),
                   (dev[::2], 1), (dev.cpu(), 1), (dev.reshape(1, -1), 1)):
        with pytest.raises(RuntimeError):
            nat.topk_candidates(bad, k)


@pytest.fixture
def gate_open(monkeypatch):
    monkeypatch.setattr(rowops, "_TOPK_MIN_ROWS", 1)
    monkeypatch.setattr(rowops, "_TOPK_MAX_FRACTION", 1)
    calls = []
    real = rowops.topk_candidates
    monkeypatch.setattr(rowops, "topk_candidates",
                        lambda keys, k: calls.append(k) or real(keys, k))
    return calls


@pytest.mark.parametrize("n", (300, 5000))
@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_topk_multi_equals_full_sort_prefix(name, n, gate_open):
    keys, desc, nf = tc.key_lists(n)[name]
    keys = [s.to(DEV) for s in keys]
    full = rowops.argsort_multi(keys, desc, nf)
    for k in tc.KS + (n,):
        got = rowops.topk_multi(keys, desc, nf, k)
        assert got.is_cuda and torch.equal(got, full[:k]), (name, n, k)
    assert gate_open == list(tc.KS + (n,))      # the select path ran


def test_dataframe_sort_limit_offset(gate_open):
    rng, n = np.random.default_rng(5), 4000
    price = (rng.integers(0, 200, size=n) / 8.0).tolist()
    day = rng.integers(0, 30, size=n).tolist()
    df = daft.from_pydict({"price": price, "day": day,
                           "row": list(range(n))}, device=DEV)
    out = (df.sort([daft.col(c) for c in ("price", "day", "row")],
                   desc=[True, False, False])
             .offset(10).limit(25).to_pydict())
    want = sorted(range(n), key=lambda i: (-price[i], day[i], i))[10:35]
    assert out["row"] == want and gate_open      # through the select path

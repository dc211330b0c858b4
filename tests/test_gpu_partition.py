"""Native stable partitioner (csrc/partition.hip) against a numpy oracle.

`hash_partition(h, P, remix)` must return, element for element, the stable
argsort and the bincount of `h % P` (unsigned 64-bit; `splitmix64(h) % P`
with remix).  The sizes cover one lane to many blocks: a block's chunk is
max(256, ceil(n / 2048)) rows walked in 256-row tiles, so 2048 * 256 + 1 rows
give 2040 blocks whose second tile holds one row (the running offset is
carried between tiles) and a ragged last block."""
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
BIG = 2048 * 256 + 1
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, BIG)
PARTS = (1, 2, 3, 7, 8, 64, 255, 256)
PATTERNS = ("uniform", "all_equal", "alternating", "sorted", "runs")


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    native_required()


def _splitmix64(x):
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def test_oracle_splitmix64_known_values():
    # first outputs of the public-domain splitmix64 generator seeded with 0
    # and 1: state + golden gamma is folded into the mix, as in common.h
    got = _splitmix64(np.array([0, 1], dtype=np.uint64))
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x910A2DEC89025CC1]


@functools.lru_cache(maxsize=None)
def _hashes(pattern, n):
    """u64 hashes as an int64 bit pattern (read-only, shared by the cases)."""
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n % 997)
    u = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if pattern == "uniform":
        pass        # about half have the top bit set: catches signed modulo
    elif pattern == "all_equal":
        u[:] = np.uint64(0xF123456789ABCDEF)
    elif pattern == "alternating":
        u = (np.arange(n) % 2).astype(np.uint64)
    elif pattern == "sorted":
        u = np.sort(u)
    elif pattern == "runs":
        # equal hashes share a partition with and without remix.  Many
        # blocks: rows 0..1023 fill whole tiles of the first blocks with one
        # partition, rows 1024..1279 fill whole waves of a tile whose last
        # wave is mixed.  One block: the first wave is all one partition.
        if n > 1280:
            u[:1024] = np.uint64(0xC0FFEE0000000001)
            u[1024:1280] = np.uint64(0x8000000000000002)
        else:
            u[:64] = np.uint64(0xC0FFEE0000000001)
    h = u.view(np.int64)
    h.setflags(write=False)
    return h


def _oracle(h, parts, remix):
    u = h.view(np.uint64)
    if remix:
        u = _splitmix64(u)
    ids = (u % np.uint64(parts)).astype(np.int64)
    return (np.argsort(ids, kind="stable").astype(np.int64),
            np.bincount(ids, minlength=parts).astype(np.int64))


def _check(got, want, what):
    perm, counts = got
    for g, w, name in ((perm, want[0], "perm"), (counts, want[1], "counts")):
        assert g.dtype == torch.int64 and g.is_cuda, (what, name)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_hash_partition_matches_stable_argsort(pattern, n):
    nat = native_required()
    h = _hashes(pattern, n)
    dev = torch.from_numpy(h.copy()).to(DEV)
    for parts in PARTS:
        for remix in (False, True):
            want = _oracle(h, parts, remix)
            if pattern == "all_equal" and n:
                assert np.count_nonzero(want[1]) == 1
            _check(nat.hash_partition(dev, parts, remix), want,
                   (pattern, n, parts, remix))


@pytest.mark.parametrize("parts", (0, 257, -1))
def test_partition_count_out_of_range_raises(parts):
    h = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        native_required().hash_partition(h, parts, False)


@pytest.mark.parametrize("remix", (False, True))
def test_strided_input_equals_its_contiguous_copy(remix):
    nat = native_required()
    h = torch.from_numpy(_hashes("uniform", BIG).copy()).to(DEV)
    pair = torch.stack([h, torch.zeros_like(h)], dim=1)
    view = pair[:, 0]
    assert not view.is_contiguous()
    got = nat.hash_partition(view, 7, remix)
    want = nat.hash_partition(h, 7, remix)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    _check(got, _oracle(_hashes("uniform", BIG), 7, remix), remix)


# ---------------------------------------------------------------------------
# rowops: the device path equals the CPU path
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _keys(kind, n):
    rng = np.random.default_rng(n % 991 + (7 if kind == "string" else 0))
    vals = rng.integers(-1000, 1000, size=n)
    valid = rng.random(n) > 0.1
    if kind == "int64":
        return Series("k", DataType.int64(),
                      data=torch.from_numpy(vals.astype(np.int64)),
                      validity=torch.from_numpy(valid))
    return Series.from_pylist(
        "k", [f"key_{v}" if ok else None for v, ok in zip(vals, valid)],
        DataType.string())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ("int64", "string"))
def test_partition_by_hash_equals_cpu(kind, n):
    s = _keys(kind, n)
    for parts in (2, 8, 256, 300):      # 300 takes the radix-sort fallback
        want = rowops.partition_by_hash([s], parts)
        got = rowops.partition_by_hash([s.to(DEV)], parts)
        for g, w, name in zip(got, want, ("perm", "counts")):
            assert g.is_cuda and g.dtype == torch.int64
            assert torch.equal(g.cpu(), w), (kind, n, parts, name)


@pytest.mark.parametrize("n", (0, 257, BIG))
def test_rowops_hash_partition_remix_equals_cpu(n):
    h = torch.from_numpy(_hashes("uniform", n).copy())
    for parts in (2, 7, 256, 300):      # 300: splitmix64 in torch ops
        want = rowops.hash_partition(h, parts, remix=True)
        _check(rowops.hash_partition(h.to(DEV), parts, remix=True),
               tuple(w.numpy() for w in want), (n, parts))
        ow = _oracle(h.numpy(), parts, True)
        assert torch.equal(want[0], torch.from_numpy(ow[0]))
        assert torch.equal(want[1], torch.from_numpy(ow[1]))

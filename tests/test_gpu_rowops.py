"""Row kernels of csrc/kernels.hip and csrc/sort.hip (hash_rows, groupby,
count_distinct_pairs, dense_first_index, compact_indices, u64_mod,
radix_argsort) against the exact oracle in rowops_cases.py: the wrapper
matrix of test_rowops_parity.py on cuda:0, then the raw bindings at the
shapes where they change path.  Every comparison is exact.

The raw bindings only get inputs the wrappers could produce: group ids
inside [0, num_groups), packed keys inside [0, rng)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from daft_amd import DataType, Series
from daft_amd import kernels
from daft_amd.kernels import native_required, rowops

import rowops_cases as rc
import test_rowops_parity as tier

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


def _dev_i64(a: np.ndarray) -> torch.Tensor:
    """numpy int64/uint64 -> int64 device tensor with the same bits."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


# ---------------------------------------------------------------------------
# wrapper matrix on the device
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,sliced,nullable,seed", tier.HASH_MATRIX)
def test_hash_column(kind, sliced, nullable, seed):
    tier.check_hash_column(kind, sliced, nullable, seed, DEV)


@pytest.mark.parametrize("name", list(rc.HASH_ROWS))
def test_hash_rows_of_mixed_columns(name):
    tier.check_hash_rows(name, DEV)


def test_hash_large_int64():
    """n = 600_001: past the 2048-block grid, so the grid-stride loop runs."""
    tier.check_hash_large(DEV)


def test_public_hash_ignores_dictionary_encoding():
    tier.check_public_hash_ignores_encoding(DEV)


@pytest.mark.parametrize("name", rc.GROUP_KEY_SETS)
def test_groupby_wrapper(name):
    tier.check_groupby(name, DEV)


@pytest.mark.parametrize("kind,nullable", tier.SORT_MATRIX)
def test_argsort_column(kind, nullable):
    tier.check_sort_column(kind, nullable, DEV)


@pytest.mark.parametrize("name", rc.TWO_KEY_SORTS)
def test_argsort_two_keys(name):
    tier.check_sort_two_keys(name, DEV)


@pytest.mark.parametrize("name", rc.MASKS)
def test_compact_indices(name):
    tier.check_compact(name, DEV)


def test_compact_indices_drops_null_rows():
    tier.check_compact_drops_nulls(DEV)


def test_partition_by_hash():
    tier.check_partition_by_hash(DEV)


def test_dataframe_sort_floats():
    tier.check_dataframe_sort(DEV)


def test_dataframe_distinct_floats():
    tier.check_dataframe_distinct(DEV)


def test_dataframe_count_distinct_floats():
    tier.check_dataframe_count_distinct(DEV)


# ---------------------------------------------------------------------------
# radix_argsort
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.RADIX_KEYS)
def test_radix_argsort_is_the_stable_permutation(name):
    nat = native_required()
    for n in rc.ROW_COUNTS:
        keys = rc.radix_keys(name, n)
        got = nat.radix_argsort(_dev_i64(keys)).cpu().numpy()
        assert got.dtype == np.int64
        want = np.argsort(keys, kind="stable")
        assert np.array_equal(got, want), f"n={n}"


# ---------------------------------------------------------------------------
# groupby (raw binding)
# ---------------------------------------------------------------------------

def _raw_groupby(cols, hashes=None):
    series = [rc.to_series(c, DEV, f"k{j}") for j, c in enumerate(cols)]
    h = rowops.hash_columns(series) if hashes is None else _dev_i64(hashes)
    tags, datas, offs, vals = kernels._descs(series)
    ids, reps = native_required().groupby(h, tags, datas, offs, vals)
    return ids.cpu(), reps.cpu()


@pytest.mark.parametrize("name", rc.GROUP_KEY_SETS)
def test_groupby_partition(name):
    for n in rc.GROUP_ROW_COUNTS:
        cols = rc.group_keys(name, n)
        ids, reps = _raw_groupby(cols)
        rc.assert_partition(ids, reps, rc.key_codes(cols))


def test_groupby_four_keys_contended():
    """4 keys over 600_001 rows: every row races for one of four slots."""
    g = np.random.default_rng(4)
    code = g.integers(0, 4, rc.LARGE_N)
    vals = np.array([-1, 0, 2**62, np.iinfo(np.int64).min], dtype=np.int64)
    ids, reps = _raw_groupby([rc.Col("int64", vals[code])])
    rc.assert_partition(ids, reps, code)


@pytest.mark.parametrize("mode", ["equal", "slot"])
def test_groupby_colliding_hashes(mode):
    """Supplied hashes that all land on one home slot: the probe chain and
    the full key compare decide, not the hash."""
    cols, code = rc.colliding_keys()
    ids, reps = _raw_groupby(cols, rc.colliding_hashes(code, mode))
    rc.assert_partition(ids, reps, code)


# ---------------------------------------------------------------------------
# count_distinct_pairs
# ---------------------------------------------------------------------------

def _count_distinct_case(kind, n):
    """7 groups: group 5 has no rows, group 1 only nulls."""
    G = 7
    g = np.random.default_rng([n, 7])
    gids = g.integers(0, G, n)
    gids[gids == 5] = 6
    c = rc.gen_col(kind, n, True, ties=True, salt=3)
    c.valid[gids == 1] = False
    return gids, G, c


@pytest.mark.parametrize("kind", ["float64", "string", "int16"])
@pytest.mark.parametrize("equal_hashes", [False, True])
def test_count_distinct_pairs(kind, equal_hashes):
    for n in ((2000,) if equal_hashes else (1, 33, 4099)):
        gids, G, c = _count_distinct_case(kind, n)
        gd = _dev_i64(gids)
        series = [Series("__gid", DataType.int64(), data=gd),
                  rc.to_series(c, DEV, "v")]
        if equal_hashes:
            h = _dev_i64(np.full(n, 0x5555555555555555, dtype=np.uint64))
        else:
            h = rowops.hash_columns(series)
        tags, datas, offs, vals = kernels._descs(series)
        cnt = native_required().count_distinct_pairs(
            h, tags, datas, offs, vals, gd, G)
        want = rc.expected_count_distinct(gids, G, c)
        assert want[1] == 0 and want[5] == 0
        assert cnt.cpu().tolist() == want, f"n={n}"


# ---------------------------------------------------------------------------
# dense_first_index
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rng", rc.DENSE_RANGES)
def test_dense_first_index(rng):
    nat = native_required()
    for n in rc.DENSE_ROW_COUNTS:
        packed = rc.dense_packed(n, rng)
        assert packed.min() >= 0 and packed.max() < rng
        got = nat.dense_first_index(_dev_i64(packed), rng, n).cpu().numpy()
        want = rc.expected_first_index(packed, rng, n)
        if rng > 2:
            assert want[rng // 2] == n         # the sentinel stays
        assert np.array_equal(got, want), f"n={n}"


# ---------------------------------------------------------------------------
# u64_mod
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", rc.MOD_DIVISORS)
def test_u64_mod(d):
    h = np.array(rc.MOD_HASHES, dtype=np.uint64)
    got = native_required().u64_mod(_dev_i64(h), d).cpu().tolist()
    assert got == [v % d for v in rc.MOD_HASHES]

"""CPU paths of the row kernels (hash_columns, groupby, argsort_multi,
compact_indices, partition_by_hash, Series.hash, DataFrame.sort / .distinct
/ count_distinct) against the exact oracle in rowops_cases.py, over its
tables.  This proves the oracle and the tables without a GPU and pins the
CPU path that test_gpu_rowops.py mirrors: the check_* drivers below take
the device and are run there again on cuda:0."""
import numpy as np
import pytest
import torch

import daft_amd as daft
from daft_amd import DataType, Series, col
from daft_amd import kernels
from daft_amd.kernels import rowops

import rowops_cases as rc

DEV = "cpu"

HASH_MATRIX = [pytest.param(kind, sliced, nullable, seed,
                            id=f"{cid}-{'null' if nullable else 'plain'}-"
                               f"seed{si}")
               for cid, kind, sliced in rc.HASH_COLUMNS
               for nullable in (False, True)
               for si, seed in enumerate(rc.SEEDS)]
SORT_MATRIX = [pytest.param(kind, nullable,
                            id=f"{kind}-{'null' if nullable else 'plain'}")
               for kind in rc.SORT_KINDS for nullable in (False, True)]


# ---------------------------------------------------------------------------
# the oracle itself
# ---------------------------------------------------------------------------

def test_oracle_fixed_points():
    # first outputs of the published SplitMix64 generator seeded with 0:
    # state k * GOLDEN, so splitmix64(k * GOLDEN) is output k + 1
    assert rc.splitmix64(0) == 0xE220A8397B1DCDAF
    assert rc.splitmix64(rc.GOLDEN) == 0x6E789E6AA1B965F4
    assert rc.splitmix64(2 * rc.GOLDEN & rc.M64) == 0x06C45D188009454F
    assert rc.hash_bytes(b"") == 0xcbf29ce484222325
    assert rc.hash_bytes(b"\0") != rc.hash_bytes(b"") != rc.hash_bytes(b"\0\0")
    # one whole word and nothing else: no tail round
    assert rc.hash_bytes(b"abcdefgh") == rc.splitmix64(
        (0xcbf29ce484222325 ^ 8) ^ 0x6867666564636261)
    # the length is folded in at the start, so a prefix is no shortcut
    assert rc.hash_bytes(b"abcdefghi") == rc.splitmix64(rc.splitmix64(
        (0xcbf29ce484222325 ^ 9) ^ 0x6867666564636261) ^ 0x69)
    assert rc.canon_f64_bits(-0.0) == 0
    assert rc.canon_f64_bits(float("nan")) == rc.CANON_NAN
    assert rc.canon_f64_bits(-float("nan")) == rc.CANON_NAN
    assert rc.canon_f64_bits(1.0) == 0x3FF0000000000000
    assert rc.canon_f64_bits(float("-inf")) == 0xFFF0000000000000


def test_oracle_vectorised_form_agrees_with_scalar():
    v = rc.large_int64()
    head = rc.Col("int64", v[:1000])
    for seed in rc.SEEDS:
        assert rc.hash_int64_np(v[:1000], seed).tolist() == \
            rc.oracle_hash([head], seed)


def test_sort_oracle_contract():
    nan = float("nan")
    c = rc.Col("float64", np.array(
        [1.0, -nan, nan, -np.inf, np.inf, -0.0, 0.0]))
    assert np.signbit(c.data[1]) and not np.signbit(c.data[2])
    # NaNs tie and sort above +inf, the zeros tie; ties keep input order
    assert rc.sort_perm([c], [False], [False]) == [3, 5, 6, 0, 4, 1, 2]
    assert rc.sort_perm([c], [True], [False]) == [1, 2, 4, 0, 5, 6, 3]
    d = rc.Col("uint8", np.array([200, 3, 0, 255], np.uint8),
               np.array([True, True, False, True]))
    assert rc.sort_perm([d], [False], [False]) == [1, 0, 3, 2]
    assert rc.sort_perm([d], [True], [False]) == [3, 0, 1, 2]
    assert rc.sort_perm([d], [True], [True]) == [2, 3, 0, 1]


def test_tables_hold_what_they_promise():
    f = rc.hash_col("float64", 4099, False).cells()
    assert any(v != v for v in f) and any(v == 0.0 for v in f)
    bits = rc.hash_col("float64", 4099, False).data.view(np.uint64)
    assert (bits == 0x8000000000000000).any()          # -0.0
    assert (bits == 0xFFF8000000000000).any()          # -NaN
    lens = {len(b) for b in rc.hash_col("binary", 4099, False).data}
    assert set(rc.STRING_LENS) <= lens
    blob = b"".join(rc.hash_col("binary", 4099, False).data)
    assert 0 in blob and max(blob) >= 0x80
    c = rc.hash_col("string", 257, True, True)
    s = rc.to_series(c, DEV)
    assert s.data.storage_offset() == 3 and len(s) == 257   # odd byte start
    got = s.to_pylist()
    assert [None if v is None else v.encode() for v in got] == c.cells()
    under_null = [b for b, ok in zip(c.data, c.valid) if not ok]
    assert sum(len(b) > 0 for b in under_null) > 10
    for kind in rc.FIXED_KINDS:
        c = rc.sort_col(kind, 257, True)
        assert len(set(map(rc.eq_key, c.cells()))) < 40     # ties
    cols, code = rc.colliding_keys()
    assert len(np.unique(code)) == 50
    assert np.array_equal(rc.key_codes(cols), rc.key_codes(
        [rc.Col("int64", code)]))
    for mode in ("equal", "slot"):
        h = rc.colliding_hashes(code, mode)
        assert len(np.unique(h % np.uint64(rc.CAP_COLLIDE))) == 1
        assert len(np.unique(h)) == (1 if mode == "equal" else 50)


# ---------------------------------------------------------------------------
# drivers: the code under test against the oracle, on `dev`
# ---------------------------------------------------------------------------

def check_hash_column(kind, sliced, nullable, seed, dev):
    for n in rc.SCALAR_ROW_COUNTS:
        c = rc.hash_col(kind, n, nullable, sliced)
        s = rc.to_series(c, dev)
        got = rc.u64_list(rowops.hash_columns([s], seed))
        assert got == rc.expected_hash([c], seed), f"n={n}"


def check_hash_rows(name, dev):
    for n in rc.SCALAR_ROW_COUNTS:
        cols = rc.hash_row_cols(name, n)
        series = [rc.to_series(c, dev, f"c{j}") for j, c in enumerate(cols)]
        for seed in rc.SEEDS:
            got = rc.u64_list(rowops.hash_columns(series, seed))
            assert got == rc.expected_hash(cols, seed), f"n={n} seed={seed}"


def check_hash_large(dev):
    v = rc.large_int64()
    s = Series("v", DataType.int64(), data=torch.from_numpy(v).to(dev))
    for seed in (0, -1):
        got = rowops.hash_columns([s], seed).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, rc.hash_int64_np(v, seed))


def check_public_hash_ignores_encoding(dev):
    """Series.hash and Expression.hash of a dictionary column are those of
    its strings."""
    for n in (1, 257, 4099):
        for nullable in (False, True):
            c = rc.gen_col("dict", n, nullable)
            s = rc.to_series(c, dev)
            assert s.is_dict()
            for seed in rc.SEEDS:
                want = rc.expected_hash([c], seed)
                assert rc.u64_list(s.hash(seed)) == want
                assert rc.u64_list(s.dict_decode().hash(seed)) == want
            out = daft.from_pydict({"s": s}, device=dev) \
                .select(col("s").hash(seed=1).alias("h")).to_pydict()
            assert out["h"] == rc.expected_hash([c], 1)


def check_groupby(name, dev):
    for n in rc.GROUP_ROW_COUNTS:
        cols = rc.group_keys(name, n)
        series = [rc.to_series(c, dev, f"k{j}") for j, c in enumerate(cols)]
        ids, reps = rowops.groupby(series)
        rc.assert_partition(ids, reps, rc.key_codes(cols))


def check_sort_column(kind, nullable, dev):
    for n in rc.SCALAR_ROW_COUNTS:
        c = rc.sort_col(kind, n, nullable)
        s = rc.to_series(c, dev)
        for desc, nf in rc.SORT_FLAGS:
            got = rowops.argsort_multi([s], [desc], [nf]).cpu().tolist()
            assert got == rc.sort_perm([c], [desc], [nf]), \
                f"n={n} desc={desc} nulls_first={nf}"


def check_sort_two_keys(name, dev):
    for n in (2, 257, 4099):
        cols = rc.two_key_sort(name, n)
        series = [rc.to_series(c, dev, f"k{j}") for j, c in enumerate(cols)]
        for d0, nf0 in rc.SORT_FLAGS:
            for d1, nf1 in ((False, False), (True, True)):
                got = rowops.argsort_multi(series, [d0, d1],
                                           [nf0, nf1]).cpu().tolist()
                assert got == rc.sort_perm(cols, [d0, d1], [nf0, nf1]), \
                    f"n={n} desc={(d0, d1)} nulls_first={(nf0, nf1)}"


def check_compact(name, dev):
    for n in rc.ROW_COUNTS:
        m = rc.mask(name, n)
        s = Series("m", DataType.bool(), data=torch.from_numpy(m).to(dev))
        got = kernels.compact_indices(s).cpu().numpy()
        assert got.dtype == np.int64
        assert np.array_equal(got, np.flatnonzero(m)), f"n={n}"


def check_compact_drops_nulls(dev):
    n = 4099
    m, v = rc.mask("random_99pct", n), rc.mask("alternating", n)
    s = Series("m", DataType.bool(), data=torch.from_numpy(m).to(dev),
               validity=torch.from_numpy(v).to(dev))
    got = kernels.compact_indices(s).cpu().numpy()
    assert np.array_equal(got, np.flatnonzero(m & v))


def check_partition_by_hash(dev):
    n = 4099
    cols = rc.group_keys("two_col", n)
    series = [rc.to_series(c, dev, f"k{j}") for j, c in enumerate(cols)]
    h = np.array(rc.oracle_hash(cols, 0), dtype=np.uint64)
    for parts in (1, 2, 7, 16):
        part = (h % np.uint64(parts)).astype(np.int64)
        perm, counts = rowops.partition_by_hash(series, parts)
        assert counts.cpu().tolist() == \
            np.bincount(part, minlength=parts).tolist()
        assert np.array_equal(perm.cpu().numpy(),
                              np.argsort(part, kind="stable"))


def _float_frame(dev):
    c = rc.sort_col("float64", 257, True)
    g = rc.Col("int64", (np.arange(257) % 3).astype(np.int64))
    df = daft.from_pydict({"g": rc.to_series(g, dev, "g"),
                           "v": rc.to_series(c, dev, "v")}, device=dev)
    return df, g, c


def check_dataframe_sort(dev):
    df, g, c = _float_frame(dev)
    cells = c.cells()
    for desc in (False, True):
        out = df.sort("v", desc=desc).to_pydict()["v"]
        # DataFrame.sort puts nulls last ascending and first descending
        nf = out[0] is None
        assert nf == desc
        want = [cells[i] for i in rc.sort_perm([c], [desc], [nf])]
        assert [repr(v) for v in out] == [repr(v) for v in want]


def check_dataframe_distinct(dev):
    df, g, c = _float_frame(dev)
    out = df.select(col("v")).distinct().to_pydict()["v"]
    want = {rc.eq_key(v) for v in c.cells()}
    assert len(out) == len(want)
    assert {rc.eq_key(v) for v in out} == want


def check_dataframe_count_distinct(dev):
    df, g, c = _float_frame(dev)
    out = df.groupby("g").agg(col("v").count_distinct().alias("nd")) \
        .sort("g").to_pydict()
    assert out["g"] == [0, 1, 2]
    assert out["nd"] == rc.expected_count_distinct(g.data, 3, c)
    total = df.agg(col("v").count_distinct().alias("nd")).to_pydict()["nd"]
    assert total == rc.expected_count_distinct(
        np.zeros(257, dtype=np.int64), 1, c)


# ---------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,sliced,nullable,seed", HASH_MATRIX)
def test_hash_column(kind, sliced, nullable, seed):
    check_hash_column(kind, sliced, nullable, seed, DEV)


@pytest.mark.parametrize("name", list(rc.HASH_ROWS))
def test_hash_rows_of_mixed_columns(name):
    check_hash_rows(name, DEV)


def test_hash_large_int64():
    check_hash_large(DEV)


def test_public_hash_ignores_dictionary_encoding():
    check_public_hash_ignores_encoding(DEV)


@pytest.mark.parametrize("name", rc.GROUP_KEY_SETS)
def test_groupby(name):
    check_groupby(name, DEV)


@pytest.mark.parametrize("kind,nullable", SORT_MATRIX)
def test_argsort_column(kind, nullable):
    check_sort_column(kind, nullable, DEV)


@pytest.mark.parametrize("name", rc.TWO_KEY_SORTS)
def test_argsort_two_keys(name):
    check_sort_two_keys(name, DEV)


@pytest.mark.parametrize("name", rc.MASKS)
def test_compact_indices(name):
    check_compact(name, DEV)


def test_compact_indices_drops_null_rows():
    check_compact_drops_nulls(DEV)


def test_partition_by_hash():
    check_partition_by_hash(DEV)


def test_dataframe_sort_floats():
    check_dataframe_sort(DEV)


def test_dataframe_distinct_floats():
    check_dataframe_distinct(DEV)


def test_dataframe_count_distinct_floats():
    check_dataframe_count_distinct(DEV)

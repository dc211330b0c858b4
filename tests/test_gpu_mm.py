"""Kernels of csrc/multimodal.hip (minhash, simhash, hll_update,
image_resize), csrc/bpe.hip and csrc/editdist.hip against the oracles in
mm_cases.py: the drivers of test_mm_parity.py on cuda:0, then the raw
hll_update and levenshtein bindings and approx_count_distinct, which has no
CPU counterpart (the CPU path counts exactly).

Every comparison is exact but two, both stated in mm_cases.py: the
HyperLogLog estimate may differ by 1 from the oracle's, and a resized pixel
whose exact value is within RESIZE_NEAR of a rounding boundary may differ
by 1.

The raw bindings only get inputs the wrappers could produce: group ids
inside [0, num_groups), offsets inside the byte buffers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import col
from daft_amd.kernels import native_required, rowops

import mm_cases as mc
import rowops_cases as rc
import strings_cases as sc
import test_mm_parity as tier

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


def _dev_i64(a: np.ndarray) -> torch.Tensor:
    """numpy int64/uint64 -> int64 device tensor with the same bits."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


# ---------------------------------------------------------------------------
# minhash and simhash
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("num_hashes,ngram,layout", tier.MINHASH_MATRIX)
def test_minhash(num_hashes, ngram, layout):
    tier.check_minhash(num_hashes, ngram, layout, DEV)


def test_minhash_row_counts():
    """8193 rows: past 2048 blocks x 4 waves, so the row-stride loop runs."""
    tier.check_minhash_row_counts(DEV)


def test_minhash_expression():
    tier.check_minhash_expression(DEV)


def test_minhash_simhash_reject_bad_arguments():
    tier.check_minhash_rejects_bad_args(DEV)


@pytest.mark.parametrize("ngram,kind,layout", tier.SIMHASH_MATRIX)
def test_simhash(ngram, kind, layout):
    tier.check_simhash(ngram, kind, layout, DEV)


def test_simhash_row_counts():
    tier.check_simhash_row_counts(DEV)


def test_simhash_expression():
    tier.check_simhash_expression(DEV)


# A bad argument raises on the host, before anything is launched; the valid
# call after each group shows that the context is still sound.
_ROWS3 = [v.encode() for v in sc.REFUSED_VALUES]


def _col3():
    s = mc.text_series(_ROWS3, DEV, "binary")
    return s.offsets, s.data


def _col4():
    s = mc.text_series(_ROWS3 + [b"d"], DEV, "binary")
    return s.offsets, s.data


def test_simhash_refuses_bad_arguments():
    nat = native_required()
    off, data = _col3()
    sc.assert_refuses_bad_columns(
        "simhash", lambda o, d: nat.simhash(o, d, 2), off, data)
    got = nat.simhash(off, data, 2).cpu().numpy().view(np.uint64).tolist()
    assert got == [mc.simhash_oracle(r, 2) for r in _ROWS3]


def test_minhash_refuses_bad_arguments():
    nat = native_required()
    off, data = _col3()
    a, b = mc.minhash_perms(4)
    pa, pb = (_dev_i64(np.array(p, dtype=np.uint64)) for p in (a, b))
    sc.assert_refuses_bad_columns(
        "minhash", lambda o, d: nat.minhash(o, d, 4, 1, pa, pb), off, data)
    for bad_a, bad_b in ((pa.cpu(), pb), (pa, pb.to(torch.int32)),
                         (torch.cat([pa, pa])[::2], pb)):
        with pytest.raises(RuntimeError, match="minhash: "):
            nat.minhash(off, data, 4, 1, bad_a, bad_b)
    got = nat.minhash(off, data, 4, 1, pa, pb).cpu().numpy()
    assert (got.view(np.uint32).reshape(3, 4) ==
            mc.expected_minhash(_ROWS3, 4, 1)).all()


# ---------------------------------------------------------------------------
# HyperLogLog: the raw binding, registers compared exactly
# ---------------------------------------------------------------------------

def _hll_update(hashes, gids, valid, groups) -> np.ndarray:
    """None goes in as an empty tensor: group 0, every row valid."""
    g = torch.empty(0, dtype=torch.int64, device=DEV) if gids is None \
        else _dev_i64(gids)
    v = torch.empty(0, dtype=torch.bool, device=DEV) if valid is None \
        else torch.from_numpy(valid).to(DEV)
    regs = native_required().hll_update(_dev_i64(hashes), g, v, groups)
    assert regs.dtype == torch.int32 and regs.numel() == groups * mc.HLL_REGS
    return regs.cpu().numpy().astype(np.int64).reshape(groups, mc.HLL_REGS)


@pytest.mark.parametrize("name", list(mc.HLL_RAW))
def test_hll_update_registers(name):
    hashes, gids, valid, groups = mc.HLL_RAW[name]
    want = mc.hll_registers_np(hashes, gids, valid, groups)
    if len(hashes) <= 3000:
        assert np.array_equal(want, mc.hll_registers(hashes, gids, valid,
                                                     groups))
    got = _hll_update(hashes, gids, valid, groups)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(g, i, got[g, i], want[g, i])
                           for g, i in bad[:5].tolist()]


def test_hll_update_without_rows():
    got = _hll_update(np.zeros(0, np.uint64), None, None, 2)
    assert not got.any()


# ---------------------------------------------------------------------------
# approx_count_distinct end to end
# ---------------------------------------------------------------------------

def _check_hll_column(c: mc.HllColumn, batch_rows=None):
    s = rc.to_series(c.col, DEV, "v")
    # the registers the aggregation builds: row hashes through hll_update
    h = rowops.hash_columns([s])
    assert rc.u64_list(h) == rc.expected_hash([c.col], 0)
    regs = _hll_update(h.cpu().numpy(), c.gids, c.col.valid, c.groups)
    assert np.array_equal(regs, c.registers)
    agg = col("v").approx_count_distinct().alias("n")
    if c.gids is None:
        df = daft.from_pydict({"v": s}, device=DEV)
        if batch_rows:
            df = df.into_batches(batch_rows)
        got = df.agg(agg).to_pydict()["n"]
    else:
        g = rc.to_series(rc.Col("int64", c.gids), DEV, "g")
        df = daft.from_pydict({"g": g, "v": s}, device=DEV)
        if batch_rows:
            df = df.into_batches(batch_rows)
        out = df.groupby("g").agg(agg).sort("g").to_pydict()
        assert out["g"] == list(range(c.groups))
        got = out["n"]
    assert len(got) == c.groups
    for n, est, true in zip(got, c.estimates, c.true):
        print(f"approx_count_distinct {n}, oracle {est:.3f}, true {true}")
        # torch.log and math.log may round a .5 apart
        assert abs(n - mc.round_half_up_int(est)) <= 1
        assert abs(n - true) <= mc.HLL_4SIGMA * true
    return got


@pytest.mark.parametrize("distinct", mc.HLL_DISTINCT)
def test_approx_count_distinct_int64(distinct):
    _check_hll_column(mc.hll_column("int64", distinct))


@pytest.mark.parametrize("kind,distinct,nullable", [
    ("string", 0, False), ("string", 1, False), ("string", 5000, False),
    ("string", 5000, True), ("int64", 0, True), ("int64", 1, True),
    ("int64", 5000, True)])
def test_approx_count_distinct_strings_and_nulls(kind, distinct, nullable):
    _check_hll_column(mc.hll_column(kind, distinct, nullable))


@pytest.mark.parametrize("kind", ["int64", "string"])
def test_approx_count_distinct_grouped(kind):
    """Group 2 is all null and group 3 one value: 0 and 1, next to 100 and
    5000 distinct values in the neighbouring register blocks."""
    got = _check_hll_column(mc.hll_grouped(kind))
    assert got[2] == 0 and got[3] == 1


def test_approx_count_distinct_in_batches_equals_one_batch():
    c = mc.hll_column("int64", 5000, True)
    assert _check_hll_column(c, batch_rows=1024) == _check_hll_column(c)
    g = mc.hll_grouped("int64")
    assert _check_hll_column(g, batch_rows=1000) == _check_hll_column(g)


# ---------------------------------------------------------------------------
# BPE
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,utf8", tier.BPE_MATRIX)
def test_bpe_encode_series(name, utf8):
    tier.check_bpe(name, utf8, DEV)


@pytest.mark.parametrize("layout", mc.LAYOUTS)
def test_bpe_encode_columns(layout):
    tier.check_bpe_columns(layout, DEV)


def test_bpe_encode_many_short_rows():
    """4100 rows on a 4096-block grid: a block's second row reuses its LDS."""
    tier.check_bpe_many_short_rows(DEV)


def test_bpe_raw_binding_flags_long_rows():
    """Counts of the raw binding: -1 exactly for the rows over 4096 bytes."""
    texts = mc.bpe_texts("aa", False)
    s = mc.text_series(texts, DEV, "binary")
    tok = mc.bpe_table("aa").tokenizer
    byte2id, keys, vals = tok.tables(s.device)
    ids, counts = native_required().bpe_encode(s.offsets, s.data, byte2id,
                                               keys, vals)
    want = mc.expected_bpe("aa", texts)
    offs = s.offsets.cpu().tolist()
    ids, counts = ids.cpu().tolist(), counts.cpu().tolist()
    for i, x in enumerate(texts):
        if len(x) > mc.BPE_MAX_LEN:
            assert counts[i] == -1
        else:
            assert ids[offs[i]:offs[i] + counts[i]] == list(want[i]), i


def test_bpe_encode_refuses_bad_arguments():
    nat = native_required()
    off, data = _col3()
    byte2id, keys, vals = mc.bpe_table("aa").tokenizer.tables(off.device)
    sc.assert_refuses_bad_columns(
        "bpe_encode", lambda o, d: nat.bpe_encode(o, d, byte2id, keys, vals),
        off, data)
    for tables in ((byte2id.cpu(), keys, vals),
                   (byte2id.to(torch.int64), keys, vals),
                   (byte2id[:255], keys, vals),
                   (byte2id, keys.to(torch.int32), vals),
                   (byte2id, keys, vals.cpu()),
                   (byte2id, keys, vals[:-1])):
        with pytest.raises(RuntimeError, match="bpe_encode: "):
            nat.bpe_encode(off, data, *tables)
    ids, counts = nat.bpe_encode(off, data, byte2id, keys, vals)
    ids, counts, offs = ids.cpu().tolist(), counts.cpu().tolist(), \
        off.cpu().tolist()
    want = mc.expected_bpe("aa", tuple(_ROWS3))
    assert [ids[offs[i]:offs[i] + counts[i]] for i in range(3)] == \
        [list(w) for w in want]


# ---------------------------------------------------------------------------
# Levenshtein
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", mc.LAYOUTS)
def test_levenshtein_series(layout):
    tier.check_levenshtein(layout, DEV)


def test_levenshtein_expression():
    tier.check_levenshtein_expression(DEV)


def test_levenshtein_raw_binding_large():
    """n = 600 001 with max_len = 8: past the 2048-block grid, so the
    grid-stride loop runs, on a 9-int scratch row per pair."""
    pool, want = mc.lev_raw_pool()
    n = mc.LEV_RAW_N
    pick = (np.arange(n, dtype=np.int64) * 37 + np.arange(n) // 64) % 64
    sides = []
    for side in (0, 1):
        lens = np.array([len(p[side]) for p in pool], dtype=np.int64)[pick]
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        blob = np.frombuffer(b"".join(pool[j][side] for j in pick.tolist()),
                             dtype=np.uint8).copy()
        assert off[-1] == len(blob)
        sides += [torch.from_numpy(off).to(DEV),
                  torch.from_numpy(blob).to(DEV)]
    got = native_required().levenshtein(*sides, mc.LEV_RAW_MAX_LEN)
    assert got.dtype == torch.int32 and got.numel() == n
    expect = np.array(want, dtype=np.int32)[pick]
    bad = np.flatnonzero(got.cpu().numpy() != expect)
    assert bad.size == 0, [(int(i), pool[pick[i]]) for i in bad[:5]]


def test_levenshtein_raw_binding_flags_rows_for_the_host():
    """-1 for a pair with a row over max_len or with a byte >= 0x80."""
    a = [b"abc", b"abcdefghi", b"", "é".encode(), b"abcdefgh"]
    b = [b"abd", b"abc", b"abcdefghi", b"e", b"abcdefg\xc3"]
    sa = mc.text_series(a, DEV, "binary")
    sb = mc.text_series(b, DEV, "binary")
    got = native_required().levenshtein(sa.offsets, sa.data, sb.offsets,
                                        sb.data, 8)
    assert got.cpu().tolist() == [1, -1, -1, -1, -1]


def test_levenshtein_refuses_bad_arguments():
    nat = native_required()
    off, data = _col3()
    off4, data4 = _col4()
    sc.assert_refuses_bad_columns(
        "levenshtein", lambda o, d: nat.levenshtein(o, d, off, data, 8), off,
        data)
    sc.assert_refuses_bad_columns(
        "levenshtein", lambda o, d: nat.levenshtein(off, data, o, d, 8), off,
        data)
    with pytest.raises(RuntimeError, match="levenshtein: "):
        nat.levenshtein(off, data, off4, data4, 8)
    with pytest.raises(RuntimeError, match="levenshtein: "):
        nat.levenshtein(off4, data4, off, data, 8)
    other = [b"abd", b"e", b""]
    sb = mc.text_series(other, DEV, "binary")
    got = nat.levenshtein(off, data, sb.offsets, sb.data, 8)
    # -1: the row with a byte >= 0x80 is left to the host
    assert got.cpu().tolist() == \
        [mc.levenshtein_oracle(x, y) if x.isascii() else -1
         for x, y in zip(_ROWS3, other)] == [1, -1, 3]


# ---------------------------------------------------------------------------
# image resize
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.RESIZE_CASES)
def test_resize(name):
    tier.check_resize(name, DEV)


def test_resize_rejects_other_channel_counts():
    tier.check_resize_rejects_other_channel_counts(DEV)

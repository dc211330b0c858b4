"""The text-cleanup kernels (csrc/strtransform.hip: str_strip, str_right,
str_reverse, str_normalize_ascii) and the functions of
daft_amd/kernels/strings.py built on them and on the shared ragged copy
(normalize, strip / lstrip / rstrip, right, reverse, capitalize, lpad / rpad,
repeat, split), against the Python oracle of strtransform_cases.py: all 29
whitespace characters and their near misses, 64-byte chunk edges of the
wave-per-row normalizer, sizes that cross the block edge, sliced, dictionary
and null-over-bytes columns, and which path (kernels or host Python) a call
took.  All comparisons are exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import DataType, Series, col
from daft_amd.functions import strings_extra as fx
from daft_amd.kernels import native_required
from daft_amd.kernels import strings as strk

import strings_cases as sc
import strtransform_cases as tc

DEV = "cuda:0"
MATRIX = [(n, v) for n in tc.SIZES for v in tc.VARIANTS]
matrix = pytest.mark.parametrize("n,variant", MATRIX)
FLAG_TRIPLES = [(rp, lc, ws) for rp in (False, True) for lc in (False, True)
                for ws in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


def _column(values) -> Series:
    return Series.from_pylist("s", list(values), DataType.string(),
                              device=DEV)


def _rows(offsets, data) -> list:
    off = offsets.cpu().tolist()
    buf = bytes(data.cpu().tolist())
    assert off[0] == 0 and off[-1] == len(buf)
    return [buf[a:b] for a, b in zip(off[:-1], off[1:])]


# ---------------------------------------------------------------------------
# driver matrix: the drivers of the CPU tier on cuda:0
# ---------------------------------------------------------------------------

def test_corpus_guards():
    tc.corpus_guards()


@matrix
def test_strip(n, variant):
    tc.check_strip(n, variant, DEV)


@matrix
def test_right(n, variant):
    tc.check_right(n, variant, DEV)


@matrix
def test_reverse(n, variant):
    tc.check_reverse(n, variant, DEV)


@matrix
def test_capitalize(n, variant):
    tc.check_capitalize(n, variant, DEV)


@matrix
def test_pad(n, variant):
    tc.check_pad(n, variant, DEV)


@matrix
def test_repeat(n, variant):
    tc.check_repeat(n, variant, DEV)


@matrix
def test_split(n, variant):
    tc.check_split(n, variant, DEV)


@matrix
def test_normalize(n, variant):
    """All eight flag triples, nfd_unicode both ways."""
    assert len(tc.NORMALIZE_FLAGS) == 16
    tc.check_normalize(n, variant, DEV)


def test_negative_counts_and_errors():
    tc.check_negative_counts(DEV)
    tc.check_errors(DEV)


# ---------------------------------------------------------------------------
# raw bindings
# ---------------------------------------------------------------------------

def _raw_values(n: int) -> list:
    """`n` non-null rows: the fixed rows first, then the corpus."""
    pool = tc.FIXED_ROWS + [v for v in tc.corpus(4099) if v is not None]
    return pool[:n]


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_raw_normalize_ascii(n):
    """The kernel against the per-byte machine; row counts around the four
    waves of a block."""
    nat = native_required()
    vals = _raw_values(n)
    s = _column(vals)
    raw = [v.encode() for v in vals]
    high = [any(b >= 0x80 for b in r) for r in raw]
    assert n < 257 or (any(high) and not all(high))
    for rp, lc, ws in FLAG_TRIPLES:
        off, data, flagged = nat.str_normalize_ascii(
            s.offsets, s.data, None, rp, lc, ws)
        assert off.dtype == torch.int64 and off.shape == (n + 1,)
        assert data.dtype == torch.uint8 and flagged.dtype == torch.bool
        assert off.is_cuda and data.is_cuda and flagged.is_cuda
        assert flagged.cpu().tolist() == high
        assert _rows(off, data) == [
            b"" if h else tc.machine(r, rp, lc, ws)
            for r, h in zip(raw, high)]
    if n:
        # a null row is empty and not flagged, whatever bytes it owns
        valid = torch.tensor([i % 3 != 0 for i in range(n)], device=DEV)
        off, data, flagged = nat.str_normalize_ascii(
            s.offsets, s.data, valid, True, True, True)
        keep = valid.cpu().tolist()
        assert flagged.cpu().tolist() == [h and k for h, k in zip(high, keep)]
        assert _rows(off, data) == [
            b"" if h or not k else tc.machine(r, True, True, True)
            for r, h, k in zip(raw, high, keep)]


@pytest.mark.parametrize("n", [0, 1, 257, 4099])
def test_raw_strip_right_reverse(n):
    nat = native_required()
    vals = _raw_values(n)
    s = _column(vals)
    for mode, o in ((0, tc.o_strip), (1, tc.o_lstrip), (2, tc.o_rstrip)):
        off, data = nat.str_strip(s.offsets, s.data, mode)
        assert _rows(off, data) == [v.encode() for v in o(vals)]
    for k in tc.RIGHT_ARGS:
        off, data = nat.str_right(s.offsets, s.data, k)
        assert _rows(off, data) == [v.encode() for v in tc.o_right(vals, k)]
    off, data = nat.str_reverse(s.offsets, s.data)
    assert off.cpu().tolist() == s.offsets.cpu().tolist()
    assert _rows(off, data) == [v.encode() for v in tc.o_reverse(vals)]


def test_raw_invalid_utf8_and_offsets_above_zero():
    """Bytes that are no UTF-8: a truncated space at the row's end, a row of
    continuation bytes.  The scans stay inside the row, and reverse permutes
    every row onto itself."""
    nat = native_required()
    rows = [b" a\xe2\x80", b"\x80 ", b"\xc2", b"\xa0x", b"\x85\xa0",
            b"\xe2\x80\x80", b"a\xe2\x80\x80", b"", b"\x80\xe2", b"x"]
    # read across the row edge, rows 0 + 1 hold U+2000 (forwards from row 0,
    # backwards from row 1) and rows 2 + 3 hold U+00A0
    assert (rows[0] + rows[1])[2:5].decode() == "\u2000"
    assert (rows[2] + rows[3])[:2].decode() == "\xa0"
    lens = [len(r) for r in rows]
    off = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(rows))],
                       dtype=torch.int64, device=DEV)
    data = torch.frombuffer(bytearray(b"".join(rows)),
                            dtype=torch.uint8).to(DEV)
    stripped = [b"a\xe2\x80", b"\x80", b"\xc2", b"\xa0x", b"\x85\xa0", b"",
                b"a", b"", b"\x80\xe2", b"x"]
    last = [b"\xe2\x80", b" ", b"\xc2", b"x", b"\x85\xa0", b"\xe2\x80\x80",
            b"\xe2\x80\x80", b"", b"\xe2", b"x"]
    assert _rows(*nat.str_strip(off, data, 0)) == stripped
    assert _rows(*nat.str_right(off, data, 1)) == last
    got = _rows(*nat.str_reverse(off, data))
    assert [sorted(g) for g in got] == [sorted(r) for r in rows]
    assert got[:4] == [b"\xe2\x80a ", b" \x80", b"\xc2", b"x\xa0"]
    # offsets that start above 0, over the whole byte buffer
    sub = off[3:8]
    assert int(sub[0]) > 0
    assert _rows(*nat.str_strip(sub, data, 0)) == stripped[3:7]
    assert _rows(*nat.str_right(sub, data, 1)) == last[3:7]
    assert _rows(*nat.str_reverse(sub, data)) == got[3:7]
    o, d, flagged = nat.str_normalize_ascii(sub, data, None, True, True, True)
    assert _rows(o, d) == [b""] * 4 and flagged.cpu().tolist() == [True] * 4


def test_raw_bindings_refuse_bad_columns():
    """A bad column fails on the host, before any launch; the valid call
    after each group still gives the oracle's answer."""
    nat = native_required()
    vals = sc.REFUSED_VALUES
    s = _column(vals)
    n = len(vals)
    calls = {
        "str_strip": lambda o, d: nat.str_strip(o, d, 0),
        "str_right": lambda o, d: nat.str_right(o, d, 1),
        "str_reverse": lambda o, d: nat.str_reverse(o, d),
        "str_normalize_ascii":
            lambda o, d: nat.str_normalize_ascii(o, d, None, True, True, True),
    }
    for name, call in calls.items():
        sc.assert_refuses_bad_columns(name, call, s.offsets, s.data)
    for bad in (torch.ones(n + 1, dtype=torch.bool, device=DEV),
                torch.ones(n - 1, dtype=torch.bool, device=DEV),
                torch.ones(n, dtype=torch.uint8, device=DEV),
                torch.ones(n, dtype=torch.bool),                  # on the CPU
                torch.ones(2 * n, dtype=torch.bool, device=DEV)[::2]):
        with pytest.raises(RuntimeError, match="str_normalize_ascii: "):
            nat.str_normalize_ascii(s.offsets, s.data, bad, True, True, True)
    with pytest.raises(RuntimeError, match="str_strip: "):
        nat.str_strip(s.offsets, s.data, 3)
    with pytest.raises(RuntimeError, match="str_right: "):
        nat.str_right(s.offsets, s.data, -1)
    assert _rows(*nat.str_strip(s.offsets, s.data, 0)) == \
        [v.encode() for v in vals]
    assert _rows(*nat.str_right(s.offsets, s.data, 1)) == \
        [v[-1:].encode() for v in vals]
    assert _rows(*nat.str_reverse(s.offsets, s.data)) == \
        [v[::-1].encode() for v in vals]
    off, data, flagged = nat.str_normalize_ascii(
        s.offsets, s.data, torch.ones(n, dtype=torch.bool, device=DEV),
        True, True, True)
    assert _rows(off, data) == [b"ab", b"", b"abc"]
    assert flagged.cpu().tolist() == [False, True, False]


# ---------------------------------------------------------------------------
# which path ran
# ---------------------------------------------------------------------------

def _boom(what):
    def boom(*a, **k):
        raise AssertionError(what + " taken")
    return boom


def test_normalize_of_ascii_never_reaches_the_host(monkeypatch):
    monkeypatch.setattr(strk, "_host_normalize", _boom("host normalize"))
    monkeypatch.setattr(strk, "_map_python", _boom("_map_python"))
    for variant in tc.VARIANTS:
        s, vals = tc.ascii_column(4099, variant, DEV)
        for flags in tc.NORMALIZE_FLAGS:
            sc.assert_strings(strk.normalize(s, *flags),
                              tc.o_normalize(vals, *flags))
    # through the public function too
    s, vals = tc.ascii_column(257, "plain", DEV)
    node = fx.normalize(col("s"), remove_punct=True)._node
    sc.assert_strings(node.fn(s), tc.o_normalize(vals, True, True, True, True))


@pytest.mark.parametrize("variant", ["plain", "masked"])
def test_normalize_sends_only_non_ascii_rows_to_the_host(monkeypatch, variant):
    s, vals = tc.column(4099, variant, DEV)
    seen = []
    real = strk._host_normalize

    def spy(part, *flags):
        seen.append((part.to_pylist(), flags))
        return real(part, *flags)
    monkeypatch.setattr(strk, "_host_normalize", spy)
    monkeypatch.setattr(strk, "_map_python", _boom("_map_python"))
    want_rows = [v for v in vals if v is not None and not v.isascii()]
    assert 0.05 < len(want_rows) / len(vals) < 0.60
    for flags in ((False, True, True, True), (True, False, False, False)):
        del seen[:]
        sc.assert_strings(strk.normalize(s, *flags),
                          tc.o_normalize(vals, *flags))
        assert seen == [(want_rows, flags)]


def test_cleanup_functions_do_not_touch_the_host(monkeypatch):
    """strip, lstrip, rstrip, right, reverse, lpad, rpad, repeat and ASCII
    capitalize with the per-row Python map taken away."""
    monkeypatch.setattr(strk, "_map_python", _boom("_map_python"))
    for variant in tc.VARIANTS:
        tc.check_strip(4099, variant, DEV)
        tc.check_right(4099, variant, DEV)
        tc.check_reverse(4099, variant, DEV)
        tc.check_pad(4099, variant, DEV)
        tc.check_repeat(4099, variant, DEV)
        s, vals = tc.ascii_column(4099, variant, DEV)
        sc.assert_strings(strk.capitalize(s), tc.o_capitalize(vals))


def test_split_takes_the_span_kernels(monkeypatch):
    monkeypatch.setattr(strk, "_host_regexp_split", _boom("host split"))
    monkeypatch.setattr(strk, "_pylist_str", _boom("host split"))
    for variant in ("plain", "dict"):
        s, vals = tc.column(4099, variant, DEV)
        for sep in tc.SEPARATORS:
            tc.assert_lists(strk.split(s, sep), tc.o_split(vals, sep))


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

def test_dataframe_select():
    vals = tc.corpus(4099)

    def query(**kw):
        return daft.from_pydict({"s": vals}, **kw).select(
            fx.normalize(col("s"), remove_punct=True).alias("n"),
            col("s").str.strip().alias("t"),
            col("s").str.lpad(12, "é").alias("p"),
        ).to_pydict()
    want = query()
    assert query(device=DEV) == want
    assert want == {"n": tc.o_normalize(vals, True, True, True, True),
                    "t": tc.o_strip(vals),
                    "p": tc.o_lpad(vals, 12, "é")}

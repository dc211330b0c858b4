"""The DFA match kernel (csrc/regex.hip) and its routing in
daft_amd/kernels/strings.py against Python `re` and the host table walk:
multi-byte UTF-8, `$` before a final newline, sizes that cross the
256-thread block edge, sliced, dictionary and null-over-bytes columns, and
which of the two paths (kernel or host `re`) a call took.  All comparisons
are exact."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import DataType, Series, col
from daft_amd.kernels import native_required, regex_dfa as rd
from daft_amd.kernels import strings as strk

import regex_cases as rc
import strings_cases as sc

DEV = "cuda:0"
MATRIX = [(n, v) for n in sc.SIZES for v in sc.VARIANTS]
matrix = pytest.mark.parametrize("n,variant", MATRIX)
RAW_SIZES = [257, 4099]
BLOCK = 256


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


def _column(values) -> Series:
    return Series.from_pylist("s", list(values), DataType.string(),
                              device=DEV)


def _run(prog: rd.Program, s: Series) -> list:
    t = [torch.from_numpy(a).to(DEV)
         for a in (prog.table, prog.byte_class, prog.flags)]
    out = native_required().regex_match(s.offsets, s.data, t[0], t[1], t[2],
                                        prog.n_classes, prog.start)
    assert out.dtype == torch.bool and out.shape == (len(s),)
    return out.cpu().tolist()


# ---------------------------------------------------------------------------
# raw binding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ascii_only", [False, True])
@pytest.mark.parametrize("n", RAW_SIZES)
def test_raw_regex_match(n, ascii_only):
    """Every supported pattern that is valid for the column: all of them on
    the ASCII column, those that are not ASCII-only on the UTF-8 one."""
    assert n > BLOCK and n % BLOCK != 0     # a second, partly filled block
    vals = rc.raw_values(n, ascii_only)
    s = _column(vals)
    assert s.validity is None and s.is_gpu()
    ran = 0
    for pattern, needs_ascii in rc.SUPPORTED:
        if needs_ascii and not ascii_only:
            continue
        prog = rd.compile(pattern, "search")
        want = list(rc.raw_expected(n, ascii_only, pattern))
        got = _run(prog, s)
        assert got == want, pattern
        assert got == [prog.match_host(v.encode()) for v in vals], pattern
        ran += 1
    assert ran == (len(rc.SUPPORTED) if ascii_only else
                   sum(not a for _, a in rc.SUPPORTED))
    # rows past the first block: one at 257, both answers among 4099
    past = rc.raw_expected(n, ascii_only, r"a")[BLOCK:]
    assert len(past) == n - BLOCK >= 1
    assert n == 257 or {True, False} == set(past)


def test_raw_regex_match_edges():
    """`$` before one final newline, the empty row, single characters of
    every width, and rows that touch their neighbours."""
    vals = ["a\n", "a\n\n", "", "\n", "😀", sc.ALL_MULTIBYTE_40,
            "a", "a", "\na", "a\n", "😀a", "a😀", "", "", "é", "\n\n", "😀\n",
            "aa", "€", "b"]
    s = _column(vals)
    assert rc.o_search(vals, r"a$")[:2] == [True, False]
    assert rc.o_search(vals, r"a\Z")[:2] == [False, False]
    assert rc.o_search(vals, r"^$")[2:4] == [True, True]
    for pattern in (r"a$", r"a\Z", r"^$", r".", r"(?s).", r"[^a]", r"😀$"):
        prog = rd.compile(pattern, "search")
        assert _run(prog, s) == rc.o_search(vals, pattern), pattern
        full = rd.compile(pattern, "full")
        rx = re.compile(pattern)
        assert _run(full, s) == [rx.fullmatch(v) is not None for v in vals], \
            pattern


def test_raw_regex_match_empty_and_sliced():
    nat = native_required()
    prog = rd.compile(r"a.b", "search")
    t = [torch.from_numpy(a).to(DEV)
         for a in (prog.table, prog.byte_class, prog.flags)]
    # no rows, and rows with no bytes at all
    for vals in ([], ["", "", ""]):
        s = _column(vals)
        assert s.data.numel() == 0
        out = nat.regex_match(s.offsets, s.data, t[0], t[1], t[2],
                              prog.n_classes, prog.start)
        assert out.cpu().tolist() == [False] * len(vals)
    vals = rc.raw_values(257, False)
    want = list(rc.raw_expected(257, False, r"a.b"))
    whole = _column(vals)
    # a sliced column: `data` is a view at a non-zero storage offset
    s = whole.slice(3, 255)
    assert s.data.storage_offset() > 0
    assert _run(prog, s) == want[3:255]
    # offsets that start above 0, over the whole byte buffer
    offs = whole.offsets[3:256]
    assert int(offs[0]) > 0 and offs.storage_offset() == 3
    out = nat.regex_match(offs, whole.data, t[0], t[1], t[2],
                          prog.n_classes, prog.start)
    assert out.cpu().tolist() == want[3:255]


def test_raw_regex_match_refuses_bad_programs():
    """A bad program fails on the host, before any launch."""
    nat = native_required()
    s = _column(["ab", "c"])
    prog = rd.compile(r"a.b", "search")
    table, byte_class, flags = [
        torch.from_numpy(a).to(DEV)
        for a in (prog.table, prog.byte_class, prog.flags)]

    def call(table=table, byte_class=byte_class, flags=flags,
             n_classes=prog.n_classes, start=prog.start):
        return nat.regex_match(s.offsets, s.data, table, byte_class, flags,
                               n_classes, start)
    assert call().cpu().tolist() == [False, False]
    with pytest.raises(RuntimeError):
        call(table=table.to(torch.int32))
    with pytest.raises(RuntimeError):
        call(byte_class=byte_class.to(torch.int64))
    with pytest.raises(RuntimeError):
        call(flags=flags.to(torch.bool))
    with pytest.raises(RuntimeError):
        call(n_classes=prog.n_classes + 1)
    with pytest.raises(RuntimeError):
        call(start=prog.n_states)
    with pytest.raises(RuntimeError):
        call(byte_class=byte_class[:255])
    # 2 classes x 17000 states: 68000 + 256 + 17000 bytes > 64 KiB of LDS
    big_states = 17000
    with pytest.raises(RuntimeError, match="LDS"):
        call(table=torch.zeros(big_states * 2, dtype=torch.int16, device=DEV),
             flags=torch.zeros(big_states, dtype=torch.uint8, device=DEV),
             n_classes=2, start=0)


def test_raw_regex_match_refuses_bad_columns():
    """A bad column or a table on the CPU fails on the host, before any
    launch; the valid call afterwards still gives the oracle's answer."""
    nat = native_required()
    vals = sc.REFUSED_VALUES
    s = _column(vals)
    prog = rd.compile(r"a.", "search")
    table, byte_class, flags = [
        torch.from_numpy(a).to(DEV)
        for a in (prog.table, prog.byte_class, prog.flags)]

    def call(o, d, table=table, byte_class=byte_class, flags=flags):
        return nat.regex_match(o, d, table, byte_class, flags,
                               prog.n_classes, prog.start)
    sc.assert_refuses_bad_columns("regex_match", call, s.offsets, s.data)
    for bad in (dict(table=table.cpu()), dict(byte_class=byte_class.cpu()),
                dict(flags=flags.cpu()),
                dict(flags=torch.cat([flags, flags])[::2])):
        with pytest.raises(RuntimeError, match="regex_match: "):
            call(s.offsets, s.data, **bad)
    assert call(s.offsets, s.data).cpu().tolist() == \
        rc.o_search(vals, r"a.") == [True, False, True]


# ---------------------------------------------------------------------------
# wrappers: daft_amd/kernels/strings.py on cuda:0 Series
# ---------------------------------------------------------------------------

# two are ASCII-only, `(a)\1` is outside the engine and falls back
WRAPPER_PATTERNS = [r"a.b", r"^a|b$", r"[^a\n]b", r"\d+", r"(?i)ab",
                    r"(a)\1"]
WRAPPER_LIKES = [("a_", False), ("%_b", False), ("_%", False),
                 ("%a_b%", False), ("%AB%", True), ("a_", True)]


def _columns(n, variant):
    """The shared UTF-8 corpus and the all-ASCII one, as the same variant."""
    yield sc.column(n, variant, DEV)
    yield sc.make_variant(rc.ascii_corpus(n, nulls=True), variant, DEV)


@matrix
def test_regexp_match(n, variant):
    for s, vals in _columns(n, variant):
        assert s.is_gpu() and len(s) == len(vals)
        for pattern in WRAPPER_PATTERNS:
            sc.assert_bool(strk.regexp_match(s, pattern),
                           rc.o_search(vals, pattern), s)


@matrix
def test_like_underscore_and_ilike(n, variant):
    for s, vals in _columns(n, variant):
        for pattern, ci in WRAPPER_LIKES:
            sc.assert_bool(strk.like(s, pattern, case_insensitive=ci),
                           sc.o_like(vals, pattern, ci=ci), s)


def test_wrapper_patterns_are_what_they_claim():
    assert [rd.compile(p).needs_ascii for p in WRAPPER_PATTERNS[:5]] == \
        [False, False, False, True, True]
    with pytest.raises(rd.Unsupported):
        rd.compile(WRAPPER_PATTERNS[5])
    vals = [v for v in rc.ascii_corpus(4099, nulls=True) if v is not None]
    for pattern in WRAPPER_PATTERNS[:5]:
        assert {True, False} == set(rc.o_search(vals, pattern)), pattern
    for pattern, ci in WRAPPER_LIKES:
        assert {True, False} == set(sc.o_like(vals, pattern, ci=ci)), pattern


# ---------------------------------------------------------------------------
# which path ran
# ---------------------------------------------------------------------------

def test_supported_patterns_do_not_touch_the_host(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("host regex path taken")
    monkeypatch.setattr(strk, "_host_regex_pred", boom)
    s, vals = sc.column(4099, "plain", DEV)
    for pattern in (r"a.b", r"^a|b$", r"[^a\n]b", r"é+", r"a$"):
        sc.assert_bool(strk.regexp_match(s, pattern),
                       rc.o_search(vals, pattern), s)
    for pattern in ("a_", "%_b", "%é_%"):
        sc.assert_bool(strk.like(s, pattern), sc.o_like(vals, pattern), s)
    avals = rc.ascii_corpus(4099, nulls=True)
    a, avals = sc.make_variant(avals, "plain", DEV)
    for pattern in (r"\d+", r"(?i)ab", r"^[A-Z][a-z]+ \d{2,4}$"):
        sc.assert_bool(strk.regexp_match(a, pattern),
                       rc.o_search(avals, pattern), a)
    for pattern in ("%AB%", "a_", "ab"):
        sc.assert_bool(strk.like(a, pattern, case_insensitive=True),
                       sc.o_like(avals, pattern, ci=True), a)


@pytest.mark.parametrize("pattern,ascii_column", [
    (r"\d+", False),            # ASCII-only program, column holds `é`
    (r"(a)\1", True),           # backreference
    (rc.STATE_BOMB, True),      # over the state cap
])
def test_fallbacks_call_the_host_once(monkeypatch, pattern, ascii_column):
    calls = []
    real = strk._host_regex_pred

    def spy(s, rx, full):
        calls.append(rx.pattern)
        return real(s, rx, full)
    monkeypatch.setattr(strk, "_host_regex_pred", spy)
    vals = rc.ascii_corpus(257, nulls=True)
    if not ascii_column:
        vals = vals + ["é1", "é"]
    s = _column(vals)
    sc.assert_bool(strk.regexp_match(s, pattern),
                   rc.o_search(vals, pattern), s)
    assert calls == [pattern]


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

def test_dataframe_where_str_match():
    vals = sc.corpus(4099)
    want = daft.from_pydict({"s": vals}) \
        .where(col("s").str.match(r"^a.*b$")).to_pydict()
    got = daft.from_pydict({"s": vals}, device=DEV) \
        .where(col("s").str.match(r"^a.*b$")).to_pydict()
    assert got == want
    assert want["s"] == [v for v in vals
                         if v is not None and re.search(r"^a.*b$", v)]
    assert 10 < len(want["s"]) < 4000


def test_sql_where_ilike():
    vals = sc.corpus(4099)
    q = "select s from t where s ILIKE '%a_b%'"
    t = daft.from_pydict({"s": vals})
    want = daft.sql(q).to_pydict()
    t = daft.from_pydict({"s": vals}, device=DEV)   # noqa: F841
    got = daft.sql(q).to_pydict()
    assert got == want
    assert want["s"] == [v for v, hit in
                         zip(vals, sc.o_like(vals, "%a_b%", ci=True)) if hit]
    assert 10 < len(want["s"]) < 4000

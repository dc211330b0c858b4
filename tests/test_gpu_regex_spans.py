"""The match-position kernels (csrc/regex.hip: regex_count, regex_spans;
csrc/strings.hip: copy_segments) and the five functions built on them in
daft_amd/kernels/strings.py, against Python `re` and the host table walk:
multi-byte UTF-8, adjacent matches, row boundaries, sizes that cross the
256-thread block edge, sliced, dictionary and null-over-bytes columns, and
which of the two paths (kernels or host `re`) a call took.  All comparisons
are exact."""
import random
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import DataType, Series, col
from daft_amd.functions import strings_extra as fx
from daft_amd.kernels import native_required, regex_dfa as rd
from daft_amd.kernels import strings as strk

import regex_cases as rc
import regex_span_cases as spc
import strings_cases as sc

DEV = "cuda:0"
MATRIX = [(n, v) for n in sc.SIZES for v in sc.VARIANTS]
matrix = pytest.mark.parametrize("n,variant", MATRIX)
RAW_SIZES = [257, 4099]
BLOCK = 256
HOST_HELPERS = ["_host_regexp_count", "_host_regexp_extract",
                "_host_regexp_extract_all", "_host_regexp_replace",
                "_host_regexp_split"]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


def _column(values) -> Series:
    return Series.from_pylist("s", list(values), DataType.string(),
                              device=DEV)


def _tables(prog: rd.SpanProgram) -> dict:
    t = {k: torch.from_numpy(getattr(prog, k)).to(DEV)
         for k in ("fwd_table", "byte_class", "fwd_flags", "rev_table",
                   "rev_flags")}
    t.update(n_classes=prog.n_classes, start=prog.start,
             rev_start=prog.rev_start)
    return t


def _count(t: dict, offsets, data, valid=None, limit=-1) -> torch.Tensor:
    out = native_required().regex_count(
        offsets, data, valid, t["fwd_table"], t["byte_class"],
        t["fwd_flags"], t["n_classes"], t["start"], limit)
    assert out.dtype == torch.int64 and out.shape == (offsets.numel() - 1,)
    assert out.is_cuda
    return out


def _spans(t: dict, offsets, data, valid=None, limit=-1):
    """(counts, per row the list of spans relative to the row's start)."""
    counts = _count(t, offsets, data, valid, limit)
    n = counts.numel()
    mo = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    mo[1:] = torch.cumsum(counts, 0)
    starts, ends = native_required().regex_spans(
        offsets, data, valid, t["fwd_table"], t["byte_class"],
        t["fwd_flags"], t["n_classes"], t["start"], t["rev_table"],
        t["rev_flags"], t["rev_start"], mo, limit)
    m = int(mo[-1])
    assert starts.dtype == ends.dtype == torch.int64
    assert starts.shape == ends.shape == (m,)
    st, en, mol = starts.cpu().tolist(), ends.cpu().tolist(), mo.cpu().tolist()
    off = offsets.cpu().tolist()
    rows = [[(st[k] - off[i], en[k] - off[i])
             for k in range(mol[i], mol[i + 1])] for i in range(n)]
    return counts.cpu().tolist(), rows


def _run(prog, s: Series, limit=-1):
    return _spans(_tables(prog), s.offsets, s.data, s.validity, limit)


# ---------------------------------------------------------------------------
# raw bindings
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ascii_only", [False, True])
@pytest.mark.parametrize("n", RAW_SIZES)
def test_raw_count_and_spans(n, ascii_only):
    """Every supported pattern that is valid for the column: all of them on
    the ASCII column, those that are not ASCII-only on the UTF-8 one."""
    vals = list(rc.raw_values(n, ascii_only)) + spc.EXTRA_ROWS
    assert len(vals) > BLOCK and len(vals) % BLOCK != 0
    s = _column(vals)
    assert s.validity is None and s.is_gpu()
    ran = 0
    for pattern, needs_ascii in spc.SPAN_SUPPORTED:
        if needs_ascii and not ascii_only:
            continue
        prog = rd.compile_spans(pattern)
        want = [list(w) for w in spc.raw_spans(n, ascii_only, pattern)] + \
            spc.o_spans(spc.EXTRA_ROWS, pattern)
        counts, rows = _run(prog, s)
        assert counts == [len(w) for w in want], pattern
        assert rows == want, pattern
        assert rows == [prog.spans_host(v.encode()) for v in vals], pattern
        ran += 1
    assert ran == (len(spc.SPAN_SUPPORTED) if ascii_only else
                   sum(not a for _, a in spc.SPAN_SUPPORTED))
    # rows past the first block have matches, and rows without any
    past = spc.raw_spans(n, ascii_only, r"a")[BLOCK:]
    assert len(past) == n - BLOCK >= 1
    assert n == 257 or {True, False} == {bool(w) for w in past}


def test_raw_edges():
    t_aa = _tables(rd.compile_spans(r"aa"))
    t_ab = _tables(rd.compile_spans(r"ab"))
    t_a = _tables(rd.compile_spans(r"a"))
    t_dot = _tables(rd.compile_spans(r"(?s)."))
    # adjacent matches
    s = _column(["aaaa", "aaa", "a"])
    assert _spans(t_aa, s.offsets, s.data) == \
        ([2, 1, 0], [[(0, 2), (2, 4)], [(0, 2)], []])
    # no match across a row boundary
    s = _column(["a", "b", "ab", "a", "b"])
    assert _spans(t_ab, s.offsets, s.data) == \
        ([0, 0, 1, 0, 0], [[], [], [(0, 2)], [], []])
    # a match at byte 0 and one at the last byte
    s = _column(["abba", "a", "bba", "abb"])
    assert _spans(t_a, s.offsets, s.data) == \
        ([2, 1, 1, 1], [[(0, 1), (3, 4)], [(0, 1)], [(2, 3)], [(0, 1)]])
    # a 4-byte character alone, and 40 multi-byte characters
    s = _column(["😀", sc.ALL_MULTIBYTE_40, ""])
    width = [len(c.encode()) for c in sc.ALL_MULTIBYTE_40]
    edges = [sum(width[:i]) for i in range(41)]
    assert _spans(t_dot, s.offsets, s.data) == \
        ([1, 40, 0], [[(0, 4)], list(zip(edges[:-1], edges[1:])), []])
    assert spc.o_spans(["😀", sc.ALL_MULTIBYTE_40], r"(?s).") == \
        [[(0, 4)], list(zip(edges[:-1], edges[1:]))]
    # one long row
    s = _column(["ab" * 2500, "b"])
    counts, rows = _spans(t_ab, s.offsets, s.data)
    assert counts == [2500, 0]
    assert rows[0] == [(2 * k, 2 * k + 2) for k in range(2500)]
    # limit
    assert _spans(t_ab, s.offsets, s.data, limit=1) == ([1, 0], [[(0, 2)], []])
    assert _spans(t_ab, s.offsets, s.data, limit=3) == \
        ([3, 0], [[(0, 2), (2, 4), (4, 6)], []])
    # a null row that owns bytes counts 0 and writes no span
    s = _column(["ab", "abab", "xab"])
    valid = torch.tensor([True, False, True], device=DEV)
    assert s.data.numel() == 9
    assert _spans(t_ab, s.offsets, s.data, valid) == \
        ([1, 0, 1], [[(0, 2)], [], [(1, 3)]])


def test_raw_empty_and_sliced():
    prog = rd.compile_spans(r"a.b")
    t = _tables(prog)
    # no rows, and rows with no bytes at all
    for vals in ([], ["", "", ""]):
        s = _column(vals)
        assert s.data.numel() == 0
        assert _spans(t, s.offsets, s.data) == \
            ([0] * len(vals), [[] for _ in vals])
    vals = rc.raw_values(257, False)
    want = [list(w) for w in spc.raw_spans(257, False, r"a.b")]
    assert sum(map(len, want)) > 20
    whole = _column(vals)
    # a sliced column: `data` is a view at a non-zero storage offset
    s = whole.slice(3, 255)
    assert s.data.storage_offset() > 0
    assert _run(prog, s)[1] == want[3:255]
    # offsets that start above 0, over the whole byte buffer
    offs = whole.offsets[3:256]
    assert int(offs[0]) > 0 and offs.storage_offset() == 3
    assert _spans(t, offs, whole.data)[1] == want[3:255]


@pytest.mark.parametrize("k", [0, 257, 4099])
def test_raw_copy_segments(k):
    nat = native_required()
    rng = random.Random(k)
    src = bytes(rng.randrange(256) for _ in range(5000))
    lens = [rng.randrange(0, 41) for _ in range(k)]
    # runs of empty segments: at the start, in the middle, at the end
    for lo, hi in ((0, 3), (k // 2, k // 2 + 70), (k - 5, k)):
        for i in range(max(lo, 0), min(hi, k)):
            lens[i] = 0
    begin = [rng.randrange(0, len(src) - 40) for _ in range(k)]
    off = [0]
    for ln in lens:
        off.append(off[-1] + ln)
    out = nat.copy_segments(
        torch.frombuffer(bytearray(src), dtype=torch.uint8).to(DEV),
        torch.tensor(begin, dtype=torch.int64, device=DEV),
        torch.tensor(off, dtype=torch.int64, device=DEV))
    assert out.dtype == torch.uint8 and out.is_cuda
    want = b"".join(src[b:b + ln] for b, ln in zip(begin, lens))
    assert out.shape == (len(want),)
    assert bytes(out.cpu().tolist()) == want
    assert k == 0 or len(want) > 20 * k // 2


def test_raw_bindings_refuse_bad_programs():
    """A bad program fails on the host, before any launch."""
    nat = native_required()
    s = _column(["ab", "c"])
    prog = rd.compile_spans(r"a.b")
    good = _tables(prog)
    mo = torch.zeros(3, dtype=torch.int64, device=DEV)

    def count(limit=-1, valid=None, **kw):
        t = dict(good, **kw)
        return nat.regex_count(s.offsets, s.data, valid, t["fwd_table"],
                               t["byte_class"], t["fwd_flags"],
                               t["n_classes"], t["start"], limit)

    def spans(limit=-1, match_offsets=mo, **kw):
        t = dict(good, **kw)
        return nat.regex_spans(s.offsets, s.data, None, t["fwd_table"],
                               t["byte_class"], t["fwd_flags"],
                               t["n_classes"], t["start"], t["rev_table"],
                               t["rev_flags"], t["rev_start"], match_offsets,
                               limit)
    assert count().cpu().tolist() == [0, 0]
    assert [x.numel() for x in spans()] == [0, 0]
    big_states = 17000
    big = dict(fwd_table=torch.zeros(big_states * 2, dtype=torch.int16,
                                     device=DEV),
               fwd_flags=torch.zeros(big_states, dtype=torch.uint8,
                                     device=DEV), n_classes=2, start=0,
               rev_table=torch.zeros(2, dtype=torch.int16, device=DEV),
               rev_flags=torch.zeros(1, dtype=torch.uint8, device=DEV),
               rev_start=0)
    for call in (count, spans):
        with pytest.raises(RuntimeError):
            call(fwd_table=good["fwd_table"].to(torch.int32))
        with pytest.raises(RuntimeError):
            call(byte_class=good["byte_class"].to(torch.int64))
        with pytest.raises(RuntimeError):
            call(fwd_flags=good["fwd_flags"].to(torch.bool))
        with pytest.raises(RuntimeError):
            call(n_classes=prog.n_classes + 1)
        with pytest.raises(RuntimeError):
            call(start=prog.fwd_table.shape[0])
        with pytest.raises(RuntimeError):
            call(byte_class=good["byte_class"][:255])
        with pytest.raises(RuntimeError):
            call(limit=0)
        # 2 classes x 17000 states: 68000 + 256 + 17000 bytes > 64 KiB of LDS
        with pytest.raises(RuntimeError, match="LDS"):
            call(**big)
    with pytest.raises(RuntimeError):
        count(valid=torch.ones(3, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError):
        count(valid=torch.ones(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        spans(rev_table=good["rev_table"].to(torch.int32))
    with pytest.raises(RuntimeError):
        spans(rev_flags=good["rev_flags"].to(torch.bool))
    with pytest.raises(RuntimeError):
        spans(rev_start=prog.rev_table.shape[0])
    with pytest.raises(RuntimeError):
        spans(rev_table=good["rev_table"][:-1])
    with pytest.raises(RuntimeError):
        spans(match_offsets=mo[:2])
    with pytest.raises(RuntimeError):
        spans(match_offsets=mo.to(torch.int32))
    # forward and reverse tables that fit alone but not together
    half = 9000
    with pytest.raises(RuntimeError, match="LDS"):
        spans(fwd_table=torch.zeros(half * 2, dtype=torch.int16, device=DEV),
              fwd_flags=torch.zeros(half, dtype=torch.uint8, device=DEV),
              rev_table=torch.zeros(half * 2, dtype=torch.int16, device=DEV),
              rev_flags=torch.zeros(half, dtype=torch.uint8, device=DEV),
              n_classes=2, start=0, rev_start=0)
    src = torch.zeros(8, dtype=torch.uint8, device=DEV)
    seg = torch.zeros(2, dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 2, 4], dtype=torch.int64, device=DEV)
    assert nat.copy_segments(src, seg, off).numel() == 4
    with pytest.raises(RuntimeError):
        nat.copy_segments(src.to(torch.int8), seg, off)
    with pytest.raises(RuntimeError):
        nat.copy_segments(src, seg.to(torch.int32), off)
    with pytest.raises(RuntimeError):
        nat.copy_segments(src, seg, off[:2])
    with pytest.raises(RuntimeError):
        nat.copy_segments(src, seg, off + 1)


def test_raw_bindings_refuse_bad_columns():
    """A bad column fails on the host, before any launch; the valid call
    after each group still gives the oracle's answer."""
    nat = native_required()
    vals = sc.REFUSED_VALUES
    s = _column(vals)
    t = _tables(rd.compile_spans(r"a."))
    want = spc.o_spans(vals, r"a.")
    assert want == [[(0, 2)], [], [(0, 2)]]
    mo = torch.tensor([0, 1, 1, 2], dtype=torch.int64, device=DEV)

    def spans(o, d, match_offsets=mo, **kw):
        g = dict(t, **kw)
        return nat.regex_spans(o, d, None, g["fwd_table"], g["byte_class"],
                               g["fwd_flags"], g["n_classes"], g["start"],
                               g["rev_table"], g["rev_flags"], g["rev_start"],
                               match_offsets, -1)
    sc.assert_refuses_bad_columns(
        "regex_count", lambda o, d: _count(t, o, d), s.offsets, s.data)
    with pytest.raises(RuntimeError, match="regex_count: "):
        _count(dict(t, fwd_table=t["fwd_table"].cpu()), s.offsets, s.data)
    with pytest.raises(RuntimeError, match="regex_count: "):
        _count(t, s.offsets, s.data,
               valid=torch.ones(3, dtype=torch.bool))       # on the CPU
    sc.assert_refuses_bad_columns("regex_spans", spans, s.offsets, s.data)
    for bad in (dict(rev_flags=t["rev_flags"].cpu()),
                dict(match_offsets=mo.cpu()),
                dict(match_offsets=torch.cat([mo, mo])[::2])):
        with pytest.raises(RuntimeError, match="regex_spans: "):
            spans(s.offsets, s.data, **bad)
    assert _spans(t, s.offsets, s.data) == ([len(w) for w in want], want)

    # copy_segments: out_offsets and src are its column
    seg = torch.tensor([3, 0, 5], dtype=torch.int64, device=DEV)
    sc.assert_refuses_bad_columns(
        "copy_segments", lambda o, d: nat.copy_segments(d, seg, o),
        s.offsets, s.data)
    for bad in (seg.cpu(), seg[:2], torch.cat([seg, seg])[::2]):
        with pytest.raises(RuntimeError, match="copy_segments: "):
            nat.copy_segments(s.data, bad, s.offsets)
    buf = "".join(vals).encode()
    lens = [len(v.encode()) for v in vals]
    assert bytes(nat.copy_segments(s.data, seg, s.offsets).cpu().tolist()) \
        == b"".join(buf[b:b + n] for b, n in zip(seg.cpu().tolist(), lens))


# ---------------------------------------------------------------------------
# wrappers: daft_amd/kernels/strings.py on cuda:0 Series
# ---------------------------------------------------------------------------

# two are ASCII-only; `^a` is outside span mode and falls back
WRAPPER_PATTERNS = [r"ab|b", r"é+|a{2,3}", r"\w+", r"(?i)ab", r"^a"]
REPLACEMENT = "<é>"


def _columns(n, variant):
    """The shared UTF-8 corpus and the all-ASCII one, as the same variant."""
    yield sc.column(n, variant, DEV)
    yield sc.make_variant(rc.ascii_corpus(n, nulls=True), variant, DEV)


def _assert_lists(out: Series, expected, src: Series):
    """A list<string> result: values, list offsets, row validity, and the
    child as raw offsets + bytes."""
    assert out.dtype == DataType.list(DataType.string())
    assert out.is_gpu() and len(out) == len(expected)
    assert out.to_pylist() == expected
    assert out.offsets.cpu().tolist() == spc.list_offsets(expected)
    valid = [True] * len(out) if out.validity is None \
        else out.validity.cpu().tolist()
    assert valid == [e is not None for e in expected]
    sc.assert_strings(out.children[0],
                      [x for e in expected if e is not None for x in e])


def _check_all(s: Series, vals, pattern):
    out = strk.regexp_count(s, pattern)
    assert out.dtype == DataType.int64() and out.is_gpu()
    assert out.to_pylist() == spc.o_count(vals, pattern)
    out = strk.regexp_extract(s, pattern)
    assert out.dtype == DataType.string() and out.is_gpu()
    sc.assert_strings(out, spc.o_extract(vals, pattern))
    _assert_lists(strk.regexp_extract_all(s, pattern),
                  spc.o_extract_all(vals, pattern), s)
    for rep in (REPLACEMENT, ""):
        out = strk.regexp_replace(s, pattern, rep)
        assert out.dtype == DataType.string() and out.is_gpu()
        sc.assert_strings(out, spc.o_replace(vals, pattern, rep))
    _assert_lists(strk.regexp_split(s, pattern),
                  spc.o_split(vals, pattern), s)


@matrix
def test_wrappers(n, variant):
    for s, vals in _columns(n, variant):
        assert s.is_gpu() and len(s) == len(vals)
        for pattern in WRAPPER_PATTERNS:
            _check_all(s, list(vals), pattern)


def test_wrapper_patterns_are_what_they_claim():
    assert [rd.compile_spans(p).needs_ascii for p in WRAPPER_PATTERNS[:4]] \
        == [False, False, True, True]
    with pytest.raises(rd.Unsupported):
        rd.compile_spans(WRAPPER_PATTERNS[4])
    vals = [v for v in rc.ascii_corpus(4099, nulls=True) if v is not None]
    for pattern in WRAPPER_PATTERNS:
        counts = set(spc.o_count(vals, pattern))
        assert 0 in counts and 1 in counts, pattern
        assert pattern == r"^a" or max(counts) >= 2, pattern


# ---------------------------------------------------------------------------
# which path ran
# ---------------------------------------------------------------------------

def test_supported_patterns_do_not_touch_the_host(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("host regex path taken")
    for name in HOST_HELPERS:
        monkeypatch.setattr(strk, name, boom)
    for variant in ("plain", "dict"):
        s, vals = sc.column(4099, variant, DEV)
        for pattern in (r"é+", r"a.*?b", r"[^a\n]b"):
            _check_all(s, list(vals), pattern)
    a, avals = sc.make_variant(rc.ascii_corpus(4099, nulls=True), "masked",
                               DEV)
    for pattern in (r"\d+", r"(?i)ab"):
        _check_all(a, list(avals), pattern)


def _spy_on_host(monkeypatch) -> list:
    calls = []
    for name in HOST_HELPERS:
        real = getattr(strk, name)

        def spy(s, pattern, *rest, _real=real, _name=name):
            calls.append((_name, pattern))
            return _real(s, pattern, *rest)
        monkeypatch.setattr(strk, name, spy)
    return calls


@pytest.mark.parametrize("pattern,ascii_column", [
    (r"\d+", False),            # ASCII-only program, column holds `é`
    (r"a*", True),              # can match the empty string
    (r"^a", True),              # anchor
    (rc.STATE_BOMB, True),      # over the state cap
])
def test_fallbacks_call_the_host_once(monkeypatch, pattern, ascii_column):
    calls = _spy_on_host(monkeypatch)
    vals = rc.ascii_corpus(257, nulls=True)
    if not ascii_column:
        vals = vals + ["é1", "é"]
    s = _column(vals)
    assert strk.regexp_count(s, pattern).to_pylist() == \
        spc.o_count(vals, pattern)
    sc.assert_strings(strk.regexp_extract(s, pattern),
                      spc.o_extract(vals, pattern))
    assert strk.regexp_extract_all(s, pattern).to_pylist() == \
        spc.o_extract_all(vals, pattern)
    sc.assert_strings(strk.regexp_replace(s, pattern, "X"),
                      spc.o_replace(vals, pattern, "X"))
    assert strk.regexp_split(s, pattern).to_pylist() == \
        spc.o_split(vals, pattern)
    assert calls == [(name, pattern) for name in HOST_HELPERS]


def test_templates_groups_and_grouped_split_call_the_host_once(monkeypatch):
    calls = _spy_on_host(monkeypatch)
    vals = rc.ascii_corpus(257, nulls=True)
    s = _column(vals)
    sc.assert_strings(strk.regexp_replace(s, r"ab", r"[\g<0>]"),
                      spc.o_replace(vals, r"ab", r"[\g<0>]"))
    out = strk.regexp_split(s, r"(a)")
    assert out.is_gpu()
    assert out.to_pylist() == spc.o_split(vals, r"(a)")
    sc.assert_strings(strk.regexp_extract(s, r"(a)b", 1),
                      spc.o_extract(vals, r"(a)b", 1))
    assert strk.regexp_extract_all(s, r"(a)b", 1).to_pylist() == \
        spc.o_extract_all(vals, r"(a)b", 1)
    assert calls == [("_host_regexp_replace", r"ab"),
                     ("_host_regexp_split", r"(a)"),
                     ("_host_regexp_extract", r"(a)b"),
                     ("_host_regexp_extract_all", r"(a)b")]
    # the same patterns without the template or the group stay on the device
    del calls[:]
    sc.assert_strings(strk.regexp_replace(s, r"ab", "[]"),
                      spc.o_replace(vals, r"ab", "[]"))
    assert strk.regexp_split(s, r"(?:a)").to_pylist() == \
        spc.o_split(vals, r"(?:a)")
    sc.assert_strings(strk.regexp_extract(s, r"(a)b", 0),
                      spc.o_extract(vals, r"(a)b", 0))
    assert calls == []


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

def test_dataframe_select():
    vals = sc.corpus(4099)

    def query(**kw):
        return daft.from_pydict({"s": vals}, **kw).select(
            fx.regexp_count(col("s"), r"a+b").alias("c"),
            col("s").str.replace(r"é+|b", "<€>", regex=True).alias("r"),
            fx.regexp_extract_all(col("s"), r"a.*?b").alias("ea"),
        ).to_pydict()
    want = query()
    assert query(device=DEV) == want
    assert want == {"c": spc.o_count(vals, r"a+b"),
                    "r": spc.o_replace(vals, r"é+|b", "<€>"),
                    "ea": spc.o_extract_all(vals, r"a.*?b")}
    assert max(c for c in want["c"] if c is not None) >= 2


def test_sql_regexp_replace():
    vals = sc.corpus(4099)
    q = "select regexp_replace(s, 'a+', 'X') as r from t"
    t = daft.from_pydict({"s": vals})
    want = daft.sql(q).to_pydict()
    t = daft.from_pydict({"s": vals}, device=DEV)   # noqa: F841
    got = daft.sql(q).to_pydict()
    assert got == want == {"r": spc.o_replace(vals, r"a+", "X")}
    assert sum(a != b for a, b in zip(want["r"], vals)) > 100

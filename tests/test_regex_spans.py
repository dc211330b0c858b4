"""Match positions (daft_amd/kernels/regex_dfa.py compile_spans) against
Python `re`: `SpanProgram.spans_host` walks the forward and reverse tables
exactly as the HIP kernels do, so every comparison here is exact and needs no
device.  Also the five kernel-layer functions on CPU Series."""
import random
import re
import time

import numpy as np
import pytest

from daft_amd import DataType, Series
from daft_amd.kernels import regex_dfa as rd
from daft_amd.kernels import strings as strk

import regex_cases as rc
import regex_span_cases as spc
import strings_cases as sc

N = 4099
CORPUS = [v for v in sc.corpus(N) if v is not None]
ASCII = rc.ascii_corpus(N)


def _rows(needs_ascii: bool) -> list:
    """Every value of the ASCII corpus, every non-null value of the shared
    one where the pattern may see it, and the extra rows."""
    return ASCII + spc.EXTRA_ROWS + ([] if needs_ascii else CORPUS)


def test_pattern_list_is_what_the_issue_asks():
    pats = [p for p, _ in spc.SPAN_SUPPORTED]
    assert len(pats) >= 25 and len(set(pats)) == len(pats)
    for p in (r"a", r"ab|b", r"a|ab", r"(a|ab)(c|bcd)", r"a+", r"a+?",
              r"a+?b", r"a{2,3}", r"a{1,2}?", r"(ab)+", r"[ab]+B", r"[^a]",
              r"[^a\n]b", r"a.b", r"(?s)a.b", r"a.*b", r"a.*?b", r"é+",
              r"[é€]a", r"😀.", r".😀", r"(?:a|é)(?P<x>b|\n)", r"\d+",
              r"\w+", r"\s+", r"(?i)ab", r"(?i)[^a-c]+"):
        assert p in pats, p
    assert all(v.isascii() for v in ASCII)
    assert any(not v.isascii() for v in CORPUS)


@pytest.mark.parametrize("pattern,needs_ascii", spc.SPAN_SUPPORTED)
def test_spans_match_re(pattern, needs_ascii):
    prog = rd.compile_spans(pattern)
    assert prog.needs_ascii is needs_ascii
    rx = re.compile(pattern)
    many = none = at_end = False
    for v in _rows(needs_ascii):
        data = v.encode()
        want = spc.byte_spans(rx, v)
        assert prog.spans_host(data) == want, (pattern, v)
        assert prog.count_host(data) == len(want), (pattern, v)
        assert prog.spans_host(data, 1) == want[:1], (pattern, v)
        assert prog.count_host(data, 1) == min(len(want), 1), (pattern, v)
        many |= len(want) >= 2
        none |= not want
        at_end |= bool(want) and want[-1][1] == len(data)
    # no answer is vacuous
    assert many and none and at_end


def test_limit_stops_early():
    prog = rd.compile_spans(r"ab")
    data = b"ab" * 5
    assert prog.spans_host(data, 3) == [(0, 2), (2, 4), (4, 6)]
    assert prog.count_host(data, 3) == 3
    assert prog.count_host(data) == 5 and prog.count_host(b"") == 0


def test_property_random_patterns():
    """Every generated pattern is refused or agrees with `re` exactly."""
    rng = random.Random(20240607)
    n_patterns, n_texts = 2000, 20
    compiled = 0
    for _ in range(n_patterns):
        pattern = spc.random_pattern(rng)
        texts = [spc.random_text(rng) for _ in range(n_texts)]
        try:
            prog = rd.compile_spans(pattern)
        except rd.Unsupported:
            continue
        compiled += 1
        rx = re.compile(pattern)
        for t in texts:
            want = spc.byte_spans(rx, t)
            data = t.encode()
            assert prog.spans_host(data) == want, (pattern, t)
            assert prog.count_host(data) == len(want), (pattern, t)
    # the condition that keeps this honest: a generator that mostly makes
    # refused patterns tests nothing
    assert compiled * 3 >= n_patterns, compiled


@pytest.mark.parametrize("pattern", spc.SPAN_UNSUPPORTED)
def test_unsupported_in_span_mode(pattern):
    re.compile(pattern)     # a valid pattern: only span mode refuses
    t0 = time.perf_counter()
    with pytest.raises(rd.Unsupported):
        rd.compile_spans(pattern)
    assert time.perf_counter() - t0 < 5.0


def test_why_empty_repeat_bodies_are_refused():
    """sre ends a repeat on an empty iteration; an automaton would give
    (0, 5), (6, 7) here."""
    rx = re.compile(spc.EMPTY_BODY)
    assert [m.span() for m in rx.finditer("bcbbc\nb")] == \
        [(0, 2), (2, 3), (3, 5), (6, 7)]
    with pytest.raises(rd.Unsupported):
        rd.compile_spans(spc.EMPTY_BODY)


def test_boolean_mode_keeps_anchors_and_empty_matches():
    for pattern in (r"^a", r"a*"):
        prog = rd.compile(pattern, "search")
        assert prog.match_host(b"ab")
        with pytest.raises(rd.Unsupported):
            rd.compile_spans(pattern)


@pytest.mark.parametrize("pattern,needs_ascii", spc.SPAN_SUPPORTED)
def test_span_table_invariants(pattern, needs_ascii):
    prog = rd.compile_spans(pattern)
    for table, flags, start in ((prog.fwd_table, prog.fwd_flags, prog.start),
                                (prog.rev_table, prog.rev_flags,
                                 prog.rev_start)):
        assert table.dtype == np.int16 and table.ndim == 2
        assert table.flags["C_CONTIGUOUS"]
        assert table.shape == (flags.shape[0], prog.n_classes)
        assert flags.dtype == np.uint8
        assert 0 <= table.min() and table.max() < table.shape[0]
        assert table.shape[0] <= rd.MAX_STATES
        assert 0 <= start < table.shape[0]
        # the pattern cannot match the empty string
        assert not flags[start] & rd.SPAN_MATCH
        for s in range(table.shape[0]):
            f = int(flags[s])
            assert f & ~(rd.SPAN_MATCH | rd.DEAD) == 0
            if f & rd.DEAD:     # absorbing, and no match from here on
                assert (flags[table[s]] == rd.DEAD).all()
    assert prog.byte_class.dtype == np.uint8
    assert prog.byte_class.shape == (256,)
    assert prog.byte_class.max() < prog.n_classes
    assert prog.nbytes == (prog.fwd_table.nbytes + prog.rev_table.nbytes +
                           256 + prog.fwd_flags.shape[0] +
                           prog.rev_flags.shape[0])
    assert prog.nbytes <= rd.MAX_TABLE_BYTES


def test_compile_spans_is_cached_and_counts_groups():
    assert rd.compile_spans(r"a.b") is rd.compile_spans(r"a.b")
    assert rd.compile_spans(r"a.b", re.DOTALL) is not rd.compile_spans(r"a.b")
    assert rd.compile_spans(r"a.b").n_groups == 0
    assert rd.compile_spans(r"(a)(?:b)(?P<x>c)").n_groups == 2
    prog = rd.compile_spans(r"a.b", re.DOTALL)
    assert prog.spans_host(b"a\nb") == [(0, 3)]


def test_span_table_bytes_cap(monkeypatch):
    monkeypatch.setattr(rd, "MAX_TABLE_BYTES", 300)
    rd._spans_cached.cache_clear()
    try:
        with pytest.raises(rd.Unsupported, match="bytes"):
            rd.compile_spans(r"[^é€😀a]+x{3}")
    finally:
        rd._spans_cached.cache_clear()      # the refusal is cached too


# ---------------------------------------------------------------------------
# the five kernel-layer functions on CPU Series
# ---------------------------------------------------------------------------

CPU_VALUES = sc.corpus(257) + rc.ascii_corpus(64, nulls=True) + \
    ["abcab", "a1b22", "", None, "bcd abcd"]
# a supported pattern, a host-only one (anchor), and one with a group
CPU_PATTERNS = [r"a+?b", r"^a", r"(a)b"]


def _series(values):
    return Series.from_pylist("s", list(values), DataType.string())


@pytest.mark.parametrize("pattern", CPU_PATTERNS)
def test_cpu_series_functions(pattern):
    s = _series(CPU_VALUES)
    out = strk.regexp_count(s, pattern)
    assert out.dtype == DataType.int64()
    assert out.to_pylist() == spc.o_count(CPU_VALUES, pattern)
    out = strk.regexp_extract(s, pattern)
    assert out.dtype == DataType.string()
    assert out.to_pylist() == spc.o_extract(CPU_VALUES, pattern)
    out = strk.regexp_extract_all(s, pattern)
    assert out.dtype == DataType.list(DataType.string())
    assert out.to_pylist() == spc.o_extract_all(CPU_VALUES, pattern)
    out = strk.regexp_replace(s, pattern, "<é>")
    assert out.dtype == DataType.string()
    assert out.to_pylist() == spc.o_replace(CPU_VALUES, pattern, "<é>")
    out = strk.regexp_split(s, pattern)
    assert out.dtype == DataType.list(DataType.string())
    assert out.to_pylist() == spc.o_split(CPU_VALUES, pattern)


def test_cpu_series_templates_groups_and_grouped_split():
    s = _series(CPU_VALUES)
    assert strk.regexp_replace(s, r"(a)(b)", r"\2\g<1>").to_pylist() == \
        spc.o_replace(CPU_VALUES, r"(a)(b)", r"\2\g<1>")
    assert strk.regexp_split(s, r"(a)b").to_pylist() == \
        spc.o_split(CPU_VALUES, r"(a)b")
    assert strk.regexp_extract(s, r"(a)(b)", 2).to_pylist() == \
        spc.o_extract(CPU_VALUES, r"(a)(b)", 2)
    assert strk.regexp_extract_all(s, r"a(b|\d)", 1).to_pylist() == \
        spc.o_extract_all(CPU_VALUES, r"a(b|\d)", 1)
    # the oracle's answers are not vacuous
    assert any(v for v in spc.o_extract_all(CPU_VALUES, r"a(b|\d)", 1) if v)
    assert any(v is not None and len(v) > 1
               for v in spc.o_split(CPU_VALUES, r"(a)b"))
    assert None in spc.o_extract(CPU_VALUES, r"(a)(b)", 2)


def test_free_functions_route_to_the_kernel_layer(monkeypatch):
    """The public free functions evaluate through kernels/strings.py."""
    import daft_amd as daft
    from daft_amd import col
    from daft_amd.functions import strings_extra as fx
    seen = []
    for name in ("_host_regexp_count", "_host_regexp_extract",
                 "_host_regexp_extract_all", "_host_regexp_replace",
                 "_host_regexp_split"):
        real = getattr(strk, name)

        def spy(*a, _real=real, _name=name):
            seen.append(_name)
            return _real(*a)
        monkeypatch.setattr(strk, name, spy)
    vals = ["abab", None, "b", ""]
    got = daft.from_pydict({"s": vals}).select(
        fx.regexp_count(col("s"), "ab").alias("c"),
        fx.regexp_extract(col("s"), "ab").alias("e"),
        fx.regexp_extract_all(col("s"), "ab").alias("ea"),
        fx.regexp_replace(col("s"), "ab", "X").alias("r"),
        fx.regexp_split(col("s"), "a").alias("sp")).to_pydict()
    assert got == {"c": spc.o_count(vals, "ab"),
                   "e": spc.o_extract(vals, "ab"),
                   "ea": spc.o_extract_all(vals, "ab"),
                   "r": spc.o_replace(vals, "ab", "X"),
                   "sp": spc.o_split(vals, "a")}
    assert sorted(seen) == ["_host_regexp_count", "_host_regexp_extract",
                            "_host_regexp_extract_all",
                            "_host_regexp_replace", "_host_regexp_split"]
    with pytest.raises(re.error):
        fx.regexp_count(col("s"), "(")

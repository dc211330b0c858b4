"""The regex -> DFA compiler (daft_amd/kernels/regex_dfa.py) against Python
`re`: `Program.match_host` walks the same tables as the HIP kernel, so
every comparison here is exact and needs no device."""
import re
import time

import numpy as np
import pytest

from daft_amd.kernels import regex_dfa as rd

import regex_cases as rc
import strings_cases as sc

CORPUS = [v for v in sc.corpus(4099) if v is not None]
ASCII = rc.ascii_corpus(600) + [v for v in CORPUS if v.isascii()]


def _rows(needs_ascii: bool) -> list:
    return ASCII if needs_ascii else ASCII + CORPUS


def test_corpora_hold_what_the_patterns_need():
    sc.corpus_guards()
    assert ASCII[:4] == ["a\n", "a\n\n", "\n", ""]
    assert all(v.isascii() for v in ASCII)
    text = "".join(ASCII)
    for ch in "0_!\t\x1cZ":
        assert ch in text
    assert sum(v.endswith("\n") for v in ASCII) > 50
    assert any(not v.isascii() for v in CORPUS)


@pytest.mark.parametrize("pattern,needs_ascii", rc.SUPPORTED)
def test_search_matches_re(pattern, needs_ascii):
    prog = rd.compile(pattern, "search")
    assert prog.needs_ascii is needs_ascii
    rx = re.compile(pattern)
    rows = _rows(prog.needs_ascii)
    want = [rx.search(v) is not None for v in rows]
    got = [prog.match_host(v.encode()) for v in rows]
    assert got == want
    # neither answer is vacuous
    assert True in want
    assert (False in want) or pattern in rc.ALWAYS_TRUE


@pytest.mark.parametrize("pattern,needs_ascii", rc.SUPPORTED)
def test_full_matches_re(pattern, needs_ascii):
    prog = rd.compile(pattern, "full")
    rx = re.compile(pattern)
    rows = _rows(prog.needs_ascii)
    assert [prog.match_host(v.encode()) for v in rows] == \
        [rx.fullmatch(v) is not None for v in rows]


def test_dollar_and_end_of_string():
    for pattern, want in ((r"a$", [True, False, False, False]),
                          (r"a\Z", [False, False, False, False]),
                          (r"^$", [False, False, True, True])):
        prog = rd.compile(pattern)
        assert [prog.match_host(v.encode()) for v in ASCII[:4]] == want
        assert rc.o_search(ASCII[:4], pattern) == want


def test_ignorecase_non_ascii_literal_on_ascii_rows():
    """`re` lets `ſ` match `s` under IGNORECASE: the program is ASCII-only
    and right on ASCII rows."""
    prog = rd.compile("(?i)ſa")
    assert prog.needs_ascii
    rows = ["sa", "Sa", "xa", "", "s"]
    assert [prog.match_host(v.encode()) for v in rows] == \
        rc.o_search(rows, "(?i)ſa") == [True, True, False, False, False]


@pytest.mark.parametrize("pattern", sc.LIKE_PATTERNS + rc.LIKE_EXTRA)
def test_like_program(pattern):
    prog = rd.like_program(pattern, False)
    assert prog.needs_ascii is False
    rows = ASCII + CORPUS
    assert [prog.match_host(v.encode()) for v in rows] == \
        sc.o_like(rows, pattern)
    prog = rd.like_program(pattern.upper(), True)
    assert prog.needs_ascii is True
    assert [prog.match_host(v.encode()) for v in ASCII] == \
        sc.o_like(ASCII, pattern.upper(), ci=True)
    prog = rd.like_program(pattern, True)
    assert [prog.match_host(v.encode()) for v in ASCII] == \
        sc.o_like(ASCII, pattern, ci=True)


def test_like_underscore_is_one_code_point():
    prog = rd.like_program("_")
    rows = ["", "a", "\n", "é", "€", "😀", "ab", "éa", "😀😀"]
    assert [prog.match_host(v.encode()) for v in rows] == \
        sc.o_like(rows, "_") == [False] + [True] * 5 + [False] * 3


@pytest.mark.parametrize("pattern", rc.UNSUPPORTED)
def test_unsupported(pattern):
    re.compile(pattern)     # a valid pattern: only the DFA engine refuses
    t0 = time.perf_counter()
    with pytest.raises(rd.Unsupported):
        rd.compile(pattern, "search")
    assert time.perf_counter() - t0 < 5.0


def test_state_cap_stops_construction_early():
    rd._compile_cached.cache_clear()
    t0 = time.perf_counter()
    with pytest.raises(rd.Unsupported, match="DFA states"):
        rd.compile(rc.STATE_BOMB)
    assert time.perf_counter() - t0 < 5.0
    assert rd.MAX_STATES < 2 ** 13


def test_table_bytes_cap(monkeypatch):
    assert rd.MAX_TABLE_BYTES <= 64 * 1024
    monkeypatch.setattr(rd, "MAX_TABLE_BYTES", 300)
    rd._compile_cached.cache_clear()
    try:
        with pytest.raises(rd.Unsupported, match="bytes"):
            rd.compile(r"[^é€😀a]+x{3}$")
    finally:
        rd._compile_cached.cache_clear()    # the refusal is cached too


@pytest.mark.parametrize("pattern,needs_ascii", rc.SUPPORTED)
@pytest.mark.parametrize("mode", ["search", "full"])
def test_table_invariants(pattern, needs_ascii, mode):
    prog = rd.compile(pattern, mode)
    assert prog.table.dtype == np.int16 and prog.table.ndim == 2
    assert prog.byte_class.dtype == np.uint8
    assert prog.byte_class.shape == (256,)
    assert prog.flags.dtype == np.uint8
    assert prog.flags.shape == (prog.n_states,)
    assert prog.table.flags["C_CONTIGUOUS"]
    assert 0 <= prog.table.min() and prog.table.max() < prog.n_states
    assert prog.byte_class.max() < prog.n_classes
    assert 0 <= prog.start < prog.n_states
    assert prog.n_states <= rd.MAX_STATES
    assert prog.nbytes == prog.table.nbytes + 256 + prog.n_states
    assert prog.nbytes <= rd.MAX_TABLE_BYTES
    # matched and dead states are absorbing, and never both
    for s in range(prog.n_states):
        f = int(prog.flags[s])
        assert f & ~(rd.MATCHED | rd.END | rd.DEAD) == 0
        if f & rd.MATCHED:
            assert f & rd.END and not f & rd.DEAD
            assert (prog.flags[prog.table[s]] & rd.MATCHED).all()
        if f & rd.DEAD:
            assert not f & rd.END
            assert (prog.flags[prog.table[s]] & rd.DEAD).all()


def test_compile_is_cached():
    assert rd.compile(r"a.b", "search") is rd.compile(r"a.b", "search")
    assert rd.compile(r"a.b", "search") is not rd.compile(r"a.b", "full")
    assert rd.compile(r"a.b", "search", re.DOTALL) is not \
        rd.compile(r"a.b", "search")
    assert rd.like_program("a_", True) is rd.like_program("a_", True)
    with pytest.raises(ValueError):
        rd.compile("a", "prefix")


def test_flags_argument_matches_inline_flags():
    rows = ["a\nb", "axb", "AXB", "ab"]
    for flags, inline in ((re.DOTALL, "(?s)"), (re.IGNORECASE, "(?i)")):
        prog = rd.compile(r"a.b", "search", flags)
        assert [prog.match_host(v.encode()) for v in rows] == \
            rc.o_search(rows, inline + r"a.b")
    with pytest.raises(rd.Unsupported):
        rd.compile(r"^a", "search", re.MULTILINE)

"""CPU path of daft_amd/kernels/strings.py and of the string branch of
rowops.argsort_multi against the Python oracle in strings_cases.py, over
every size and column variant.  This proves the corpus and the oracle
without a GPU and pins the CPU path that test_gpu_strings.py mirrors."""
import pytest

import daft_amd as daft
from daft_amd.sql import sql

import strings_cases as sc

DEV = "cpu"
MATRIX = [(n, v) for n in sc.SIZES for v in sc.VARIANTS]
matrix = pytest.mark.parametrize("n,variant", MATRIX)


def test_corpus_guards():
    sc.corpus_guards()


def test_corpus_is_deterministic_and_variants_hold_the_values():
    assert sc.corpus(257) == sc.corpus(257)
    assert sc.corpus(257, seed=1) != sc.corpus(257)
    for n in sc.SIZES:
        for variant in sc.VARIANTS:
            s, vals = sc.column(n, variant, DEV)
            assert s.to_pylist() == list(vals)
    s, _ = sc.column(257, "slice", DEV)
    assert s.data.storage_offset() > 0
    s, _ = sc.column(257, "dict", DEV)
    assert s.is_dict() and s.validity is not None
    s, vals = sc.column(257, "masked", DEV)
    lens = (s.offsets[1:] - s.offsets[:-1])[~s.validity]
    assert int((lens > 0).sum()) > 10


@matrix
def test_find_family(n, variant):
    sc.check_find_family(n, variant, DEV)


@matrix
def test_like(n, variant):
    sc.check_like(n, variant, DEV)


@pytest.mark.parametrize("value,pattern,ci,want", [
    ("a\nb", "_%", False, True),      # `_` and `%` match a newline
    ("a\nb", "a_b", False, True),
    ("a\n", "a", True, False),        # no match before a trailing newline
    ("a\n", "a_", True, True),
    ("A\n", "a%", True, True),
])
def test_like_newlines(value, pattern, ci, want):
    s = daft.Series.from_pylist("s", [value])
    from daft_amd.kernels import strings as strk
    assert strk.like(s, pattern, case_insensitive=ci).to_pylist() == [want]
    assert sc.o_like([value], pattern, ci) == [want]


@matrix
def test_lengths(n, variant):
    sc.check_lengths(n, variant, DEV)


@matrix
def test_substr_left(n, variant):
    sc.check_substr(n, variant, DEV)


def test_substr_binary_counts_bytes():
    sc.check_substr_binary(DEV)


def test_substr_rejects_negative():
    sc.check_substr_rejects_negative(DEV)


@matrix
def test_lower_upper(n, variant):
    sc.check_case(n, variant, DEV)


def test_lower_upper_ascii():
    sc.check_case_ascii(257, DEV)


@matrix
def test_concat(n, variant):
    sc.check_concat(n, variant, DEV)


@matrix
def test_compare(n, variant):
    sc.check_compare(n, variant, DEV)


@matrix
def test_if_else(n, variant):
    sc.check_if_else(n, variant, DEV)


@matrix
def test_sort(n, variant):
    sc.check_sort(n, variant, DEV)


def test_sort_long_shared_chunks():
    sc.check_sort_long(DEV)


def test_sort_nul_tail():
    sc.check_sort_nul_tail(DEV)


@pytest.mark.parametrize("expr,want", [
    ("substring(x, 0, 2)", ["h", "h"]),
    ("substring(x, -1, 3)", ["h", "h"]),
    ("substring(x, 0)", ["hello", "héllo"]),
    ("substring(x, 2, 2)", ["el", "él"]),
    ("substring(x from 0 for 2)", ["h", "h"]),
    ("substring(x from 2 for 2)", ["el", "él"]),
    ("substring(x, -5, 2)", ["", ""]),
    ("substring(x, 1)", ["hello", "héllo"]),
])
def test_sql_substring(expr, want):
    df = daft.from_pydict({"x": ["hello", "héllo"]})  # noqa: F841
    assert sql(f"select {expr} as y from df").to_pydict() == {"y": want}

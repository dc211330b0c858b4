"""Public surface of boolean regex matching: the free function
`daft_amd.functions.regexp_match` and SQL `regexp_match(col, 'pat')`."""
import pytest

import daft_amd as daft
import daft_amd.functions as F
from daft_amd import col
from daft_amd.kernels import strings as strk
from daft_amd.sql.planner import SQLPlanError

import regex_cases as rc

VALUES = ["axb", "ab", None, "a\nb", "xxa€b", "", "A.B"]


def _frame():
    return daft.from_pydict({"s": VALUES, "p": ["a.b"] * len(VALUES)})


def test_free_function_equals_str_match():
    df = _frame()
    got = df.select(F.regexp_match(col("s"), r"a.b").alias("m")).to_pydict()
    via_ns = df.select(col("s").str.match(r"a.b").alias("m")).to_pydict()
    assert got == via_ns == {"m": rc.o_search(VALUES, r"a.b")}
    assert got["m"] == [True, False, None, False, True, False, False]
    assert F.regexp_match is not F.regexp


def test_free_function_rejects_non_string_pattern():
    with pytest.raises(TypeError):
        F.regexp_match(col("s"), col("p"))


def test_sql_regexp_match():
    t = _frame()    # noqa: F841 - looked up by name from the query
    got = daft.sql("select regexp_match(s, 'a.b') as m from t").to_pydict()
    assert got == {"m": rc.o_search(VALUES, r"a.b")}
    got = daft.sql(
        "select s from t where regexp_match(s, '^a|B$')").to_pydict()
    assert got == {"s": ["axb", "ab", "a\nb", "A.B"]}


@pytest.mark.parametrize("call", ["regexp_match(s, p)", "regexp_match(s, 3)",
                                  "regexp_match(s)"])
def test_sql_regexp_match_needs_a_literal_pattern(call):
    t = _frame()    # noqa: F841
    with pytest.raises(SQLPlanError):
        daft.sql(f"select {call} as m from t").to_pydict()


def test_cpu_columns_stay_on_re(monkeypatch):
    """A CPU column never reaches the DFA path: every predicate goes
    through `_host_regex_pred`."""
    calls = []
    real = strk._host_regex_pred

    def spy(s, rx, full):
        calls.append((rx.pattern, full))
        return real(s, rx, full)
    monkeypatch.setattr(strk, "_host_regex_pred", spy)
    s = daft.Series.from_pylist("s", VALUES, daft.DataType.string())
    assert strk.regexp_match(s, r"a.b").to_pylist() == \
        rc.o_search(VALUES, r"a.b")
    assert strk.like(s, "a_b").to_pylist() == \
        [True, False, None, True, False, False, False]
    assert strk.like(s, "a.b", case_insensitive=True).to_pylist() == \
        [False, False, None, False, False, False, True]
    assert [full for _, full in calls] == [False, True, True]

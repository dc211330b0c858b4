"""As-of join on the CPU path against the brute-force oracle in
asof_cases.py: asof_match over the case grid for every strategy, the null
rules, string `by` keys, the DataFrame interface and its errors, and the
number of host syncs, which must not grow with the number of groups."""
import numpy as np
import pytest
import torch

import daft_amd as daft
from daft_amd import DataType, Series
from daft_amd.logical.plan import AsofJoin
from daft_amd.physical.asof import asof_match

import asof_cases as ac


# ---------------------------------------------------------------------------
# the oracle itself
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(ac.HAND)))
def test_oracle_hand_cases(i):
    lk, lg, rk, rg, strategy, allow_exact, want = ac.HAND[i]
    got = ac.oracle(lk, [True] * len(lk), lg, rk, [True] * len(rk), rg,
                    strategy, allow_exact)
    assert got == want


def test_oracle_nulls():
    # null on-keys on either side, and null by keys (None), never match
    got = ac.oracle([10, 10, 10], [True, False, True], [0, 0, None],
                    [9, 10, 8], [True, False, True], [0, 0, None],
                    "backward")
    assert got == [0, -1, -1]


@pytest.mark.parametrize("i", range(len(ac.HAND)))
def test_match_hand_cases(i):
    lk, lg, rk, rg, strategy, allow_exact, want = ac.HAND[i]
    dt = "float64" if isinstance(lk[0], float) else "int64"
    got = asof_match(
        ac.key_series("t", dt, lk, [True] * len(lk)),
        ac.key_series("t", dt, rk, [True] * len(rk)),
        [ac.gid_series("g", lg)], [ac.gid_series("g", rg)],
        strategy, allow_exact)
    assert got.tolist() == want


# ---------------------------------------------------------------------------
# asof_match over the grid
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ac.grid(), ids=ac.case_ids())
def test_match_equals_oracle(case):
    lk, rk, lb, rb = ac.case_series(case)
    for strategy, allow_exact in ac.VARIANTS:
        got = asof_match(lk, rk, lb, rb, strategy, allow_exact)
        assert got.dtype == torch.int64 and got.shape == (len(lk),)
        assert tuple(got.tolist()) == ac.expected(case, strategy,
                                                  allow_exact), \
            (strategy, allow_exact)


def test_match_big_case():
    case = ac.big_case()
    lk, rk, lb, rb = ac.case_series(case)
    for strategy, allow_exact in ac.VARIANTS:
        got = asof_match(lk, rk, lb, rb, strategy, allow_exact)
        assert tuple(got.tolist()) == ac.expected(case, strategy,
                                                  allow_exact)


def _sym(name, gids):
    return Series.from_pylist(
        name, [None if g is None else f"sym-{g:03d}" for g in gids])


@pytest.mark.parametrize("two_columns", [False, True])
def test_match_string_by(two_columns):
    # gid g becomes the string "sym-g" (and, with two columns, the pair
    # (string of g // 3, int g % 3)): the same grouping under another type
    case = ac._make("string-by", 77, 65, 64, 7, "heavy_dups")
    lk, rk, _, _ = ac.case_series(case)
    if two_columns:
        split = lambda gs: ([None if g is None else g // 3 for g in gs],
                            [None if g is None else g % 3 for g in gs])
        (la, lb2), (ra, rb2) = split(case.left_gid), split(case.right_gid)
        lby = [_sym("a", la), ac.gid_series("b", lb2)]
        rby = [_sym("a", ra), ac.gid_series("b", rb2)]
    else:
        lby, rby = [_sym("a", case.left_gid)], [_sym("a", case.right_gid)]
    for strategy, allow_exact in ac.VARIANTS:
        got = asof_match(lk, rk, lby, rby, strategy, allow_exact)
        assert tuple(got.tolist()) == ac.expected(case, strategy,
                                                  allow_exact)


# ---------------------------------------------------------------------------
# nulls
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", ac.STRATEGIES)
def test_null_left_on_key_matches_nothing(strategy):
    # the data slot under the null holds a key that would match
    lk = ac.key_series("t", "int64", [10, 10], [True, False])
    rk = ac.key_series("t", "int64", [10], [True])
    assert asof_match(lk, rk, [], [], strategy).tolist() == [0, -1]


@pytest.mark.parametrize("strategy", ac.STRATEGIES)
def test_null_right_on_key_is_never_chosen(strategy):
    # the null row's slot holds the exact key; the valid rows are farther
    lk = ac.key_series("t", "int64", [10], [True])
    rk = ac.key_series("t", "int64", [7, 10, 13], [True, False, True])
    want = {"backward": [0], "forward": [2], "nearest": [2]}[strategy]
    assert asof_match(lk, rk, [], [], strategy).tolist() == want
    rk = ac.key_series("t", "int64", [10, 10], [False, False])
    assert asof_match(lk, rk, [], [], strategy).tolist() == [-1]


@pytest.mark.parametrize("strategy", ac.STRATEGIES)
def test_null_by_matches_nothing(strategy):
    lk = ac.key_series("t", "int64", [10, 10, 10], [True] * 3)
    rk = ac.key_series("t", "int64", [10, 10], [True] * 2)
    # left: group 0, null, group 1; right: null, group 1
    for mk in (ac.gid_series,
               lambda n, g: _sym(n, g)):
        lb, rb = mk("g", [0, None, 1]), mk("g", [None, 1])
        assert asof_match(lk, rk, [lb], [rb], strategy).tolist() == \
            [-1, -1, 1]


def test_unknown_strategy_and_inexact_nearest():
    k = ac.key_series("t", "int64", [1], [True])
    with pytest.raises(ValueError):
        asof_match(k, k, [], [], "sideways")
    with pytest.raises(ValueError):
        asof_match(k, k, [], [], "nearest", allow_exact=False)


# ---------------------------------------------------------------------------
# host syncs
# ---------------------------------------------------------------------------

def test_host_reads_do_not_grow_with_groups(monkeypatch):
    counts = {"item": 0, "tolist": 0}
    for name in counts:
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)

    def run(groups):
        c = ac._make("sync", 5, 257, 1000, groups, nulls=False)
        lk, rk, lb, rb = ac.case_series(c)
        before = dict(counts)
        out = asof_match(lk, rk, lb, rb, "backward")
        used = {k: counts[k] - before[k] for k in counts}
        assert (out >= 0).any()
        return used
    assert run(2) == run(200)


# ---------------------------------------------------------------------------
# DataFrame interface
# ---------------------------------------------------------------------------

def _doc_frames(device="cpu"):
    left = daft.from_pydict({"entity": ["A", "A", "B"],
                             "timestamp": [10, 11, 10]}, device=device)
    right = daft.from_pydict({"entity": ["A", "A", "A", "B", "B"],
                              "timestamp": [9, 10, 11, 9, 11],
                              "value": [1.0, 2.0, 3.0, 5.0, 6.0]},
                             device=device)
    return left, right


def test_df_on_and_by_as_strings():
    left, right = _doc_frames()
    out = left.join_asof(right, on="timestamp", by="entity") \
        .sort(["entity", "timestamp"]).to_pydict()
    assert out == {"entity": ["A", "A", "B"], "timestamp": [10, 11, 10],
                   "value": [2.0, 3.0, 5.0]}


def test_df_left_by_right_by_and_positional():
    left, right = _doc_frames()
    right = right.select(daft.col("entity").alias("e2"),
                         daft.col("timestamp").alias("t2"),
                         daft.col("value"))
    out = left.join_asof(right, "timestamp", "t2", left_by="entity",
                         right_by=["e2"], strategy="forward") \
        .sort(["entity", "timestamp"]).to_pydict()
    assert out["value"] == [2.0, 3.0, 6.0]
    assert out["t2"] == [10, 11, 11]


def test_df_nearest_and_unmatched_nulls():
    left = daft.from_pydict({"k": ["a", "a", "b", "c"],
                             "t": [10, 3, 10, 10]})
    right = daft.from_pydict({"k": ["a", "a", "b", "b"],
                              "t": [8, 12, 1, 100],
                              "v": [1, 2, 3, 4]})
    out = left.join_asof(right, on="t", by="k", strategy="nearest") \
        .to_pydict()
    assert out == {"k": ["a", "a", "b", "c"], "t": [10, 3, 10, 10],
                   "v": [2, 1, 3, None]}


def test_df_prefix_suffix_naming():
    left = daft.from_pydict({"t": [1, 5], "v": [10, 20]})
    right = daft.from_pydict({"t": [0, 4], "v": [7, 8], "w": [1, 2]})
    names = lambda **kw: left.join_asof(right, on="t", **kw).column_names()
    assert names() == ["t", "v", "v_right", "w"]
    assert names(suffix="_r") == ["t", "v", "v_r", "w"]
    assert names(prefix="r.") == ["t", "v", "r.v_right", "w"]
    assert names(prefix="r.", suffix="") == ["t", "v", "r.v", "w"]
    out = left.join_asof(right, on="t", prefix="r.", suffix="").to_pydict()
    assert out["r.v"] == [7, 8] and out["v"] == [10, 20]


@pytest.mark.parametrize("kwargs", [
    dict(on="t", left_on="t"),
    dict(on="t", right_on="t"),
    dict(),
    dict(left_on="t"),
    dict(right_on="t"),
    dict(on="t", by="k", left_by="k"),
    dict(on="t", by="k", right_by="k"),
    dict(on="t", left_by="k"),
    dict(on="t", right_by="k"),
    dict(on="t", left_by=["k", "t"], right_by=["k"]),
    dict(on="t", strategy="sideways"),
    dict(on="t", strategy="Backward"),
    dict(on="k"),                     # a string on-key
])
def test_df_misuse_raises_value_error(kwargs):
    left = daft.from_pydict({"k": ["a"], "t": [1]})
    right = daft.from_pydict({"k": ["a"], "t": [1], "v": [2]})
    with pytest.raises(ValueError):
        left.join_asof(right, **kwargs)


def test_plan_node_checks_strategy_and_carries_prefix():
    left = daft.from_pydict({"t": [1], "v": [1]})
    right = daft.from_pydict({"t": [1], "v": [2]})
    lp, rp = left._builder.plan, right._builder.plan
    with pytest.raises(ValueError):
        AsofJoin(lp, rp, "t", "t", [], [], "sideways")
    node = AsofJoin(lp, rp, "t", "t", [], [], "nearest", "_s", "p.")
    again = node.with_children([lp, rp])
    assert (again.prefix, again.suffix, again.strategy) == \
        ("p.", "_s", "nearest")
    assert again.schema.names() == ["t", "v", "p.v_s"]


def test_df_float_keys_nan_and_negative_zero():
    nan, inf = float("nan"), float("inf")
    left = daft.from_pydict({"t": [nan, -0.0, inf]})
    right = daft.from_pydict({"t2": [0.0, inf, nan], "v": [1, 2, 3]})
    out = left.join_asof(right, left_on="t", right_on="t2").to_pydict()
    assert out["v"] == [3, 1, 2]
    out = left.join_asof(right, left_on="t", right_on="t2",
                         strategy="forward").to_pydict()
    assert out["v"] == [3, 1, 2]

"""Host-only planning of the fused Filter -> Aggregate pass: which shapes
it accepts, and that its kernel text is stable."""
import datetime as dt

import pytest
import torch

from daft_amd import DataType, Series, col
from daft_amd.kernels import fused, load_native
from daft_amd.physical.agg import decompose_agg_exprs
from daft_amd.recordbatch import RecordBatch

N = 100


def _dict(name, words, codes):
    vocab = Series.from_pylist(name, words, DataType.string())
    return Series.make_dict(name, vocab, codes.to(torch.int32))


def _lineitem():
    g = torch.Generator().manual_seed(7)

    def f64():
        return torch.rand(N, generator=g, dtype=torch.float64)
    return RecordBatch([
        Series("l_quantity", DataType.float64(), data=f64() * 50),
        Series("l_extendedprice", DataType.float64(), data=f64() * 1e5),
        Series("l_discount", DataType.float64(), data=f64() * 0.1),
        Series("l_tax", DataType.float64(), data=f64() * 0.08),
        Series("l_shipdate", DataType.date(),
               data=torch.randint(8000, 10500, (N,), generator=g,
                                  dtype=torch.int32)),
        _dict("l_returnflag", ["R", "A", "N"],
              torch.randint(0, 3, (N,), generator=g)),
        _dict("l_linestatus", ["F", "O"],
              torch.randint(0, 2, (N,), generator=g)),
        Series("l_orderkey", DataType.int64(),
               data=torch.arange(N, dtype=torch.int64)),
        Series("l_null_flag", DataType.bool(),
               data=torch.zeros(N, dtype=torch.bool),
               validity=torch.rand(N, generator=g) > 0.5),
        Series.from_pylist("l_comment", ["c%d" % (i % 3) for i in range(N)],
                           DataType.string()),
    ], num_rows=N)


def _plan(batch, pred, keys, aggs):
    named, _ = decompose_agg_exprs([a._node for a in aggs])
    return fused.plan_scan_agg(batch, None if pred is None else pred._node,
                               [col(k)._node for k in keys], named)


DISC_PRICE = col("l_extendedprice") * (1 - col("l_discount"))
Q1_PRED = col("l_shipdate") <= dt.date(1998, 9, 2)
Q1_KEYS = ["l_returnflag", "l_linestatus"]
Q1_AGGS = [col("l_quantity").sum().alias("sum_qty"),
           col("l_extendedprice").sum().alias("sum_base_price"),
           DISC_PRICE.sum().alias("sum_disc_price"),
           (DISC_PRICE * (1 + col("l_tax"))).sum().alias("sum_charge"),
           col("l_quantity").mean().alias("avg_qty"),
           col("l_extendedprice").mean().alias("avg_price"),
           col("l_discount").mean().alias("avg_disc"),
           col("l_quantity").count().alias("count_order")]
Q6_PRED = ((col("l_shipdate") >= dt.date(1994, 1, 1)) &
           (col("l_shipdate") < dt.date(1995, 1, 1)) &
           (col("l_discount") >= 0.05) & (col("l_discount") <= 0.07) &
           (col("l_quantity") < 24))
Q6_AGGS = [(col("l_extendedprice") * col("l_discount")).sum()
           .alias("revenue")]


def test_accepts_q1_and_q6_shapes():
    batch = _lineitem()
    q1 = _plan(batch, Q1_PRED, Q1_KEYS, Q1_AGGS)
    assert q1 is not None and q1.groups == 6 and q1.cards == [3, 2]
    # five distinct sums; the means read them and the count is the hits
    assert q1.ops == [0] * 5 and q1.own_valid == [0] * 5
    assert q1.agg_acc == [0, 1, 2, 3, 0, 1, 4, None]
    q6 = _plan(batch, Q6_PRED, [], Q6_AGGS)
    assert q6 is not None and q6.groups == 1 and q6.ops == [0]


def test_shared_input_is_loaded_once():
    body = _plan(_lineitem(), Q1_PRED, Q1_KEYS, Q1_AGGS).body
    # seven columns, one load each: quantity feeds sum, mean and count
    assert body.count("[i]") == 7, body


def test_same_plan_same_text():
    batch = _lineitem()
    a = _plan(batch, Q1_PRED, Q1_KEYS, Q1_AGGS)
    b = _plan(_lineitem(), Q1_PRED, Q1_KEYS, Q1_AGGS)
    assert a.body == b.body and a.ops == b.ops
    if load_native() is not None:
        assert a.source() == b.source()
        assert "#define FA_G 6" in a.source()


@pytest.mark.parametrize("pred,keys,aggs", [
    (None, ["l_orderkey"], [col("l_quantity").sum()]),       # integer key
    (None, ["l_shipdate"], [col("l_quantity").sum()]),       # date key
    (None, ["l_comment"], [col("l_quantity").sum()]),        # plain string
    (None, ["l_null_flag"], [col("l_quantity").sum()]),      # key validity
    (None, [], [col("l_orderkey").sum()]),                   # integer sum
    (None, [], [col("l_quantity").stddev()]),                # other kind
    (None, [], [col("l_quantity").count("all")]),            # reads nothing
    (col("l_comment") == "c1", [], [col("l_quantity").sum()]),  # no lowering
    (None, Q1_KEYS, [(col("l_quantity") * float(i)).sum().alias("a%d" % i)
                     for i in range(342)]),                  # 6 x 342 slots
])
def test_ineligible_shapes(pred, keys, aggs):
    assert _plan(_lineitem(), pred, keys, aggs) is None


def test_slot_count_counts_named_aggregates():
    batch = _lineitem()
    # 6 groups x 341 distinct aggregates = 2046 slots, but more than the
    # 16 accumulators the unrolled skeleton takes
    many = [(col("l_quantity") * float(i)).sum().alias("a%d" % i)
            for i in range(341)]
    assert _plan(batch, None, Q1_KEYS, many) is None
    assert _plan(batch, None, Q1_KEYS, many[:16]) is not None


def test_empty_batch_is_not_planned():
    assert _plan(_lineitem().slice(0, 0), Q1_PRED, Q1_KEYS, Q1_AGGS) is None


def test_switches(monkeypatch):
    assert fused.scan_agg_enabled()
    for name in ("DAFT_AMD_DISABLE_FUSED", "DAFT_AMD_DISABLE_JIT",
                 "DAFT_AMD_DISABLE_FUSED_AGG"):
        monkeypatch.setenv(name, "1")
        assert not fused.scan_agg_enabled()
        monkeypatch.delenv(name)

"""Fused expression kernels on the GPU against the exact Python oracle of
expr_cases.py: every case list through the hipRTC kernel, through the
postfix interpreter and through evaluate_with_cse, on every row, with a
spy telling which kernel produced the result."""
import datetime
import functools
import random

import pytest
import torch

import expr_cases as ec
from daft_amd import DataType, Series, col, lit
from daft_amd.expressions.expressions import resolve_exprs
from daft_amd.kernels import fused, native_required
from daft_amd.physical.cse import evaluate_with_cse
from daft_amd.recordbatch import RecordBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = list(ec.case_lists())
CORPORA = [(n, c) for n in ec.SIZES for c in ec.cycles(n)]
BIG_N = 2048 * 1024 + 1025      # past the capped grid: grid-stride regime


@functools.lru_cache(maxsize=4)
def _dev_batch(n, cycle):
    return ec.corpus(n, cycle).batch.to(DEV)


class _Spy:
    """Counts calls into the two kernel bindings and keeps what they
    raised."""

    def __init__(self, monkeypatch):
        native = native_required()
        self.calls = {"fused_eval_jit": 0, "fused_eval": 0}
        self.outputs = {"fused_eval_jit": 0, "fused_eval": 0}
        self.errors = []
        for name in self.calls:
            monkeypatch.setattr(native, name,
                                self._wrap(name, getattr(native, name)))

    def _wrap(self, name, real):
        def call(*a):
            self.calls[name] += 1
            try:
                out = real(*a)
            except Exception as e:
                self.errors.append((name, e))
                raise
            self.outputs[name] += len(out) // 2
            return out
        return call


def _run(route, nodes, batch, monkeypatch):
    """Evaluate one list through a route; assert which kernel ran."""
    if route == "interp":
        monkeypatch.setenv("DAFT_AMD_DISABLE_JIT", "1")
    spy = _Spy(monkeypatch)
    fn = {"jit": fused.try_fuse_jit, "interp": fused.try_fuse,
          "cse": evaluate_with_cse}[route]
    out = fn(nodes, batch)
    assert out is not None, f"{route}: nothing fused"
    assert not spy.errors, spy.errors
    ran, idle = ("fused_eval", "fused_eval_jit") if route == "interp" \
        else ("fused_eval_jit", "fused_eval")
    assert spy.calls[ran] == 1 and spy.calls[idle] == 0, (route, spy.calls)
    return out, spy.outputs[ran]


@pytest.mark.parametrize("route", ["jit", "interp", "cse"])
@pytest.mark.parametrize("n,cycle", CORPORA)
def test_fused_matches_oracle(n, cycle, route, monkeypatch):
    """Every list, every case, every row: a fused result equals the
    oracle, and so does the per-node result of what is not fused."""
    batch = _dev_batch(n, cycle)
    for family in FAMILIES:
        cases = ec.case_lists()[family]
        out, n_fused = _run(route, ec.nodes(cases), batch, monkeypatch)
        if route != "interp":
            # the planner's promise: these cases stay on the fused path
            assert n_fused == sum(c.fused for c in cases), family
        want = ec.expected(family, n, cycle)
        for case, got, w in zip(cases, out, want):
            ec.check(case, got, w, f"{route} n={n} cycle={cycle} {family}")


@pytest.mark.parametrize("route", ["jit", "interp"])
def test_grid_stride_regime(route, monkeypatch):
    """Above kMaxBlocks blocks both kernels loop; the last tile is
    partial.  Compared on the device with a torch-computed expectation."""
    g = torch.Generator().manual_seed(3)
    i = torch.randint(-(1 << 31), 1 << 31, (BIG_N,), generator=g,
                      dtype=torch.int64).to(torch.int32)
    valid = torch.rand(BIG_N, generator=g) > 0.1
    i[-5:] = torch.tensor([2**31 - 1, -2**31, 0, 715827880, 715827881],
                          dtype=torch.int32)
    valid[-2:] = torch.tensor([True, False])
    batch = RecordBatch([Series("i", DataType.int32(), data=i,
                                validity=valid)]).to(DEV)
    c = 2147483647
    (node,) = resolve_exprs([col("i") * 3 + 7 > c])
    (out,), n_fused = _run(route, [node], batch, monkeypatch)
    assert n_fused == 1
    want = (i.to(DEV).to(torch.int64) * 3 + 7) > c
    assert out.dtype == DataType.bool()
    assert torch.equal(out.validity, valid.to(DEV))
    assert torch.equal(out.data[out.validity], want[out.validity])
    assert want[out.validity].any() and not want[out.validity].all()


def test_zero_rows_through_the_bindings():
    """try_fuse never launches on an empty batch; the bindings themselves
    must still return empty, typed outputs without launching."""
    native = native_required()
    batch = ec.corpus(257).batch.to(DEV)
    empty = RecordBatch([Series(s.name, s.dtype, data=s.data[:0],
                                validity=None if s.validity is None
                                else s.validity[:0])
                         for s in batch.columns if s.data is not None], 0)
    nodes = resolve_exprs([col("i32") * 3 + 7, col("i16_n") > col("i8"),
                           col("f32") * col("f32_n")])
    want = [torch.int64, torch.bool, torch.float32]
    jp = fused.plan_jit(nodes, empty)
    m = jp.out_meta
    flat = native.fused_eval_jit(
        jp.src, [s.data for s in jp.cols], [s.validity for s in jp.cols],
        [x[3] for x in m], [1 if x[4] else 0 for x in m], 0)
    ip = fused.plan_interp(nodes, empty)
    flat2 = native.fused_eval(
        ip.prog, ip.lits, [s.data for s in ip.cols],
        [s.validity for s in ip.cols], ip.codes, ip.scales,
        [x[3] for x in ip.out_meta], [1.0] * 3,
        [1 if x[4] else 0 for x in ip.out_meta], 0)
    for f in (flat, flat2):
        assert [t.dtype for t in f[0::2]] == want
        assert all(t.numel() == 0 and t.is_cuda for t in f[0::2])
        # a validity buffer exactly where an input is nullable
        assert [None if t is None else t.numel() for t in f[1::2]] == \
            [None, 0, 0]
    assert fused.try_fuse(nodes, empty) is None


def _tpch_like(n=1000):
    rng = random.Random(7)
    d0 = datetime.date(1992, 1, 1)
    return RecordBatch.from_pydict({
        "a": [rng.uniform(-100, 100) for _ in range(n)],
        "b": [rng.uniform(0.1, 10) if i % 7 else None for i in range(n)],
        "i": [rng.randint(-1000, 1000) for _ in range(n)],
        "j": [rng.randint(0, 5) if i % 11 else None for i in range(n)],
        "d": [d0 + datetime.timedelta(days=rng.randint(0, 2500))
              for _ in range(n)],
        "f": [bool(i % 3) for i in range(n)],
        "l_quantity": [float(rng.randint(1, 50)) for _ in range(n)],
        "l_extendedprice": [rng.uniform(900, 100000) for _ in range(n)],
        "l_discount": [rng.randint(0, 10) / 100 for _ in range(n)],
        "l_tax": [rng.randint(0, 8) / 100 for _ in range(n)],
        "l_shipdate": [d0 + datetime.timedelta(days=rng.randint(0, 2500))
                       for _ in range(n)],
    }).to(DEV)


def test_benchmark_shaped_lists_stay_fused(monkeypatch):
    """The list of test_fused_expr_eval_matches_unfused and the q1- and
    q6-shaped lists fuse every expression they always did: a fix that
    merely bails would move the benchmark off the fused path."""
    date = datetime.date
    disc_price = col("l_extendedprice") * (1 - col("l_discount"))
    lists = {
        "existing": ([
            col("a") * (lit(1) - col("b")),
            col("a") + col("b") * 2.5 - col("i"),
            (col("a") > lit(0)) & (col("b") <= lit(5.0)),
            col("i") >= lit(0),
            col("b").is_null(),
            col("b").fill_null(lit(-1.0)),
            col("f").if_else(col("a"), col("b")),
            col("j").is_in([1, 3, 5]),
            col("d") >= lit(date(1994, 1, 1)),
            (col("a") > 0) | (col("b") > 1),
            col("i") * 3 + 7], 11),
        # q1: aggregation inputs; bare columns are passed through
        "q1": ([col("l_quantity"), col("l_extendedprice"), disc_price,
                disc_price * (1 + col("l_tax")), col("l_discount")], 2),
        "q6": ([(col("l_shipdate") >= lit(date(1994, 1, 1))) &
                (col("l_shipdate") < lit(date(1995, 1, 1))) &
                (col("l_discount") >= 0.05) & (col("l_discount") <= 0.07) &
                (col("l_quantity") < 24),
                col("l_extendedprice") * col("l_discount")], 2),
    }
    batch = _tpch_like()
    for name, (exprs, want) in lists.items():
        nodes = resolve_exprs(exprs)
        out, n_fused = _run("jit", nodes, batch, monkeypatch)
        assert n_fused == want, name
        for node, got in zip(nodes, out):
            ref = node.evaluate(batch)
            assert got.dtype == ref.dtype
            assert got.cpu().to_pylist() == pytest.approx(
                ref.cpu().to_pylist(), rel=1e-12, nan_ok=True), name

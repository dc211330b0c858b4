"""Host half of the fused expression path (daft_amd/kernels/fused.py):
the oracle corpus guards, the postfix compiler checked with a host walker,
literal conversion, and the generated hipRTC source.  Runs without a GPU;
the kernels themselves are in test_gpu_fused.py."""
import datetime as dt
import random
import re

import pytest

import expr_cases as ec
from daft_amd import DataType, col
from daft_amd.expressions.expressions import Literal, resolve_exprs
from daft_amd.kernels import fused

FAMILIES = list(ec.case_lists())


# ---------------------------------------------------------------------------
# corpus guards: asserted on the oracle alone
# ---------------------------------------------------------------------------

def _nullable(case) -> bool:
    return any(c.endswith("_n") for c in case.cols)


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_boolean_cases_reach_every_outcome(family):
    """At n = 4099 every boolean case yields True, False and, where its
    inputs are nullable, None; every integer case whose inputs allow it
    has a result beyond +-2^53."""
    want = ec.expected(family, 4099)
    for case, w in zip(ec.case_lists()[family], want):
        if case.kind == "bool":
            seen = set(w)
            need = {True, False} | ({None} if _nullable(case) else set())
            assert need <= seen, (case.name, seen)
        if case.big:
            assert any(v is not None and abs(v) > ec.P53 for v in w), \
                case.name


def _same(a, b) -> bool:
    return (a != a and b != b) or (a == b and repr(a) == repr(b))


@pytest.mark.parametrize("n", ec.SIZES)
def test_corpus_edges_reach_the_last_tile(n):
    """Every edge value of every column a case names lands in the last
    partial tile (tail_len rows); where that tile is shorter than the
    edge list, the corpus parameter rotates the list through it.  A
    nullable column shows nulls there and each edge value somewhere."""
    t = ec.tail_len(n)
    cols = sorted({c for cases in ec.case_lists().values()
                   for case in cases for c in case.cols})
    tails = {c: [] for c in cols}
    whole = {c: [] for c in cols}
    for cyc in ec.cycles(n):
        rows = ec.corpus(n, cyc).rows
        for c in cols:
            tails[c] += [r[c] for r in rows[-t:]]
            whole[c] += [r[c] for r in rows]
    for c in cols:
        base = c[:-2] if c.endswith("_n") else c
        pool = tails[c] if base == c else whole[c]
        for e in ec.EDGES[base]:
            assert any(v is not None and _same(v, e) for v in pool), (c, e)
        if base != c and t * len(ec.cycles(n)) >= 3:
            assert None in tails[c], c
            assert any(v is not None for v in tails[c]), c
    # one column is null over the whole last tile
    assert all(r["i32_z"] is None for r in ec.corpus(n).rows[-t:])


# ---------------------------------------------------------------------------
# planner: declared dtypes, which cases fuse
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
def test_case_dtypes_and_jit_plan(family):
    cases = ec.case_lists()[family]
    batch = ec.corpus(257).batch
    nodes = ec.nodes(cases)
    for case, node in zip(cases, nodes):
        assert node.to_field(batch.schema).dtype == case.dtype, case.name
    plan = fused.plan_jit(nodes, batch)
    got = {m[0] for m in plan.out_meta}
    assert got == {k for k, c in enumerate(cases) if c.fused}
    # the source is produced without a device and is valid C: inf and nan
    # never appear as bare tokens
    assert not re.search(r"\b(inf|nan)\b", plan.src), plan.src
    assert plan.src.count("extern \"C\" __global__ void fe(") == 1
    if family == "float":
        assert "__builtin_inf()" in plan.src
        assert "__builtin_nan(\"\")" in plan.src
    # planning is deterministic: the kernel cache is keyed by the source
    assert fused.plan_jit(nodes, batch).src == plan.src


@pytest.mark.parametrize("family", FAMILIES)
def test_per_node_evaluation_matches_oracle(family):
    """What is not fused is answered per node, so that path has to equal
    the oracle as well (here on the host; the GPU run covers the device
    side for the unfused cases)."""
    corp = ec.corpus(1025)
    cases = ec.case_lists()[family]
    for case, node, want in zip(cases, ec.nodes(cases),
                                ec.expected(family, 1025)):
        ec.check(case, node.evaluate(corp.batch), want, "per-node")


def test_jit_shares_common_subtrees():
    batch = ec.corpus(257).batch
    nodes = resolve_exprs([col("dy1") * col("dy2") + col("dy1"),
                           col("dy1") * col("dy2") - col("dy2")])
    src = fused.plan_jit(nodes, batch).src
    assert len(re.findall(r"\) \* \(", src)) == 1, src


# ---------------------------------------------------------------------------
# postfix compiler against the oracle, through the host walker
# ---------------------------------------------------------------------------

def _walk(plan, rows):
    cols = [[r[s.name] for r in rows] for s in plan.cols]
    ins = list(zip(plan.prog.tolist()[0::2], plan.prog.tolist()[1::2]))
    return ec.walk_program(ins, plan.lits.tolist(), cols, plan.scales,
                           len(plan.out_meta), len(rows))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [1, 257])
def test_interpreter_program_matches_oracle(family, n):
    """Whatever the postfix compiler accepts must evaluate, opcode by
    opcode on an f64 stack, to the oracle's value on every row."""
    cases = ec.case_lists()[family]
    corp = ec.corpus(n)
    plan = fused.plan_interp(ec.nodes(cases), corp.batch)
    assert plan is not None
    outs = _walk(plan, corp.rows)
    want = ec.expected(family, n)
    for k, (i, _name, out_dt, code, pn) in enumerate(plan.out_meta):
        case = cases[i]
        assert case.fused and out_dt == case.dtype, case.name
        data, valid = [], []
        for v, ok in outs[k]:
            valid.append(ok)
            if code in (2, 3):
                assert v == int(v) and abs(v) <= ec.P53, (case.name, v)
                v = int(v)
            elif code == 6:
                v = v != 0.0
            elif code == 1:
                v = ec.f32(v)
            data.append(v)
        if not pn:
            assert all(valid), case.name
        ec.check_values(case, data, valid, want[i], "walker")


def test_interpreter_refuses_what_f64_cannot_hold():
    """The f64 stack is exact only below 2^53: 64-bit integer and
    timestamp columns and unbounded products are left to the JIT."""
    batch = ec.corpus(257).batch
    for e in (col("i64") + 1, col("u64") > col("u32"),
              col("tns") == col("tnsb"), col("tus") > ec.lit(ec.LIT_US),
              col("i32") * col("u32"), col("i32") * col("i32") > 5):
        (node,) = resolve_exprs([e])
        with pytest.raises(fused._Bail):
            fused._Compiler(batch).compile(node)
    # narrow products are bounded and wrap through OP_CAST
    (node,) = resolve_exprs([col("i16") * col("i8") + col("i32")])
    comp = fused._Compiler(batch)
    comp.compile(node)
    assert (fused.OP_CAST, fused.CAST_I32) in comp.ins


def test_between_and_is_in_stack_bookkeeping():
    batch = ec.corpus(257).batch
    (bt, isin) = resolve_exprs([col("i32").between(col("i16"), col("i8")),
                                col("i8").is_in([1, 2, 3, 4, 5, 6, 7, 8])])
    comp = fused._Compiler(batch)
    comp.compile(bt)
    assert comp.depth == 1 and comp.max_depth == 3
    ops = [o for o, _ in comp.ins]
    assert ops.count(fused.OP_GE) == 1 and ops.count(fused.OP_LE) == 1
    assert ops[-1] == fused.OP_AND
    comp = fused._Compiler(batch)
    comp.compile(isin)
    assert comp.depth == 1 and comp.max_depth == 3
    ops = [o for o, _ in comp.ins]
    assert ops.count(fused.OP_EQ) == 8 and ops.count(fused.OP_OR) == 7
    (too_many,) = resolve_exprs([col("i8").is_in(list(range(9)))])
    with pytest.raises(fused._Bail):
        fused._Compiler(batch).compile(too_many)


def _deep(depth: int):
    e = col("dy1")
    for _ in range(depth):
        e = col("dy2") - e          # right-nested: one slot per level
    return e


def test_max_stack_bail_and_rollback():
    """An expression deeper than the kernel's stack bails, and the
    expressions compiled before and after it are left intact."""
    batch = ec.corpus(257).batch
    ok1, ok2 = col("dy1") * col("dy2") + 1, col("dy1_n") - col("i8")
    (fits,) = resolve_exprs([_deep(fused._MAX_STACK - 1)])
    comp = fused._Compiler(batch)
    comp.compile(fits)
    assert comp.max_depth == fused._MAX_STACK
    (deep,) = resolve_exprs([_deep(fused._MAX_STACK)])
    with pytest.raises(fused._Bail):
        fused._Compiler(batch).compile(deep)
    with_deep = fused.plan_interp(resolve_exprs([ok1, _deep(8), ok2]), batch)
    without = fused.plan_interp(resolve_exprs([ok1, ok2]), batch)
    assert with_deep.prog.tolist() == without.prog.tolist()
    assert with_deep.lits.tolist() == without.lits.tolist()
    assert [s.name for s in with_deep.cols] == \
        [s.name for s in without.cols]
    assert [m[0] for m in with_deep.out_meta] == [0, 2]
    # a column only the bailed expression used is not kept either
    plan = fused.plan_interp(resolve_exprs(
        [ok1, col("i64") + col("f32"), ok2]), batch)
    assert "f32" not in [s.name for s in plan.cols]
    # the JIT has no stack: it takes the deep expression
    jit = fused.plan_jit(resolve_exprs([ok1, _deep(8), ok2]), batch)
    assert [m[0] for m in jit.out_meta] == [0, 1, 2]


def test_opcodes_match_the_kernel_source():
    """fused.py and csrc/fusedexpr.hip number the opcodes identically."""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "csrc",
                            "fusedexpr.hip")).read()
    enum = dict((k, int(v)) for k, v in
                re.findall(r"\b(OP_[A-Z]+) = (\d+)", src))
    mine = {k: v for k, v in vars(fused).items() if k.startswith("OP_")}
    assert enum == mine
    assert f"VSTACK = {fused._MAX_STACK};" in src


# ---------------------------------------------------------------------------
# literal conversion
# ---------------------------------------------------------------------------

def test_datetime_literals_convert_exactly():
    rng = random.Random(5)
    lo = dt.datetime(1970, 1, 1)
    span = int((dt.datetime(2052, 1, 1) - lo).total_seconds())
    for _ in range(20_000):
        v = lo + dt.timedelta(seconds=rng.randrange(span),
                              microseconds=rng.randrange(10**6))
        us = ec.us_of(v)
        for unit, want in (("us", us), ("ms", us // 1000),
                           ("ns", us * 1000)):
            t = DataType.timestamp(unit)
            assert fused._lit_scalar(Literal(v, t)) == (want, t), (v, unit)
    # the value from the issue, and the per-node path agrees
    v = ec.LIT_US
    assert fused._lit_scalar(Literal(v))[0] == 2231249559414149
    batch = ec.corpus(1).batch
    assert Literal(v).evaluate(batch).data.tolist() == [2231249559414149]
    # before the epoch: floor, not truncation
    old = dt.datetime(1960, 1, 1, 0, 0, 0, 1)
    assert fused._lit_scalar(Literal(old, DataType.timestamp("ms")))[0] == \
        ec.us_of(old) // 1000


def test_timezone_aware_literal_converts_or_bails():
    """Never a TypeError out of the compiler: the query must not crash
    only on a GPU."""
    batch = ec.corpus(257).batch
    for tz in (dt.timezone.utc, dt.timezone(dt.timedelta(hours=-8)),
               dt.timezone(dt.timedelta(hours=5, minutes=30))):
        v = dt.datetime(2024, 3, 1, 12, 0, 0, 250001, tzinfo=tz)
        (node,) = resolve_exprs([col("tus") <= ec.lit(v)])
        for compiler in (lambda: fused.plan_jit([node], batch),
                         lambda: fused.plan_interp([node], batch)):
            compiler()                       # must not raise
        try:
            got = fused._lit_scalar(Literal(v))[0]
        except fused._Bail:
            continue
        assert got == ec.us_of(v)
        assert Literal(v).evaluate(batch).data.tolist() == [ec.us_of(v)]


def test_literal_kinds():
    i64, f64 = DataType.int64(), DataType.float64()
    assert fused._lit_scalar(Literal(ec.I64_MIN, i64)) == (ec.I64_MIN, i64)
    assert fused._lit_scalar(Literal(3, f64)) == (3.0, f64)
    for bad in (Literal(1 << 63, i64), Literal(None, i64),
                Literal(2.5, i64), Literal("x")):
        with pytest.raises(fused._Bail):
            fused._lit_scalar(bad)
    assert fused._c_lit(ec.I64_MIN, i64) == "(-9223372036854775807LL - 1)"
    assert fused._c_lit(float("-inf"), f64) == "(-__builtin_inf())"

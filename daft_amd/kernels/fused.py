"""Fused expression compilation: a projection/predicate list becomes ONE
HIP kernel launch instead of a launch per expression node.

Two backends share one typed lowering (`_Lower`):

* the hipRTC JIT (csrc/fusedjit.hip) gets straight-line C in which every
  temp has the C type of the expression's dtype, so integers of any
  magnitude, unsigned 64-bit values and nanosecond timestamps are exact
  and integer arithmetic wraps at the declared width;
* the postfix interpreter (csrc/fusedexpr.hip) is the fallback when
  hipRTC is unavailable.  Its stack is f64, so it only accepts programs
  whose integer values provably stay below 2^53 (`_Compiler` tracks a
  magnitude bound) and rounds/wraps through OP_CAST.

The rule both follow: a fused result equals what per-node evaluation
defines (operands convert to the supertype, the operation runs in the
result dtype), or the expression is not fused and per-node evaluation
answers.  Anything outside the numeric core (strings, decimal-typed
results, float->int casts, UDFs, aggs, dict columns, broadcasts) is not
fused.
"""
from __future__ import annotations

import datetime as _dt
import math
import struct
from typing import Dict, List, Optional, Tuple

import torch

from ..expressions.expressions import (Alias, Between, BinaryOp, Cast,
                                       ColumnRef, ExprNode, FillNull, IfElse,
                                       IsIn, IsNull, Literal, Not)
from ..schema import DataType, TypeKind, supertype

OP_COL, OP_LIT = 0, 1
OP_ADD, OP_SUB, OP_MUL, OP_DIV = 2, 3, 4, 5
OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE = 6, 7, 8, 9, 10, 11
OP_AND, OP_OR, OP_NOT, OP_NEG = 12, 13, 14, 15
OP_ISNULL, OP_NOTNULL, OP_FILLNULL, OP_SELECT = 16, 17, 18, 19
OP_STORE = 20
OP_CAST = 21   # arg: CAST_* code below; rounds to f32 / wraps to an int width

_BIN = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL, "div": OP_DIV,
        "eq": OP_EQ, "ne": OP_NE, "lt": OP_LT, "le": OP_LE,
        "gt": OP_GT, "ge": OP_GE, "and": OP_AND, "or": OP_OR}
_CMP_OPS = ("eq", "ne", "lt", "le", "gt", "ge")

_IN_CODES = {torch.float64: 0, torch.float32: 1, torch.int64: 2,
             torch.int32: 3, torch.int16: 4, torch.int8: 5,
             torch.bool: 6, torch.uint8: 6, torch.uint32: 7,
             torch.uint64: 8}
_OUT_CODES = {torch.float64: 0, torch.float32: 1, torch.int64: 2,
              torch.int32: 3, torch.bool: 6}

# OP_CAST codes: the input codes above where they exist, plus bool/uint16
CAST_F32, CAST_I32, CAST_I16, CAST_I8 = 1, 3, 4, 5
CAST_U8, CAST_U32, CAST_BOOL, CAST_U16 = 6, 7, 9, 10

_MAX_STACK = 8  # must match VSTACK in csrc/fusedexpr.hip
_EXACT = 1 << 53   # integers up to here are exact on the f64 stack


class _Bail(Exception):
    pass


# ---------------------------------------------------------------------------
# types: every lowered node carries a DataType; kernels see its physical kind
# ---------------------------------------------------------------------------

_K = TypeKind
_INT_BITS = {_K.INT8: (8, True), _K.INT16: (16, True), _K.INT32: (32, True),
             _K.INT64: (64, True), _K.UINT8: (8, False),
             _K.UINT16: (16, False), _K.UINT32: (32, False),
             _K.UINT64: (64, False)}
_CTYPE = {_K.BOOL: "bool", _K.INT8: "signed char", _K.INT16: "short",
          _K.INT32: "int", _K.INT64: "long long",
          _K.UINT8: "unsigned char", _K.UINT16: "unsigned short",
          _K.UINT32: "unsigned int", _K.UINT64: "unsigned long long",
          _K.FLOAT32: "float", _K.FLOAT64: "double"}
_CAST_CODE = {_K.INT32: CAST_I32, _K.INT16: CAST_I16, _K.INT8: CAST_I8,
              _K.UINT8: CAST_U8, _K.UINT16: CAST_U16, _K.UINT32: CAST_U32}


def _pk(dt: DataType) -> TypeKind:
    """Physical kind the kernels compute in (date -> int32, timestamp and
    duration -> int64; decimals stay DECIMAL128 and only ever convert to
    float)."""
    if dt.kind in (_K.DATE, _K.TIMESTAMP, _K.DURATION):
        return dt.to_physical().kind
    if dt.kind in _CTYPE or dt.kind == _K.DECIMAL128:
        return dt.kind
    raise _Bail(f"dtype {dt}")


def _wrap(v: int, bits: int, signed: bool) -> int:
    v &= (1 << bits) - 1
    if signed and v >> (bits - 1):
        v -= 1 << bits
    return v


def _f32(v: float) -> float:
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:          # finite f64 beyond f32 range
        return math.copysign(math.inf, v)


class _N:
    """Lowered node.  kind: col lit conv arith cmp and or not isnull fill
    sel isin.  `dt` is the node's dtype; `key` identifies the value for
    common-subexpression reuse."""
    __slots__ = ("kind", "op", "args", "dt", "val", "key")

    def __init__(self, kind, dt, args=(), op=None, val=None):
        self.kind = kind
        self.op = op
        self.args = tuple(args)
        self.dt = dt
        self.val = val
        self.key = "%s:%s:%r:%r(%s)" % (
            kind, op, val, dt, ",".join(a.key for a in self.args))


def _lit_scalar(e: Literal) -> Tuple[object, DataType]:
    """Literal -> (bool | int | float, dtype) in the dtype's raw unit."""
    v, dt = e.value, e.dtype
    if v is None or dt is None:
        raise _Bail("null literal")
    if isinstance(v, bool):
        if dt.kind != _K.BOOL:
            raise _Bail("typed bool literal")
        return v, dt
    if isinstance(v, _dt.datetime):
        if dt.kind != _K.TIMESTAMP:
            raise _Bail("datetime literal dtype")
        from ..series import datetime_to_units
        return datetime_to_units(v, dt.timeunit), dt
    if isinstance(v, _dt.date):
        if dt.kind != _K.DATE:
            raise _Bail("date literal dtype")
        return (v - _dt.date(1970, 1, 1)).days, dt
    if isinstance(v, int):
        if dt.is_integer():
            bits, signed = _INT_BITS[dt.kind]
            if _wrap(v, bits, signed) != v:
                raise _Bail("literal out of range")
            return v, dt
        if dt.is_floating():
            v = float(v)
    if isinstance(v, float) and dt.is_floating():
        return (_f32(v) if dt.kind == _K.FLOAT32 else v), dt
    raise _Bail(f"literal {type(v).__name__}:{dt}")


class _Lower:
    """Expression tree -> typed nodes with every conversion explicit.
    Registers referenced columns (raises _Bail on unfusable ones)."""

    def __init__(self, batch):
        self.batch = batch
        self.n = len(batch)
        self.cols: List = []          # Series
        self.col_ix: Dict[str, int] = {}

    def mark(self):
        return len(self.cols), dict(self.col_ix)

    def rollback(self, mark):
        self.cols = self.cols[:mark[0]]
        self.col_ix = mark[1]

    def _dtype(self, e: ExprNode) -> DataType:
        try:
            return e.to_field(self.batch.schema).dtype
        except Exception:
            raise _Bail("untyped operand")

    def _super(self, a: DataType, b: DataType) -> DataType:
        try:
            return supertype(a, b)
        except TypeError:
            raise _Bail(f"no supertype {a},{b}")

    # -- columns -----------------------------------------------------------
    def col(self, name: str) -> _N:
        ix = self.col_ix.get(name)
        if ix is None:
            s = self.batch.column(name)
            if s.pyobjs is not None or s.data is None or s.is_dict() or \
                    s.children:
                raise _Bail(f"column {name} not fusable")
            if len(s) != self.n:
                raise _Bail("broadcast column")
            dt = s.dtype
            if not (dt.is_numeric() or dt.is_boolean() or dt.is_temporal()
                    or dt.is_decimal()):
                raise _Bail(f"dtype {dt}")
            if dt.is_decimal() and s.data.dtype != torch.int64:
                raise _Bail("wide decimal")
            if s.data.dtype not in _IN_CODES:
                raise _Bail(f"torch dtype {s.data.dtype}")
            _pk(dt)
            ix = len(self.cols)
            self.cols.append(s)
            self.col_ix[name] = ix
        return _N("col", self.cols[ix].dtype, val=ix)

    # -- conversions -------------------------------------------------------
    def conv(self, a: _N, dst: DataType) -> _N:
        src = a.dt
        sk, dk = _pk(src), _pk(dst)
        if src.is_temporal() or dst.is_temporal():
            if src.is_temporal() and dst.is_temporal():
                if src != dst:
                    raise _Bail("temporal unit mismatch")
                return a
            if not (src.is_temporal() and dst.is_integer()):
                raise _Bail(f"cast {src}->{dst}")
        if dk == _K.DECIMAL128:
            if src == dst:
                return a
            raise _Bail("cast to decimal")
        if sk == dk:
            return a if src == dst else _N("conv", dst, [a])
        if sk == _K.DECIMAL128 and not dst.is_floating():
            raise _Bail("decimal->int cast")
        if src.is_floating() and dst.is_integer():
            # torch truncates, and out-of-range values are undefined
            raise _Bail("float->int cast")
        if a.kind == "lit":
            v = a.val
            if dk == _K.BOOL:
                return _N("lit", dst, val=bool(v != 0))
            if dk in _INT_BITS:
                return _N("lit", dst, val=_wrap(int(v), *_INT_BITS[dk]))
            if dk == _K.FLOAT64:
                return _N("lit", dst, val=float(v))
            if isinstance(v, float) or abs(v) <= _EXACT:
                return _N("lit", dst, val=_f32(float(v)))
        if sk == _K.DECIMAL128 and dk == _K.FLOAT32:
            a = _N("conv", DataType.float64(), [a])
        return _N("conv", dst, [a])

    def to_bool(self, a: _N) -> _N:
        return self.conv(a, DataType.bool())

    # -- tree walk ---------------------------------------------------------
    def lower(self, e: ExprNode) -> _N:
        if isinstance(e, Alias):
            return self.lower(e.child)
        if isinstance(e, ColumnRef):
            return self.col(e.name)
        if isinstance(e, Literal):
            v, dt = _lit_scalar(e)
            return _N("lit", dt, val=v)
        if isinstance(e, BinaryOp):
            return self._binop(e)
        if isinstance(e, Not):
            return _N("not", DataType.bool(),
                      [self.to_bool(self.lower(e.child))])
        if isinstance(e, IsNull):
            return _N("isnull", DataType.bool(), [self.lower(e.child)],
                      op=bool(getattr(e, "negate", False)))
        if isinstance(e, FillNull):
            a, b = self.lower(e.child), self.lower(e.fill)
            r = self._super(a.dt, b.dt)
            if r.is_decimal():
                raise _Bail("decimal result")
            return _N("fill", r, [self.conv(a, r), self.conv(b, r)])
        if isinstance(e, IfElse):
            c = self.to_bool(self.lower(e.pred))
            t, f = self.lower(e.truthy), self.lower(e.falsy)
            r = self._super(t.dt, f.dt)
            if r.is_decimal():
                raise _Bail("decimal result")
            return _N("sel", r, [c, self.conv(t, r), self.conv(f, r)])
        if isinstance(e, Between):
            # per-node evaluation is (x >= lo) AND (x <= hi), Kleene AND
            return self.lower(BinaryOp(
                "and", BinaryOp("ge", e.child, e.lo),
                BinaryOp("le", e.child, e.hi)))
        if isinstance(e, IsIn):
            return self._isin(e)
        if isinstance(e, Cast):
            a = self.lower(e.child)
            src, dst = a.dt, e.dtype
            ok = (src.is_numeric() or src.is_boolean() or
                  src.is_temporal()) and \
                (dst.is_numeric() and not dst.is_decimal())
            if not ok:
                raise _Bail(f"cast {src}->{dst}")
            return self.conv(a, dst)
        raise _Bail(type(e).__name__)

    def _binop(self, e: BinaryOp) -> _N:
        if e.op not in _BIN:
            raise _Bail(f"binop {e.op}")
        a, b = self.lower(e.left), self.lower(e.right)
        if e.op in ("and", "or"):
            return _N(e.op, DataType.bool(),
                      [self.to_bool(a), self.to_bool(b)])
        lt, rt = a.dt, b.dt
        if lt.is_temporal() or rt.is_temporal():
            # raw values are unit-dependent (days vs us): both sides must
            # agree on kind+unit
            if lt != rt:
                raise _Bail("temporal unit mismatch")
            if e.op in _CMP_OPS:
                return _N("cmp", DataType.bool(), [a, b], op=e.op)
            if e.op != "sub" or lt.kind not in (_K.DATE, _K.TIMESTAMP):
                raise _Bail("temporal arithmetic")
            r = self._dtype(e)
            if r.kind != _K.DURATION:
                raise _Bail("temporal arithmetic")
            i64 = DataType.int64()
            d = _N("arith", i64, [_N("conv", i64, [a]) if lt.kind == _K.DATE
                                  else a,
                                  _N("conv", i64, [b]) if lt.kind == _K.DATE
                                  else b], op="sub")
            if lt.kind == _K.DATE:      # date - date is a us duration
                d = _N("arith", i64,
                       [d, _N("lit", i64, val=86_400_000_000)], op="mul")
            return _N("conv", r, [d])
        if e.op in _CMP_OPS:
            s = self._super(lt, rt)
            if s.is_decimal():
                raise _Bail("decimal compare")
            return _N("cmp", DataType.bool(),
                      [self.conv(a, s), self.conv(b, s)], op=e.op)
        r = self._dtype(e)
        if not (r.is_integer() or r.is_floating()):
            raise _Bail(f"arithmetic result {r}")
        return _N("arith", r, [self.conv(a, r), self.conv(b, r)], op=e.op)

    def _isin(self, e: IsIn) -> _N:
        vals = getattr(e, "values", None)
        if not vals or len(vals) > 8:
            raise _Bail("is_in size")
        ty = type(vals[0])
        if ty not in (int, float, bool) or \
                any(type(v) is not ty for v in vals) or \
                any(isinstance(v, float) and v != v for v in vals):
            raise _Bail("is_in value")
        vdt = {int: DataType.int64(), float: DataType.float64(),
               bool: DataType.bool()}[ty]
        a = self.lower(e.child)
        s = self._super(a.dt, vdt)
        if s.is_decimal() or s.is_temporal():
            raise _Bail("is_in dtype")
        lits = [self.conv(_N("lit", vdt, val=_lit_scalar(
            Literal(v, vdt))[0]), s) for v in vals]
        return _N("isin", DataType.bool(), [self.conv(a, s)] + lits)


# ---------------------------------------------------------------------------
# interpreter backend: postfix program over an f64 stack
# ---------------------------------------------------------------------------

def _int_range(dt: DataType) -> Optional[Tuple[int, int]]:
    k = _pk(dt)
    if k == _K.BOOL:
        return 0, 1
    if k in _INT_BITS:
        bits, signed = _INT_BITS[k]
        return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed \
            else (0, (1 << bits) - 1)
    return None


class _Compiler:
    """Typed nodes -> postfix opcodes.  The kernel's stack is f64, so each
    integer-typed value carries a (lo, hi) bound: values must stay within
    +-2^53, and a result that can leave its dtype's range is wrapped by
    OP_CAST.  Anything that cannot be bounded bails."""

    def __init__(self, batch):
        self.batch = batch
        self.low = _Lower(batch)
        self.n = len(batch)
        self.ins: List[Tuple[int, int]] = []
        self.lits: List[float] = []
        self.depth = 0
        self.max_depth = 0
        self.any_valid = False        # any pushed slot may be invalid

    @property
    def cols(self):
        return self.low.cols

    @property
    def col_ix(self):
        return self.low.col_ix

    def mark(self):
        return (len(self.ins), len(self.lits), self.any_valid,
                self.low.mark())

    def rollback(self, mark):
        self.ins = self.ins[:mark[0]]
        self.lits = self.lits[:mark[1]]
        self.any_valid = mark[2]
        self.low.rollback(mark[3])
        self.depth = 0

    def _push(self, k: int = 1):
        self.depth += k
        if self.depth > _MAX_STACK:
            raise _Bail("stack too deep")
        self.max_depth = max(self.max_depth, self.depth)

    def _pop(self, k: int = 1):
        self.depth -= k

    def emit(self, op: int, arg: int = 0):
        self.ins.append((op, arg))

    def lit(self, v: float) -> int:
        self.lits.append(float(v))
        return len(self.lits) - 1

    def compile(self, e: ExprNode):
        self.node(self.low.lower(e))

    # returns the (lo, hi) integer bound of the pushed value, None = float
    def node(self, n: _N):
        k = n.kind
        if k == "col":
            s = self.cols[n.val]
            if s.data.dtype in (torch.int64, torch.uint64) and \
                    not s.dtype.is_decimal():
                raise _Bail("64-bit integer column on the f64 stack")
            if s.validity is not None:
                self.any_valid = True
            self.emit(OP_COL, n.val)
            self._push()
            return _int_range(s.dtype)
        if k == "lit":
            v = n.val
            if isinstance(v, int) and not isinstance(v, bool) and \
                    abs(v) >= _EXACT:
                raise _Bail("literal beyond f64 exact range")
            self.emit(OP_LIT, self.lit(float(v)))
            self._push()
            return None if isinstance(v, float) else (int(v), int(v))
        if k == "conv":
            return self._conv(n)
        if k == "arith":
            a = self.node(n.args[0])
            b = self.node(n.args[1])
            self.emit(_BIN[n.op])
            self._pop()
            pk = _pk(n.dt)
            if pk == _K.FLOAT64:
                return None
            if pk == _K.FLOAT32:
                self.emit(OP_CAST, CAST_F32)
                return None
            c = [{"add": x + y, "sub": x - y, "mul": x * y}[n.op]
                 for x in a for y in b]
            return self._fit((min(c), max(c)), n.dt)
        if k == "cmp":
            self.node(n.args[0])
            self.node(n.args[1])
            self.emit(_BIN[n.op])
            self._pop()
            return 0, 1
        if k in ("and", "or"):
            self.node(n.args[0])
            self.node(n.args[1])
            self.emit(_BIN[k])
            self._pop()
            return 0, 1
        if k == "not":
            self.node(n.args[0])
            self.emit(OP_NOT)
            return 0, 1
        if k == "isnull":
            self.node(n.args[0])
            self.emit(OP_NOTNULL if n.op else OP_ISNULL)
            return 0, 1
        if k == "fill":
            a = self.node(n.args[0])
            b = self.node(n.args[1])
            self.emit(OP_FILLNULL)
            self._pop()
            return _hull(a, b)
        if k == "sel":
            self.node(n.args[0])
            a = self.node(n.args[1])
            b = self.node(n.args[2])
            self.emit(OP_SELECT)
            self._pop(2)
            return _hull(a, b)
        if k == "isin":
            # child is re-emitted per value (columns re-load from cache)
            for j, v in enumerate(n.args[1:]):
                self.node(n.args[0])
                self.node(v)
                self.emit(OP_EQ)
                self._pop()
                if j:
                    self.emit(OP_OR)
                    self._pop()
            return 0, 1
        raise _Bail(k)

    def _fit(self, b: Tuple[int, int], dt: DataType):
        """Bound after an integer result of dtype dt: wrap when it can
        leave the dtype's range; bail when f64 cannot hold it exactly."""
        if max(abs(b[0]), abs(b[1])) > _EXACT:
            raise _Bail("integer beyond f64 exact range")
        r = _int_range(dt)
        if r[0] <= b[0] and b[1] <= r[1]:
            return b
        code = _CAST_CODE.get(_pk(dt))
        if code is None:
            raise _Bail("64-bit wrap")
        self.emit(OP_CAST, code)
        return r

    def _conv(self, n: _N):
        src = n.args[0]
        b = self.node(src)
        sk, dk = _pk(src.dt), _pk(n.dt)
        if sk == _K.DECIMAL128:
            return None               # OP_COL already descaled to f64
        if dk == _K.BOOL:
            self.emit(OP_CAST, CAST_BOOL)
            return 0, 1
        if dk == _K.FLOAT64:
            return None               # ints here are bounded by 2^53
        if dk == _K.FLOAT32:
            self.emit(OP_CAST, CAST_F32)
            return None
        if b is None:
            raise _Bail("float->int cast")
        return self._fit(b, n.dt)


def _hull(a, b):
    if a is None or b is None:
        return None
    return min(a[0], b[0]), max(a[1], b[1])


class FusedPlan:
    """Host-side plan for the interpreter kernel."""
    __slots__ = ("prog", "lits", "cols", "codes", "scales", "out_meta", "n")

    def __init__(self, prog, lits, cols, codes, scales, out_meta, n):
        self.prog = prog
        self.lits = lits
        self.cols = cols
        self.codes = codes
        self.scales = scales
        self.out_meta = out_meta
        self.n = n


class JitPlan:
    """Host-side plan for the hipRTC kernel."""
    __slots__ = ("src", "cols", "out_meta", "n")

    def __init__(self, src, cols, out_meta, n):
        self.src = src
        self.cols = cols
        self.out_meta = out_meta
        self.n = n


def _fusable_outputs(exprs: List[ExprNode]):
    """(index, expr) of the expressions worth fusing."""
    for i, e in enumerate(exprs):
        base = e
        while isinstance(base, Alias):
            base = base.child
        if isinstance(base, (ColumnRef, Literal)):
            continue      # zero-copy via normal eval; fusing would copy
        yield i, e


def _out_code(e: ExprNode, batch):
    try:
        f = e.to_field(batch.schema)
    except Exception:
        raise _Bail("untyped expression")
    out_dt = f.dtype
    tdt = out_dt.to_torch() if out_dt.is_fixed_width() else None
    if tdt not in _OUT_CODES or out_dt.is_decimal():
        raise _Bail(f"out dtype {out_dt}")
    return f, _OUT_CODES[tdt]


def plan_interp(exprs: List[ExprNode], batch) -> Optional[FusedPlan]:
    """Host-only: compile as many of `exprs` as possible into one postfix
    program.  None when nothing fuses or fusion is not worthwhile (fewer
    than 4 instructions)."""
    comp = _Compiler(batch)
    out_meta = []
    for i, e in _fusable_outputs(exprs):
        mark = comp.mark()
        try:
            f, code = _out_code(e, batch)
            av_before = comp.any_valid
            comp.any_valid = False
            root = comp.low.lower(e)
            if _pk(root.dt) != _pk(f.dtype):
                raise _Bail("result dtype mismatch")
            comp.node(root)
            produces_null = comp.any_valid
            comp.any_valid = comp.any_valid or av_before
            comp.emit(OP_STORE, len(out_meta))
            comp._pop()
            out_meta.append((i, f.name, f.dtype, code, produces_null))
        except _Bail:
            comp.rollback(mark)
    if not out_meta or len(comp.ins) < 4:
        return None
    import itertools
    prog = torch.tensor(list(itertools.chain.from_iterable(comp.ins)),
                        dtype=torch.int32)
    lits = torch.tensor(comp.lits, dtype=torch.float64)
    codes = [_IN_CODES[s.data.dtype] for s in comp.cols]
    # the kernel DIVIDES by the scale: 10**s is exact in f64, 10.0**-s is not
    scales = [float(10 ** s.dtype.scale) if s.dtype.is_decimal() else 1.0
              for s in comp.cols]
    return FusedPlan(prog, lits, list(comp.cols), codes, scales, out_meta,
                     len(batch))


def _finish(exprs: List[ExprNode], batch, out_meta, flat) -> List:
    """Wrap kernel outputs as Series; per-node eval for the rest."""
    from ..series import Series
    results: List = [None] * len(exprs)
    for k, (i, name, out_dt, code, pn) in enumerate(out_meta):
        data = flat[2 * k]
        valid = flat[2 * k + 1] if pn else None
        if valid is not None and bool(valid.all().item()):
            valid = None
        if out_dt.to_torch() != data.dtype:
            data = data.to(out_dt.to_torch())
        results[i] = Series(name, out_dt, data=data, validity=valid)
    for i, e in enumerate(exprs):
        if results[i] is None:
            results[i] = e.evaluate(batch)
    return results


def try_fuse(exprs: List[ExprNode], batch) -> Optional[List]:
    """Compile as many of `exprs` as possible into one kernel; returns the
    full result list (fused + fallback per-node eval) or None when fusion
    is not worthwhile."""
    import os
    if os.environ.get("DAFT_AMD_DISABLE_FUSED"):
        return None
    if batch.device.type != "cuda" or len(batch) == 0:
        return None
    from . import load_native
    native = load_native()
    if native is None:
        return None

    jit = try_fuse_jit(exprs, batch)
    if jit is not None:
        return jit

    plan = plan_interp(exprs, batch)
    if plan is None:
        return None
    m = plan.out_meta
    flat = native.fused_eval(
        plan.prog, plan.lits, [s.data for s in plan.cols],
        [s.validity for s in plan.cols], plan.codes, plan.scales,
        [x[3] for x in m], [1.0] * len(m), [1 if x[4] else 0 for x in m],
        plan.n)
    return _finish(exprs, batch, m, flat)


# ---------------------------------------------------------------------------
# hipRTC codegen: straight-line kernel per (expression list, schema,
# validity pattern), compiled once per process and cached by source
# ---------------------------------------------------------------------------

_C_LOAD_T = {0: "double", 1: "float", 2: "long long", 3: "int", 4: "short",
             5: "signed char", 6: "unsigned char", 7: "unsigned int",
             8: "unsigned long long"}


def _c_lit(v, dt: DataType) -> str:
    k = _pk(dt)
    if k == _K.BOOL:
        return "true" if v else "false"
    if k in _INT_BITS:
        v = int(v)
        if k == _K.UINT64:
            return f"{v}ULL"
        if v == -(1 << 63):
            return "(-9223372036854775807LL - 1)"
        return f"(({_CTYPE[k]}){v}LL)"
    v = float(v)
    if v != v:
        body = "__builtin_nan(\"\")"
    elif v in (math.inf, -math.inf):
        body = "__builtin_inf()" if v > 0 else "-__builtin_inf()"
    else:
        body = repr(v)
    return f"((float)({body}))" if k == _K.FLOAT32 else f"({body})"


class _CodeGen:
    """Typed nodes -> C statements.  Every temp is declared in the C type
    of its dtype; returns (value C expr, validity C expr or None = always
    valid).  One generator per list: temps and CSE are shared across its
    expressions."""

    def __init__(self, low: _Lower):
        self.low = low
        self.lines: List[str] = []
        self.tmp = 0
        self.cache: Dict[str, Tuple[str, Optional[str]]] = {}

    def mark(self):
        return len(self.lines), self.tmp, dict(self.cache)

    def rollback(self, mark):
        self.lines = self.lines[:mark[0]]
        self.tmp = mark[1]
        self.cache = mark[2]

    def t(self) -> str:
        self.tmp += 1
        return f"t{self.tmp}"

    def emit(self, typ: str, expr: str) -> str:
        name = self.t()
        self.lines.append(f"      const {typ} {name} = {expr};")
        return name

    def gen(self, n: _N) -> Tuple[str, Optional[str]]:
        if n.kind == "lit":
            return _c_lit(n.val, n.dt), None
        hit = self.cache.get(n.key)
        if hit is None:
            hit = self.cache[n.key] = self._gen(n)
        return hit

    def _gen(self, n: _N) -> Tuple[str, Optional[str]]:
        k = n.kind
        if k == "col":
            ix = n.val
            s = self.low.cols[ix]
            ct = _C_LOAD_T[_IN_CODES[s.data.dtype]]
            if s.dtype.is_boolean():
                v = self.emit("bool", f"((const unsigned char*)C{ix}d)[i] "
                                      f"!= 0")
            else:
                v = self.emit(ct, f"((const {ct}*)C{ix}d)[i]")
            vv = None
            if s.validity is not None:
                vv = self.emit("bool", f"C{ix}v[i]")
            return v, vv
        if k == "conv":
            a, av = self.gen(n.args[0])
            src, dk = n.args[0].dt, _pk(n.dt)
            if src.is_decimal():
                # exact power of ten: one correctly rounded division
                return self.emit("double", f"(double)({a}) / "
                                 f"{float(10 ** src.scale)!r}"), av
            if dk == _K.BOOL:
                return self.emit("bool", f"({a}) != 0"), av
            return self.emit(_CTYPE[dk], f"({_CTYPE[dk]})({a})"), av
        if k == "arith":
            a, av = self.gen(n.args[0])
            b, bv = self.gen(n.args[1])
            cop = {"add": "+", "sub": "-", "mul": "*", "div": "/"}[n.op]
            ct = _CTYPE[_pk(n.dt)]
            if n.dt.is_floating():
                out = self.emit(ct, f"({a}) {cop} ({b})")
            else:
                # unsigned arithmetic wraps; the cast back narrows
                out = self.emit(ct, f"({ct})((unsigned long long)({a}) "
                                    f"{cop} (unsigned long long)({b}))")
            return out, self._and_valid(av, bv)
        if k == "cmp":
            a, av = self.gen(n.args[0])
            b, bv = self.gen(n.args[1])
            cop = {"eq": "==", "ne": "!=", "lt": "<", "le": "<=",
                   "gt": ">", "ge": ">="}[n.op]
            return self.emit("bool", f"({a}) {cop} ({b})"), \
                self._and_valid(av, bv)
        if k in ("and", "or"):
            # Kleene three-valued logic (matches kernels.logical_op)
            a, av = self.gen(n.args[0])
            b, bv = self.gen(n.args[1])
            op = "&&" if k == "and" else "||"
            out = self.emit("bool", f"({a}) {op} ({b})")
            if av is None and bv is None:
                return out, None
            avv = av or "true"
            bvv = bv or "true"
            neg = "!" if k == "and" else ""
            vv = self.emit("bool",
                           f"(({avv}) && ({bvv})) || (({avv}) && "
                           f"{neg}({a})) || (({bvv}) && {neg}({b}))")
            return out, vv
        if k == "not":
            a, av = self.gen(n.args[0])
            return self.emit("bool", f"!({a})"), av
        if k == "isnull":
            _, av = self.gen(n.args[0])
            if av is None:
                return ("true" if n.op else "false"), None
            return self.emit("bool", f"({av})" if n.op else f"!({av})"), \
                None
        if k == "fill":
            a, av = self.gen(n.args[0])
            b, bv = self.gen(n.args[1])
            if av is None:
                return a, None
            out = self.emit(_CTYPE[_pk(n.dt)], f"({av}) ? ({a}) : ({b})")
            if bv is None:
                return out, None
            return out, self.emit("bool", f"({av}) || ({bv})")
        if k == "sel":
            c, cv = self.gen(n.args[0])
            t_, tv = self.gen(n.args[1])
            f_, fv = self.gen(n.args[2])
            # a null predicate takes the falsy branch
            m = c if cv is None else self.emit("bool", f"({c}) && ({cv})")
            out = self.emit(_CTYPE[_pk(n.dt)],
                            f"({m}) ? ({t_}) : ({f_})")
            if tv is None and fv is None:
                return out, None
            return out, self.emit(
                "bool", f"({m}) ? ({tv or 'true'}) : ({fv or 'true'})")
        if k == "isin":
            a, av = self.gen(n.args[0])
            parts = [f"(({a}) == {self.gen(v)[0]})" for v in n.args[1:]]
            return self.emit("bool", " || ".join(parts)), av
        raise _Bail(k)

    def _and_valid(self, a: Optional[str], b: Optional[str]) -> Optional[str]:
        if a is None:
            return b
        if b is None:
            return a
        return self.emit("bool", f"({a}) && ({b})")


_C_STORE_T = {0: "double", 1: "float", 2: "long long", 3: "int", 6: "bool"}


def _gen_source(cols, gens, out_meta) -> str:
    """Full kernel source: hoisted column pointers, grid-stride row loop,
    straight-line body."""
    head = [
        "extern \"C\" __global__ void fe(const long long* __restrict__ "
        "cols, const long long* __restrict__ outs, long long n) {",
    ]
    for ix, s in enumerate(cols):
        head.append(f"  const void* C{ix}d = (const void*)cols[{ix} * 2];")
        if s.validity is not None:
            head.append(f"  const bool* C{ix}v = "
                        f"(const bool*)cols[{ix} * 2 + 1];")
    for k, m in enumerate(out_meta):
        head.append(f"  void* O{k}d = (void*)outs[{k} * 2];")
        if m[4]:
            head.append(f"  bool* O{k}v = (bool*)outs[{k} * 2 + 1];")
    head.append("  const long long stride = (long long)gridDim.x * "
                "blockDim.x;")
    head.append("  for (long long i = (long long)blockIdx.x * blockDim.x + "
                "threadIdx.x; i < n; i += stride) {")
    body: List[str] = []
    for k, (lines, val, vld) in enumerate(gens):
        body.extend(lines)
        ct = _C_STORE_T[out_meta[k][3]]
        body.append(f"      (({ct}*)O{k}d)[i] = {val};")
        if out_meta[k][4]:
            body.append(f"      O{k}v[i] = {vld if vld else 'true'};")
    tail = ["  }", "}"]
    return "\n".join(head + body + tail) + "\n"


def plan_jit(exprs: List[ExprNode], batch) -> Optional[JitPlan]:
    """Host-only: generate the kernel source for as many of `exprs` as
    possible.  None when nothing fuses."""
    low = _Lower(batch)
    cg = _CodeGen(low)      # ONE generator: shared temps + cross-expr CSE
    gens = []
    out_meta = []
    for i, e in _fusable_outputs(exprs):
        mark = (low.mark(), cg.mark())
        try:
            f, code = _out_code(e, batch)
            root = low.lower(e)
            if _pk(root.dt) != _pk(f.dtype):
                raise _Bail("result dtype mismatch")
            lines_before = len(cg.lines)
            val, vld = cg.gen(root)
            gens.append((cg.lines[lines_before:], val, vld))
            out_meta.append((i, f.name, f.dtype, code, vld is not None))
        except _Bail:
            low.rollback(mark[0])
            cg.rollback(mark[1])
    if not out_meta or len(cg.lines) < 3:
        return None
    return JitPlan(_gen_source(low.cols, gens, out_meta), list(low.cols),
                   out_meta, len(batch))


def try_fuse_jit(exprs: List[ExprNode], batch) -> Optional[List]:
    """hipRTC path: compile the list to a straight-line kernel.  Returns
    the full result list or None (caller falls back to the interpreter)."""
    import os
    if os.environ.get("DAFT_AMD_DISABLE_JIT"):
        return None
    from . import load_native
    native = load_native()
    if native is None or not hasattr(native, "fused_eval_jit"):
        return None
    plan = plan_jit(exprs, batch)
    if plan is None:
        return None
    m = plan.out_meta
    try:
        flat = native.fused_eval_jit(
            plan.src, [s.data for s in plan.cols],
            [s.validity for s in plan.cols], [x[3] for x in m],
            [1 if x[4] else 0 for x in m], plan.n)
    except RuntimeError:
        return None        # hiprtc unavailable/failed: interpreter path
    return _finish(exprs, batch, m, flat)

"""Corpus, exact Python oracle and check drivers for the fused expression
kernels (test_fused_compile.py on the CPU, test_gpu_fused.py on the HIP
kernels).  A plain helper module: no fixtures, not collected.

The oracle functions use Python `int`, `fractions.Fraction`,
`decimal.Decimal` and `struct` only and never call daft_amd or torch.  What
they encode is the evaluation rule of the expression layer: operands
convert to the supertype, the operation runs in the result dtype (integers
wrap at its width, Float32 rounds after every operation), a decimal
converts to Float64 as f64(unscaled) / 10**scale, and nulls propagate
(Kleene for and/or; a null if_else predicate takes the falsy branch)."""
from __future__ import annotations

import datetime as dt
import functools
import math
import random
import struct
from decimal import Decimal
from fractions import Fraction
from typing import Callable, List, NamedTuple, Optional

import numpy as np
import torch

from daft_amd import DataType, Series, col, lit
from daft_amd.expressions.expressions import resolve_exprs
from daft_amd.recordbatch import RecordBatch

# ---------------------------------------------------------------------------
# oracle helpers
# ---------------------------------------------------------------------------

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
P53 = 1 << 53


def wrap(v: int, bits: int, signed: bool) -> int:
    v &= (1 << bits) - 1
    if signed and v >= 1 << (bits - 1):
        v -= 1 << bits
    return v


def f32(v: float) -> float:
    """Round an f64 to the nearest f32 (returned as a Python float)."""
    try:
        return struct.unpack("<f", struct.pack("<f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def _finite(*vs) -> bool:
    return all(math.isfinite(v) for v in vs)


def _to_float(q: Fraction) -> float:
    try:
        return float(q)          # correctly rounded, subnormals included
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def fop(op: str, a: float, b: float) -> float:
    """One IEEE f64 operation, computed exactly in Fraction and rounded
    once.  Non-finite operands and division by zero follow IEEE 754."""
    if not _finite(a, b) or (op == "/" and b == 0):
        if op == "/" and b == 0 and _finite(a):
            if a == 0 or a != a:
                return math.nan
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
        return {"+": lambda: a + b, "-": lambda: a - b,
                "*": lambda: a * b, "/": lambda: a / b}[op]()
    fa, fb = Fraction(a), Fraction(b)
    q = {"+": fa + fb, "-": fa - fb, "*": fa * fb,
         "/": (fa / fb) if fb else None}[op]
    if q == 0:                   # IEEE signed zero
        if op == "*" or op == "/":
            neg = math.copysign(1, a) * math.copysign(1, b) < 0
        elif op == "+":
            neg = math.copysign(1, a) < 0 and math.copysign(1, b) < 0
        else:
            neg = math.copysign(1, a) < 0 and math.copysign(1, b) > 0
        return -0.0 if neg else 0.0
    return _to_float(q)


def fop32(op: str, a: float, b: float) -> float:
    """One IEEE f32 operation on f32-valued operands: rounding the exact
    result to f64 and then to f32 is innocuous for + - * / (53 >= 2*24+2)."""
    return f32(fop(op, a, b))


def i2f(v: int) -> float:
    return _to_float(Fraction(v))


def dec_f64(k: int, scale: int) -> float:
    """Decimal -> Float64 as the cast defines it: the unscaled integer
    converts to f64, then ONE correctly rounded division by 10**scale.
    For |k| < 2^53 this is the correctly rounded decimal value."""
    v = _to_float(Fraction(i2f(k)) / (10 ** scale))
    if abs(k) < P53:
        assert v == float(Decimal(k).scaleb(-scale))
    return v


def kleene_and(a: Optional[bool], b: Optional[bool]) -> Optional[bool]:
    if a is False or b is False:
        return False
    if a is None or b is None:
        return None
    return True


def kleene_or(a: Optional[bool], b: Optional[bool]) -> Optional[bool]:
    if a is True or b is True:
        return True
    if a is None or b is None:
        return None
    return False


def knot(a: Optional[bool]) -> Optional[bool]:
    return None if a is None else not a


def nn(f: Callable, *vs):
    """Null-propagating application."""
    return None if any(v is None for v in vs) else f(*vs)


def us_of(v: dt.datetime) -> int:
    """Exact microseconds since the epoch from the calendar fields."""
    if v.tzinfo is not None:
        off = v.utcoffset()
        v = v.replace(tzinfo=None)
        extra = -(off.days * 86400 + off.seconds) * 10**6 - off.microseconds
    else:
        extra = 0
    days = v.toordinal() - dt.date(1970, 1, 1).toordinal()
    return ((days * 24 + v.hour) * 60 + v.minute) * 60 * 10**6 + \
        v.second * 10**6 + v.microsecond + extra


# ---------------------------------------------------------------------------
# corpus
# ---------------------------------------------------------------------------

L = 16                     # edge values per column
TILE = 1024                # interpreter rows per block (256 threads x 4)
SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 4099]

LIT_US = dt.datetime(2040, 9, 14, 15, 32, 39, 414149)     # issue item 5
LIT_TZ = dt.datetime(2024, 3, 1, 12, 0, 0, 250001,
                     tzinfo=dt.timezone(dt.timedelta(hours=5, minutes=30)))
LIT_NS = dt.datetime(2023, 11, 14, 22, 13, 20, 123457)
LIT_DATE = dt.date(1994, 1, 1)
US0, TZ0, NS0 = us_of(LIT_US), us_of(LIT_TZ), us_of(LIT_NS) * 1000
D0 = (LIT_DATE - dt.date(1970, 1, 1)).days
NS_BASE = 1_700_000_000_123_456_789
F32_MAX = 3.4028234663852886e38
F32_TINY = 1.401298464324817e-45

EDGES = {
    "i64": [0, 1, -1, I64_MIN, I64_MAX, P53 - 1, P53, P53 + 1, -(P53 + 1),
            P53 + 2, 300, -129, 1 << 31, -(1 << 31) - 1, 1 << 62, 7],
    "i32": [0, 1, -1, -(1 << 31), (1 << 31) - 1, 300, -129, 65536, 46341,
            -46341, 127, 128, -128, 1 << 30, -(1 << 30), 7],
    "i16": [0, 1, -1, -32768, 32767, 300, -129, 255, 256, 127, 128, -128,
            2, 3, 5, 7],
    "i8": [0, 1, -1, -128, 127, 2, 3, 5, 7, 100, -100, 64, -64, 44, 10, -10],
    "u8": [0, 1, 255, 128, 127, 2, 3, 5, 7, 100, 200, 64, 44, 10, 254, 129],
    "u32": [0, 1, (1 << 32) - 1, 1 << 31, (1 << 31) - 1, 65536, 300, 7,
            (1 << 32) - 2, 46341, 65535, 3, 5, 100, (1 << 24) + 1, 1 << 30],
    "u64": [0, 1, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, P53 - 1, P53,
            P53 + 1, (1 << 63) + 1, (1 << 64) - 2, 1 << 32, 300, 7, 1 << 62,
            P53 + 2, 5],
    "f64": [0.0, -0.0, math.nan, math.inf, -math.inf, 1e300, 5e-324,
            16777217.0, 0.1, -0.1, 1.0, -1e300, 0.35, 0.57, 2.5, 5.0],
    "f32": [0.0, -0.0, math.nan, math.inf, -math.inf, f32(1e30), F32_TINY,
            16777216.0, f32(0.1), -f32(0.1), 1.0, F32_MAX, 0.5, 2.5, -1.0,
            5.0],
    "b": [True, False] * 8,
    "d": [0, 1, -1, D0, D0 - 1, D0 + 1, -25567, 47482, 10957, 10956, 19000,
          20000, 365, 366, D0 + 365, D0 + 364],
    "tus": [0, 1, -1, US0, US0 - 1, US0 + 1, TZ0, TZ0 - 1, TZ0 + 1, P53 + 1,
            -(P53 + 1), 1_700_000_000_000_000, 1_700_000_000_000_001,
            I64_MAX, I64_MIN, 7],
    "tns": [NS_BASE, NS_BASE + 1, NS_BASE - 1, NS_BASE + 2, 0, 1, -1,
            I64_MAX, I64_MIN, P53, P53 + 1, NS_BASE + 1000, NS0, NS0 + 1,
            NS0 - 1, NS_BASE - 2],
    "dec3": [35, 57, 69, 7, 5, 0, -35, -57, -69, -7, -5, 999, -999, 6, 70,
             34],
    "dec12": [35, 57, 69, 7, 5, 0, -35, -57, 12345678, 12345677, 12345679,
              10**12 - 1, -(10**12 - 1), 700, 500, -7],
    "dec18": [35, 57, 69, 7, 5, 0, -35, -57, -69, 10**18 - 1,
              -(10**18 - 1), 7000000, 6999999, 7000001, P53 + 1, -7],
}
assert all(len(v) == L for v in EDGES.values())

DTYPES = {
    "i64": DataType.int64(), "i32": DataType.int32(),
    "i16": DataType.int16(), "i8": DataType.int8(), "u8": DataType.uint8(),
    "u32": DataType.uint32(), "u64": DataType.uint64(),
    "f64": DataType.float64(), "f32": DataType.float32(),
    "b": DataType.bool(), "d": DataType.date(),
    "tus": DataType.timestamp("us"), "tns": DataType.timestamp("ns"),
    "dec3": DataType.decimal128(3, 2), "dec12": DataType.decimal128(12, 4),
    "dec18": DataType.decimal128(18, 6),
}
_NP = {"i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8,
       "u8": np.uint8, "u32": np.uint32, "u64": np.uint64,
       "f64": np.float64, "f32": np.float32, "b": np.bool_, "d": np.int32,
       "tus": np.int64, "tns": np.int64, "dec3": np.int64,
       "dec12": np.int64, "dec18": np.int64}
_SMALL = [0.1, 0.35, 0.57, 1.0, 2.5, 5.0, -0.1, 0.0]


def _rand(name: str, rng: random.Random):
    e = EDGES[name]
    if name == "b":
        return rng.random() < 0.5
    if name == "f64":
        return rng.choice(_SMALL) if rng.random() < 0.3 \
            else rng.uniform(-100, 100)
    if name == "f32":
        return f32(rng.choice(_SMALL) if rng.random() < 0.3
                   else rng.uniform(-100, 100))
    if name in ("tus", "tns", "d"):
        return rng.choice(e[:9] if name != "tns" else e[:4] + e[12:15]) + \
            rng.randint(-2, 2)
    lo, hi = min(e), max(e)
    if name.startswith("dec"):
        return rng.randint(-99, 99) if rng.random() < 0.5 \
            else rng.randint(lo, hi)
    if rng.random() < 0.5:
        return rng.randint(max(lo, -8), min(hi, 8))
    return rng.randint(lo, hi)


def tail_len(n: int) -> int:
    """Rows of the last partial interpreter tile (a full one counts as
    its last 256 rows, one block of the JIT grid)."""
    return n % TILE or min(n, 256)


def cycles(n: int) -> List[int]:
    """Corpus parameters that, together, put every edge value into the
    last partial tile.  One suffices when the tile holds all L edges; a
    shorter tile (n = 1, 1025, 4099) rotates the edge list through it."""
    t = tail_len(n)
    if t >= L:
        return [0]
    # a column shorter than two edge lists has no head to show the values
    # its tail nulls hide: go round twice, the null slots shift by one
    return list(range(0, 2 * L if n < 2 * L else L, t))


def _place(n: int, cycle: int, edges: list, fill: Callable) -> list:
    """Edges at the first rows and, rotated by `cycle`, at the last rows."""
    out = [edges[i] if i < L else fill() for i in range(n)]
    for j in range(min(L, n)):
        out[n - 1 - j] = edges[(j + cycle) % L]
    return out


class Corpus(NamedTuple):
    batch: RecordBatch       # on the CPU; move with .to(device)
    rows: list               # one dict per row: column name -> raw value


def _series(name: str, kind: str, vals: list) -> Series:
    valid = [v is not None for v in vals]
    zero = False if kind == "b" else 0
    arr = np.array([zero if v is None else v for v in vals],
                   dtype=_NP[kind])
    return Series(name, DTYPES[kind], data=torch.from_numpy(arr),
                  validity=None if all(valid)
                  else torch.tensor(valid, dtype=torch.bool))


@functools.lru_cache(maxsize=8)
def corpus(n: int, cycle: int = 0) -> Corpus:
    """Seeded corpus: every loadable type with and without validity
    (`x` / `x_n`), helper columns for the float and compare cases, one
    string column, and `i32_z`, null over the whole last tile."""
    rng = random.Random(1_000_003 * n + cycle)
    data = {}
    kinds = {}
    for name in EDGES:
        vals = _place(n, cycle, EDGES[name],
                      functools.partial(_rand, name, rng))
        data[name], kinds[name] = vals, name
        # nullable twin: other random fill; nulls at every third edge
        # slot (another third at the head than at the tail, so each edge
        # value stays visible somewhere) and ~15% elsewhere
        tw = _place(n, cycle, EDGES[name],
                    functools.partial(_rand, name, rng))
        for i in range(n):
            j = n - 1 - i
            if j < L:
                null = (j + cycle) % 3 == 2
            elif i < L:
                null = i % 3 == 1
            else:
                null = rng.random() < 0.15
            if null:
                tw[i] = None
        data[name + "_n"], kinds[name + "_n"] = tw, name
    # neighbours one unit away, beyond f64 resolution
    data["i64b"] = [wrap(v + (i % 3) - 1, 64, True)
                    for i, v in enumerate(data["i64"])]
    data["tnsb"] = [wrap(v + (i % 3) - 1, 64, True)
                    for i, v in enumerate(data["tns"])]
    kinds["i64b"], kinds["tnsb"] = "i64", "tns"
    # dyadic floats: multiples of 1/8 below 2^20, every product exact
    dy = [0.0, -0.0, 0.125, -0.125, 1048575.875, -1048575.875, 1.0, 8.0,
          3.5, -3.5, 1024.0, 0.5, 2.0, -2.0, 7.125, 100.0]
    for nm in ("dy1", "dy2"):
        data[nm] = _place(n, cycle, dy if nm == "dy1" else dy[::-1],
                          lambda: rng.randint(-(1 << 23), 1 << 23) / 8.0)
        kinds[nm] = "f64"
    data["dy1_n"] = [None if (i + cycle) % 4 == 2 else v
                     for i, v in enumerate(data["dy1"])]
    kinds["dy1_n"] = "f64"
    data["dy32"] = [f32(v) for v in _place(
        n, cycle, dy, lambda: rng.randint(-(1 << 10), 1 << 10) / 8.0)]
    kinds["dy32"] = "f32"
    # general floats: no structure, bounded error instead of bit equality
    data["ga"] = [rng.uniform(-100, 100) for _ in range(n)]
    data["gb"] = [rng.uniform(0.1, 10) for _ in range(n)]
    data["ga_n"] = [None if rng.random() < 0.2 else v for v in data["ga"]]
    data["g32a"] = [f32(rng.uniform(-100, 100)) for _ in range(n)]
    data["g32b"] = [f32(rng.uniform(-100, 100)) for _ in range(n)]
    for nm in ("ga", "gb", "ga_n"):
        kinds[nm] = "f64"
    kinds["g32a"] = kinds["g32b"] = "f32"
    # all-null over the last tile
    data["i32_z"] = [None if i >= n - TILE else v
                     for i, v in enumerate(data["i32"])]
    kinds["i32_z"] = "i32"
    cols = [_series(nm, kinds[nm], vals) for nm, vals in data.items()]
    data["s"] = [rng.choice(["a", "b", "", "ab"]) for _ in range(n)]
    cols.append(Series.from_pylist("s", data["s"], DataType.string()))
    names = list(data)
    rows = [dict(zip(names, vs)) for vs in zip(*(data[k] for k in names))]
    return Corpus(RecordBatch(cols, n), rows)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    expr: object             # daft expression
    fn: Callable             # row dict -> value | None   (general floats:
    #                          -> (Fraction, bound Fraction) | None)
    kind: str                # bool | int | fx (bit-equal) | fg (bounded)
    dtype: DataType          # result dtype the expression layer declares
    cols: tuple = ()         # corpus columns whose edges the case must see
    big: bool = False        # int case whose inputs reach beyond +-2^53
    fused: bool = True       # the JIT planner is expected to accept it


B, I32, I64 = DataType.bool(), DataType.int32(), DataType.int64()
F32, F64 = DataType.float32(), DataType.float64()
_w64 = lambda v: wrap(v, 64, True)       # noqa: E731
_w32 = lambda v: wrap(v, 32, True)       # noqa: E731
_w8 = lambda v: wrap(v, 8, True)         # noqa: E731


def _between(x, lo, hi):
    return kleene_and(nn(lambda a, b: a >= b, x, lo),
                      nn(lambda a, b: a <= b, x, hi))


def int_cases() -> List[Case]:
    c = col
    return [
        Case("i64+1", c("i64") + 1, lambda r: _w64(r["i64"] + 1), "int",
             I64, ("i64",), big=True),
        Case("i64n-1", c("i64_n") - 1,
             lambda r: nn(lambda v: _w64(v - 1), r["i64_n"]), "int", I64,
             ("i64_n",), big=True),
        Case("i64==i64b", c("i64") == c("i64b"),
             lambda r: r["i64"] == r["i64b"], "bool", B, ("i64",)),
        Case("i64<i64b", c("i64") < c("i64b"),
             lambda r: r["i64"] < r["i64b"], "bool", B, ("i64",)),
        Case("i64n>=i64b", c("i64_n") >= c("i64b"),
             lambda r: nn(lambda a, b: a >= b, r["i64_n"], r["i64b"]),
             "bool", B, ("i64_n",)),
        Case("i64*i64b", c("i64") * c("i64b"),
             lambda r: _w64(r["i64"] * r["i64b"]), "int", I64, ("i64",),
             big=True),
        Case("i32*u32", c("i32") * c("u32"),
             lambda r: _w64(r["i32"] * r["u32"]), "int", I64,
             ("i32", "u32"), big=True),
        Case("i32*3+7", c("i32") * 3 + 7, lambda r: r["i32"] * 3 + 7,
             "int", I64, ("i32",)),
        Case("i32*i16+i8", c("i32") * c("i16") + c("i8"),
             lambda r: _w32(_w32(r["i32"] * r["i16"]) + r["i8"]), "int",
             I32, ("i32", "i16", "i8")),
        Case("i32n+i32", c("i32_n") + c("i32"),
             lambda r: nn(lambda a, b: _w32(a + b), r["i32_n"], r["i32"]),
             "int", I32, ("i32_n", "i32")),
        Case("u32+i32", c("u32") + c("i32"),
             lambda r: r["u32"] + r["i32"], "int", I64, ("u32", "i32")),
        Case("u8-i8", c("u8") - c("i8"),
             lambda r: wrap(r["u8"] - r["i8"], 16, True), "int",
             DataType.int16(), ("u8", "i8"), fused=False),
        Case("i8+i8", c("i8") + c("i8_n"),
             lambda r: nn(lambda a, b: _w8(a + b), r["i8"], r["i8_n"]),
             "int", DataType.int8(), ("i8", "i8_n"), fused=False),
        Case("(i8+i8)>100", (c("i8") + c("i8")) > 100,
             lambda r: _w8(2 * r["i8"]) > 100, "bool", B, ("i8",)),
        Case("i16/i8", c("i16") / c("i8"),
             lambda r: fop("/", i2f(r["i16"]), i2f(r["i8"])), "fx", F64,
             ("i16", "i8")),
        Case("u64>u32", c("u64") > c("u32"),
             lambda r: r["u64"] > r["u32"], "bool", B, ("u64", "u32")),
        Case("u64n==u64", c("u64_n") == c("u64"),
             lambda r: nn(lambda a, b: a == b, r["u64_n"], r["u64"]),
             "bool", B, ("u64_n", "u64")),
        Case("u64.i64+1", c("u64").cast(I64) + 1,
             lambda r: _w64(_w64(r["u64"]) + 1), "int", I64, ("u64",),
             big=True),
        Case("u64.f64", c("u64").cast(F64), lambda r: i2f(r["u64"]), "fx",
             F64, ("u64",)),
        Case("u32>i8", c("u32") > c("i8"), lambda r: r["u32"] > r["i8"],
             "bool", B, ("u32", "i8")),
        Case("u8n<i16", c("u8_n") < c("i16"),
             lambda r: nn(lambda a, b: a < b, r["u8_n"], r["i16"]), "bool",
             B, ("u8_n", "i16")),
        # casts at the root
        Case("i8.i32", c("i8").cast(I32), lambda r: r["i8"], "int", I32,
             ("i8",)),
        Case("i64.i32", c("i64").cast(I32), lambda r: _w32(r["i64"]),
             "int", I32, ("i64",)),
        Case("i16n.i64", c("i16_n").cast(I64), lambda r: r["i16_n"], "int",
             I64, ("i16_n",)),
        Case("u32.i64", c("u32").cast(I64), lambda r: r["u32"], "int", I64,
             ("u32",)),
        Case("u32.i32", c("u32").cast(I32), lambda r: _w32(r["u32"]), "int",
             I32, ("u32",)),
        Case("b.i32", c("b").cast(I32), lambda r: int(r["b"]), "int", I32),
        Case("bn.i64", c("b_n").cast(I64), lambda r: nn(int, r["b_n"]),
             "int", I64),
        Case("b.f64", c("b").cast(F64), lambda r: float(r["b"]), "fx", F64),
        Case("i64.f64", c("i64").cast(F64), lambda r: i2f(r["i64"]), "fx",
             F64, ("i64",)),
        Case("i64.f32", c("i64").cast(F32),
             lambda r: _i_to_f32(r["i64"]), "fx", F32, ("i64",)),
        Case("i32n.f32", c("i32_n").cast(F32),
             lambda r: nn(lambda v: f32(float(v)), r["i32_n"]), "fx", F32,
             ("i32_n",)),
        # narrowing casts mid-tree
        Case("i64.i8+0", c("i64").cast(DataType.int8()) + 0,
             lambda r: _w8(r["i64"]), "int", I64, ("i64",)),
        Case("i64.i32*2", c("i64").cast(I32) * 2,
             lambda r: _w32(r["i64"]) * 2, "int", I64, ("i64",)),
        Case("i32.i8==44", c("i32").cast(DataType.int8()) == 44,
             lambda r: _w8(r["i32"]) == 44, "bool", B, ("i32",)),
        Case("is_in i8n", c("i8_n").is_in([0, 1, -1]),
             lambda r: nn(lambda v: v in (0, 1, -1), r["i8_n"]), "bool", B,
             ("i8_n",)),
        Case("is_in i64", c("i64").is_in([P53 + 1, 0, -129, 7, 1 << 62]),
             lambda r: r["i64"] in (P53 + 1, 0, -129, 7, 1 << 62), "bool",
             B, ("i64",)),
        Case("between i32n", c("i32_n").between(c("i16"), c("i8_n")),
             lambda r: _between(r["i32_n"], r["i16"], r["i8_n"]), "bool", B,
             ("i32_n", "i16", "i8_n")),
        Case("between i64", c("i64").between(-129, P53),
             lambda r: -129 <= r["i64"] <= P53, "bool", B, ("i64",)),
    ]


def _i_to_f32(v: int) -> float:
    """int -> f32 in ONE rounding (through f64 would round twice)."""
    if v == 0:
        return 0.0
    q = Fraction(v)
    e = abs(v).bit_length() - 24          # ulp = 2^e for 24-bit mantissa
    if e <= 0:
        return float(v)
    m = q / (1 << e)
    r = math.floor(m)
    d = m - r
    if d > Fraction(1, 2) or (d == Fraction(1, 2) and r % 2):
        r += 1
    return float(r * (1 << e))


def logic_cases() -> List[Case]:
    c = col
    gt0 = lambda v: nn(lambda x: x > 0, v)               # noqa: E731
    le5 = lambda v: nn(lambda x: x <= 5.0, v)            # noqa: E731
    return [
        Case("and", (c("i32_n") > 0) & (c("f64_n") <= 5.0),
             lambda r: kleene_and(gt0(r["i32_n"]), le5(r["f64_n"])), "bool",
             B, ("i32_n", "f64_n")),
        Case("or", (c("i32_n") > 0) | (c("f64_n") <= 5.0),
             lambda r: kleene_or(gt0(r["i32_n"]), le5(r["f64_n"])), "bool",
             B, ("i32_n", "f64_n")),
        Case("and nonnull", (c("i32") > 0) & (c("f64") <= 5.0),
             lambda r: r["i32"] > 0 and r["f64"] <= 5.0, "bool", B,
             ("i32", "f64")),
        Case("or mixed", c("b_n") | (c("i8") > 0),
             lambda r: kleene_or(r["b_n"], r["i8"] > 0), "bool", B,
             ("i8",)),
        Case("and cols", c("b") & c("b_n"),
             lambda r: kleene_and(r["b"], r["b_n"]), "bool", B),
        Case("not", ~(c("i32_n") > 0), lambda r: knot(gt0(r["i32_n"])),
             "bool", B, ("i32_n",)),
        Case("not col", ~c("b"), lambda r: not r["b"], "bool", B),
        Case("ne", c("i16_n") != c("i8"),
             lambda r: nn(lambda a, b: a != b, r["i16_n"], r["i8"]), "bool",
             B, ("i16_n", "i8")),
        Case("le", c("i16") <= c("i8_n"),
             lambda r: nn(lambda a, b: a <= b, r["i16"], r["i8_n"]), "bool",
             B, ("i16", "i8_n")),
        Case("is_null", c("f64_n").is_null(), lambda r: r["f64_n"] is None,
             "bool", B),
        Case("not_null", c("i64_n").not_null(),
             lambda r: r["i64_n"] is not None, "bool", B),
        Case("is_null expr", (c("i32_n") + c("i16_n")).is_null(),
             lambda r: r["i32_n"] is None or r["i16_n"] is None, "bool", B),
        Case("is_null nonnull", c("i32").is_null() | (c("i32") > 0),
             lambda r: r["i32"] > 0, "bool", B, ("i32",)),
        Case("not_null nonnull", c("i32").not_null() & (c("i32") > 0),
             lambda r: r["i32"] > 0, "bool", B, ("i32",)),
        Case("z>0", c("i32_z") > 0, lambda r: gt0(r["i32_z"]), "bool", B),
        Case("z fill", c("i32_z").fill_null(-5),
             lambda r: -5 if r["i32_z"] is None else r["i32_z"], "int", I64),
        Case("fill lit", c("i32_n").fill_null(lit(-1)),
             lambda r: -1 if r["i32_n"] is None else r["i32_n"], "int", I64,
             ("i32_n",)),
        Case("fill nullable", c("i32_n").fill_null(c("i16_n")),
             lambda r: r["i16_n"] if r["i32_n"] is None else r["i32_n"],
             "int", I32, ("i32_n", "i16_n")),
        Case("fill nonnull", c("i32").fill_null(c("i16_n")),
             lambda r: r["i32"], "int", I32, ("i32",)),
        Case("if_else", c("b").if_else(c("i32"), c("i16_n")),
             lambda r: r["i32"] if r["b"] else r["i16_n"], "int", I32,
             ("i32", "i16_n")),
        # a NULL predicate takes the falsy branch (pinned behaviour)
        Case("if_else null pred", c("b_n").if_else(c("i32"), c("i16_n")),
             lambda r: r["i32"] if r["b_n"] else r["i16_n"], "int", I32,
             ("i32", "i16_n")),
        Case("if_else expr pred",
             (c("i32_n") > 0).if_else(c("i64"), c("i8")),
             lambda r: r["i64"] if gt0(r["i32_n"]) else r["i8"], "int", I64,
             ("i64", "i8"), big=True),
    ]


def float_cases() -> List[Case]:
    """Bit-equal float cases: single operations (correctly rounded, so
    contraction cannot apply) and dyadic inputs (every intermediate
    exact)."""
    c = col
    inf, nan = math.inf, math.nan
    prod = lambda r: fop("*", r["dy1"], r["dy2"])        # noqa: E731
    return [
        Case("dy+", c("dy1") + c("dy2"),
             lambda r: fop("+", r["dy1"], r["dy2"]), "fx", F64),
        Case("dy-", c("dy1_n") - c("dy2"),
             lambda r: nn(lambda a, b: fop("-", a, b), r["dy1_n"],
                          r["dy2"]), "fx", F64),
        Case("dy*", c("dy1") * c("dy2"), prod, "fx", F64),
        Case("dy/8", c("dy1") / 8, lambda r: fop("/", r["dy1"], 8.0), "fx",
             F64),
        Case("dy/dy", c("dy1") / c("dy2"),
             lambda r: fop("/", r["dy1"], r["dy2"]), "fx", F64),
        # shared subtree dy1*dy2 (JIT CSE)
        Case("cse a", c("dy1") * c("dy2") + c("dy1"),
             lambda r: fop("+", prod(r), r["dy1"]), "fx", F64),
        Case("cse b", c("dy1") * c("dy2") - c("dy2"),
             lambda r: fop("-", prod(r), r["dy2"]), "fx", F64),
        Case("dy32*dy32", c("dy32") * c("dy32") + c("dy32"),
             lambda r: fop32("+", fop32("*", r["dy32"], r["dy32"]),
                             r["dy32"]), "fx", F32),
        Case("dy32*i8", c("dy32") * c("i8"),
             lambda r: fop32("*", r["dy32"], float(r["i8"])), "fx", F32,
             ("i8",)),
        Case("f64*2", c("f64") * 2, lambda r: fop("*", r["f64"], 2.0), "fx",
             F64, ("f64",)),
        Case("f64n+1", c("f64_n") + 1,
             lambda r: nn(lambda v: fop("+", v, 1.0), r["f64_n"]), "fx",
             F64, ("f64_n",)),
        Case("f32*f32", c("f32") * c("f32_n"),
             lambda r: nn(lambda a, b: fop32("*", a, b), r["f32"],
                          r["f32_n"]), "fx", F32, ("f32", "f32_n")),
        Case("f32.f64", c("f32").cast(F64), lambda r: r["f32"], "fx", F64,
             ("f32",)),
        Case("f64.f32", c("f64").cast(F32), lambda r: f32(r["f64"]), "fx",
             F32, ("f64",)),
        # f32 * int64 literal runs in Float64 (supertype of f32 and i64)
        Case("f64.f32*3", c("f64").cast(F32) * 3,
             lambda r: fop("*", f32(r["f64"]), 3.0), "fx", F64, ("f64",)),
        Case("f32+i32", c("f32") + c("i32"),
             lambda r: fop("+", r["f32"], float(r["i32"])), "fx", F64,
             ("f32", "i32")),
        Case("f64>0.1", c("f64") > 0.1, lambda r: r["f64"] > 0.1, "bool", B,
             ("f64",)),
        Case("f64n==f64", c("f64_n") == c("f64"),
             lambda r: nn(lambda a, b: a == b, r["f64_n"], r["f64"]),
             "bool", B, ("f64_n", "f64")),
        Case("f32<f64", c("f32") < c("f64"), lambda r: r["f32"] < r["f64"],
             "bool", B, ("f32", "f64")),
        Case("f32>=i16", c("f32") >= c("i16"),
             lambda r: r["f32"] >= float(r["i16"]), "bool", B,
             ("f32", "i16")),
        Case("i64==f64", c("i64") == c("f64"),
             lambda r: i2f(r["i64"]) == r["f64"], "bool", B,
             ("i64", "f64")),
        Case("f64<inf", c("f64") < lit(inf), lambda r: r["f64"] < inf,
             "bool", B, ("f64",)),
        Case("f64>-inf", c("f64_n") > lit(-inf),
             lambda r: nn(lambda v: v > -inf, r["f64_n"]), "bool", B,
             ("f64_n",)),
        Case("nan lit", ~(c("f64") == lit(nan)) & (c("f64") > 0),
             lambda r: r["f64"] > 0, "bool", B, ("f64",)),
        Case("sel nan", (c("f64") > 0).if_else(c("f64"), lit(nan)),
             lambda r: r["f64"] if r["f64"] > 0 else nan, "fx", F64,
             ("f64",)),
        Case("fill inf", c("f64_n").fill_null(lit(inf)),
             lambda r: inf if r["f64_n"] is None else r["f64_n"], "fx", F64,
             ("f64_n",)),
        Case("is_in f64", c("f64").is_in([0.1, 1e300, 0.0]),
             lambda r: r["f64"] in (0.1, 1e300, 0.0), "bool", B, ("f64",)),
        Case("between f64", c("f64_n").between(0.1, 2.5),
             lambda r: nn(lambda v: 0.1 <= v <= 2.5, r["f64_n"]), "bool", B,
             ("f64_n",)),
    ]


def _bounded(ops: int, eps: Fraction, value: Fraction, inter: list):
    return value, ops * eps * sum(abs(x) for x in inter)


_E53, _E24 = Fraction(1, 1 << 53), Fraction(1, 1 << 24)


def general_cases() -> List[Case]:
    """Unstructured floats: the reference is the exact Fraction result and
    the bound is ops * 2^-53 * sum|intermediate| (2^-24 for Float32),
    derived from the oracle per row."""
    c = col
    F = Fraction

    def q1(r):
        a, b = F(r["ga"]), F(r["gb"])
        return _bounded(2, _E53, a * (1 - b), [1 - b, a * (1 - b)])

    def q2(r):
        a, b, i = F(r["ga"]), F(r["gb"]), r["i8"]
        m = b * F(2.5)
        return _bounded(3, _E53, a + m - i, [m, a + m, a + m - i])

    def q3(r):
        if r["ga_n"] is None:
            return None
        a, b = F(r["ga_n"]), F(r["gb"])
        return _bounded(3, _E53, (a * b + a) / b,
                        [a * b, a * b + a, (a * b + a) / b])

    def q4(r):
        a, b = F(r["g32a"]), F(r["g32b"])
        return _bounded(2, _E24, a * b + a, [a * b, a * b + a])

    return [
        Case("a*(1-b)", c("ga") * (lit(1) - c("gb")), q1, "fg", F64),
        Case("a+b*2.5-i", c("ga") + c("gb") * 2.5 - c("i8"), q2, "fg", F64),
        Case("(a*b+a)/b", (c("ga_n") * c("gb") + c("ga_n")) / c("gb"), q3,
             "fg", F64),
        Case("f32 a*b+a", c("g32a") * c("g32b") + c("g32a"), q4, "fg", F32),
    ]


def decimal_cases() -> List[Case]:
    c = col
    d3 = lambda r, k="dec3": nn(lambda v: dec_f64(v, 2), r[k])   # noqa: E731
    d12 = lambda r: dec_f64(r["dec12"], 4)               # noqa: E731
    d18 = lambda r, k="dec18": nn(lambda v: dec_f64(v, 6), r[k])  # noqa: E731
    cmp_ = lambda f: (lambda *a: nn(f, *a))              # noqa: E731
    return [
        Case("dec3==0.35", c("dec3") == 0.35, lambda r: d3(r) == 0.35,
             "bool", B, ("dec3",)),
        Case("dec3>0.57", c("dec3") > 0.57, lambda r: d3(r) > 0.57, "bool",
             B, ("dec3",)),
        Case("dec3<0.69", c("dec3") < 0.69, lambda r: d3(r) < 0.69, "bool",
             B, ("dec3",)),
        Case("dec3n==0.07", c("dec3_n") == 0.07,
             lambda r: cmp_(lambda v: v == 0.07)(d3(r, "dec3_n")), "bool",
             B, ("dec3_n",)),
        Case("dec3 between", c("dec3").between(0.05, 0.07),
             lambda r: 0.05 <= d3(r) <= 0.07, "bool", B, ("dec3",)),
        Case("dec3n between", c("dec3_n").between(0.05, 0.07),
             lambda r: cmp_(lambda v: 0.05 <= v <= 0.07)(d3(r, "dec3_n")),
             "bool", B, ("dec3_n",)),
        Case("dec12>=", c("dec12") >= 1234.5678,
             lambda r: d12(r) >= 1234.5678, "bool", B, ("dec12",)),
        Case("dec12==", c("dec12") == 0.0057, lambda r: d12(r) == 0.0057,
             "bool", B, ("dec12",)),
        Case("dec18<", c("dec18") < 0.000007, lambda r: d18(r) < 0.000007,
             "bool", B, ("dec18",)),
        Case("dec18n==7", c("dec18_n") == 7.0,
             lambda r: cmp_(lambda v: v == 7.0)(d18(r, "dec18_n")), "bool",
             B, ("dec18_n",)),
        Case("dec3*2.0", c("dec3") * 2.0, lambda r: fop("*", d3(r), 2.0),
             "fx", F64, ("dec3",)),
        Case("dec18/f", c("dec18") / c("dy2"),
             lambda r: fop("/", d18(r), r["dy2"]), "fx", F64, ("dec18",)),
        Case("dec3.f64", c("dec3_n").cast(F64), lambda r: d3(r, "dec3_n"),
             "fx", F64, ("dec3_n",)),
        Case("dec3 is_null", c("dec3_n").is_null(),
             lambda r: r["dec3_n"] is None, "bool", B),
    ]


def temporal_cases() -> List[Case]:
    c = col
    ns_t = DataType.timestamp("ns")
    d1 = (dt.date(1995, 1, 1) - dt.date(1970, 1, 1)).days
    return [
        Case("d>=lit", c("d") >= lit(LIT_DATE), lambda r: r["d"] >= D0,
             "bool", B, ("d",)),
        Case("dn<lit", c("d_n") < lit(LIT_DATE),
             lambda r: nn(lambda v: v < D0, r["d_n"]), "bool", B,
             ("d_n",)),
        Case("d between", c("d").between(lit(LIT_DATE),
                                         lit(dt.date(1995, 1, 1))),
             lambda r: D0 <= r["d"] <= d1, "bool", B, ("d",)),
        Case("d==d_n", c("d") == c("d_n"),
             lambda r: nn(lambda a, b: a == b, r["d"], r["d_n"]), "bool", B,
             ("d", "d_n")),
        Case("d-lit", c("d") - lit(LIT_DATE),
             lambda r: (r["d"] - D0) * 86_400_000_000, "int",
             DataType.duration("us"), ("d",)),
        # literal with a nonzero microsecond field (issue item 5)
        Case("tus>lit", c("tus") > lit(LIT_US), lambda r: r["tus"] > US0,
             "bool", B, ("tus",)),
        Case("tusn==lit", c("tus_n") == lit(LIT_US),
             lambda r: nn(lambda v: v == US0, r["tus_n"]), "bool", B,
             ("tus_n",)),
        # timezone-aware literal: compared at its UTC instant
        Case("tus<=tz", c("tus") <= lit(LIT_TZ), lambda r: r["tus"] <= TZ0,
             "bool", B, ("tus",)),
        Case("tns==tnsb", c("tns") == c("tnsb"),
             lambda r: r["tns"] == r["tnsb"], "bool", B, ("tns",)),
        Case("tnsn<tnsb", c("tns_n") < c("tnsb"),
             lambda r: nn(lambda a, b: a < b, r["tns_n"], r["tnsb"]),
             "bool", B, ("tns_n",)),
        Case("tns>=lit", c("tns") >= lit(LIT_NS, ns_t),
             lambda r: r["tns"] >= NS0, "bool", B, ("tns",)),
        Case("tns-tnsb", c("tns") - c("tnsb"),
             lambda r: _w64(r["tns"] - r["tnsb"]), "int",
             DataType.duration("ns"), ("tns",)),
        Case("d.i32", c("d").cast(I32), lambda r: r["d"], "int", I32,
             ("d",)),
        Case("dn.i64", c("d_n").cast(I64), lambda r: r["d_n"], "int", I64,
             ("d_n",)),
        Case("tus.i64", c("tus").cast(I64), lambda r: r["tus"], "int", I64,
             ("tus",), big=True),
        Case("tns.i64+1", c("tns").cast(I64) + 1,
             lambda r: _w64(r["tns"] + 1), "int", I64, ("tns",), big=True),
        Case("tns.i32", c("tns_n").cast(I32),
             lambda r: nn(_w32, r["tns_n"]), "int", I32, ("tns_n",)),
    ]


def mixed_cases() -> List[Case]:
    """Fusable and unfusable expressions in one list: the string
    expression bails between two fusable ones (rollback paths)."""
    c = col
    return [
        Case("pre", c("i32") + c("i16"),
             lambda r: _w32(r["i32"] + r["i16"]), "int", I32,
             ("i32", "i16")),
        Case("str", c("s") == "a", lambda r: r["s"] == "a", "bool", B,
             fused=False),
        Case("post", c("i32") * c("i8_n"),
             lambda r: nn(lambda a, b: _w32(a * b), r["i32"], r["i8_n"]),
             "int", I32, ("i32", "i8_n")),
        Case("bare col", c("i64"), lambda r: r["i64"], "int", I64,
             fused=False),
        Case("dec out", c("dec3") + c("dec3"), lambda r: 2 * r["dec3"],
             "int", DataType.decimal128(4, 2), fused=False),
        Case("post2", c("u8") + c("i32_n"),
             lambda r: nn(lambda a, b: _w32(a + b), r["u8"], r["i32_n"]),
             "int", I32, ("u8", "i32_n")),
    ]


@functools.lru_cache(maxsize=1)
def case_lists() -> dict:
    """A handful of lists per type family: one kernel (one hipRTC
    compile) per list, not per case."""
    return {"int": int_cases(), "logic": logic_cases(),
            "float": float_cases(), "general": general_cases(),
            "decimal": decimal_cases(), "temporal": temporal_cases(),
            "mixed": mixed_cases()}


def nodes(cases: List[Case]) -> list:
    return resolve_exprs([c.expr for c in cases])


@functools.lru_cache(maxsize=64)
def expected(family: str, n: int, cycle: int = 0) -> list:
    """Oracle results, computed once per (list, corpus) and shared."""
    rows = corpus(n, cycle).rows
    return [[c.fn(r) for r in rows] for c in case_lists()[family]]


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------

def _bits(v: float, single: bool) -> bytes:
    return struct.pack("<f" if single else "<d", v)


def raw_values(s: Series):
    """(values, validity) as Python lists straight from the buffers: no
    logical conversion, every row."""
    s = s.cpu() if hasattr(s, "cpu") else s
    n = len(s)
    data = s.data.numpy().tolist()
    valid = [True] * n if s.validity is None else s.validity.tolist()
    if len(data) == 1 and n > 1:
        data, valid = data * n, valid * n
    return data, valid


def check(case: Case, got: Series, want: list, tag: str = ""):
    """Every row of a result Series against the oracle."""
    assert got.dtype == case.dtype, \
        f"{tag} case {case.name!r}: dtype {got.dtype!r}"
    data, valid = raw_values(got)
    check_values(case, data, valid, want, tag)


def check_values(case: Case, data: list, valid: list, want: list,
                 tag: str = ""):
    """Every row: validity, then the value (exact, bit-equal or within the
    oracle's bound, by case kind)."""
    where = f"{tag} case {case.name!r}"
    assert len(data) == len(valid) == len(want), f"{where}: {len(data)} rows"
    single = case.dtype.kind.value == "float32"
    bad = []
    for i, (x, ok, y) in enumerate(zip(data, valid, want)):
        if y is None or not ok:
            if (y is None) != (not ok):
                bad.append((i, x if ok else None, y))
            continue
        if case.kind == "bool":
            good = bool(x) is y
        elif case.kind == "int":
            good = int(x) == y
        elif case.kind == "fx":
            good = (x != x and y != y) or \
                _bits(x, single) == _bits(y, single)
        else:
            ref, bound = y
            good = math.isfinite(x) and abs(Fraction(x) - ref) <= bound
            y = (float(ref), float(bound))
        if not good:
            bad.append((i, x, y))
    assert not bad, f"{where}: {len(bad)} rows differ, first (row, got, " \
                    f"want) {bad[:5]}"


# ---------------------------------------------------------------------------
# host walker for the postfix program (mirrors csrc/fusedexpr.hip)
# ---------------------------------------------------------------------------

def _cast(v: float, code: int) -> float:
    if code == 1:
        return f32(v)
    if code == 9:
        return 1.0 if v != 0.0 else 0.0
    if not math.isfinite(v):
        return v                 # never an integer lane; leave as is
    bits, signed = {3: (32, True), 4: (16, True), 5: (8, True),
                    6: (8, False), 7: (32, False), 10: (16, False)}[code]
    return float(wrap(int(v), bits, signed))


def _fdiv(a: float, b: float) -> float:
    if b == 0.0 and a == a and a != 0.0 and math.isfinite(a):
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    if b == 0.0:
        return math.nan if math.isfinite(a) or a != a else \
            a * math.copysign(1.0, b)
    return a / b


def walk_program(ins: list, lits: list, cols: list, scales: list,
                 n_out: int, n: int) -> list:
    """Run the postfix program on the host with `float`, opcode by opcode
    as the kernel does.  cols[k] is a list of raw values or None.  Returns
    per output a list of (value, valid)."""
    from daft_amd.kernels import fused as fz
    outs = [[None] * n for _ in range(n_out)]
    arith = {fz.OP_ADD: lambda a, b: a + b, fz.OP_SUB: lambda a, b: a - b,
             fz.OP_MUL: lambda a, b: a * b, fz.OP_DIV: _fdiv,
             fz.OP_EQ: lambda a, b: float(a == b),
             fz.OP_NE: lambda a, b: float(a != b),
             fz.OP_LT: lambda a, b: float(a < b),
             fz.OP_LE: lambda a, b: float(a <= b),
             fz.OP_GT: lambda a, b: float(a > b),
             fz.OP_GE: lambda a, b: float(a >= b)}
    for i in range(n):
        st = []
        for op, arg in ins:
            if op == fz.OP_COL:
                v = cols[arg][i]
                st.append((0.0, False) if v is None
                          else (_fdiv(float(v), scales[arg]), True))
            elif op == fz.OP_LIT:
                st.append((lits[arg], True))
            elif op in arith:
                (b, bv), (a, av) = st.pop(), st.pop()
                st.append((arith[op](a, b), av and bv))
            elif op in (fz.OP_AND, fz.OP_OR):
                (b, bv), (a, av) = st.pop(), st.pop()
                a, b = a != 0.0, b != 0.0
                if op == fz.OP_AND:
                    st.append((float(a and b), (av and bv) or
                               (av and not a) or (bv and not b)))
                else:
                    st.append((float(a or b), (av and bv) or (av and a) or
                               (bv and b)))
            elif op == fz.OP_NOT:
                a, av = st.pop()
                st.append((0.0 if a != 0.0 else 1.0, av))
            elif op == fz.OP_CAST:
                a, av = st.pop()
                st.append((_cast(a, arg), av))
            elif op in (fz.OP_ISNULL, fz.OP_NOTNULL):
                a, av = st.pop()
                st.append((float(av == (op == fz.OP_NOTNULL)), True))
            elif op == fz.OP_FILLNULL:
                b, a = st.pop(), st.pop()
                st.append(a if a[1] else b)
            elif op == fz.OP_SELECT:
                f, t, (c, cv) = st.pop(), st.pop(), st.pop()
                st.append(t if (c != 0.0 and cv) else f)
            elif op == fz.OP_STORE:
                outs[arg][i] = st.pop()
            else:
                raise AssertionError(f"opcode {op}")
            assert len(st) <= fz._MAX_STACK
        assert not st
    return outs

"""Exact oracle and case tables for the row kernels: row hashing, grouping,
count-distinct, dense first-index, selection, modulo and sorting
(test_rowops_parity.py on the CPU path, test_gpu_rowops.py on the HIP path).
A plain helper module: no fixtures, and nothing from daft_amd.kernels.

Everything here is exact; no comparison in these tests has a tolerance.

* The hash oracle is Python-integer arithmetic modulo 2^64, written from
  the definitions in csrc/common.h and csrc/row_ops.h.
* Key equality for the grouping oracles: null == null, any NaN == any NaN,
  -0.0 == +0.0, strings by bytes.
* The sort oracle is `sorted` with a comparator over row indices.  Python's
  sort is stable, so the expected permutation is unique.
"""
from __future__ import annotations

import functools
import struct
from typing import List, Optional, Sequence

import numpy as np
import torch

from daft_amd import DataType, Series

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15          # splitmix64 increment and row-fold factor
K_NULL_HASH = 0x9E3779B97F4A7C15     # kNullHash
ROW_SEED_ADD = 0x8445D61A4E774912
CANON_NAN = 0x7FF8000000000000

# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------

# chunked kernels (radix sort, compaction) give block b the rows
# [b*chunk, (b+1)*chunk) with chunk = max(256, ceil(n / 2048)) and walk them
# in 256-row tiles: 524_288 = 2048 * 256 is the last size at which every
# block owns one whole tile, 524_289 the first with a chunk (257) that is no
# multiple of the tile
ROW_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 4099,
              524_288, 524_289, 600_001]
# where the expected value comes from the scalar Python oracle
SCALAR_ROW_COUNTS = [n for n in ROW_COUNTS if n <= 4099]
LARGE_N = 600_001
SEEDS = [0, 1, 2**63 - 1, -1]
STRING_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 64]


# ---------------------------------------------------------------------------
# hash oracle: Python integers modulo 2^64
# ---------------------------------------------------------------------------

def splitmix64(x: int) -> int:
    x = (x + GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def hash_bytes(b: bytes) -> int:
    """hash_bytes_dev: the length folded into the start value, whole 8-byte
    little-endian words, then the tail as one zero-padded word."""
    h = 0xcbf29ce484222325 ^ len(b)
    full = len(b) // 8 * 8
    for i in range(0, full, 8):
        h = splitmix64(h ^ int.from_bytes(b[i:i + 8], "little"))
    if full < len(b):
        h = splitmix64(h ^ int.from_bytes(b[full:], "little"))
    return h


def canon_f64_bits(v: float) -> int:
    if v == 0.0:
        return 0                      # -0.0 -> +0.0
    if v != v:
        return CANON_NAN
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def fold_rows(col_hashes: Sequence[Sequence[int]], n: int, seed: int) -> list:
    """row_hash over per-column cell hashes; `seed` is taken modulo 2^64."""
    out = []
    start = (seed + ROW_SEED_ADD) & M64
    for i in range(n):
        acc = start
        for h in col_hashes:
            acc = ((acc * GOLDEN) & M64) ^ splitmix64(h[i])
        out.append(acc)
    return out


def _splitmix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def hash_int64_np(values: np.ndarray, seed: int = 0) -> np.ndarray:
    """Vectorised row hash of ONE non-null int64 column (uint64 out), for
    the large shape; checked against the scalar form on its first rows."""
    start = np.uint64((seed + ROW_SEED_ADD) & M64)
    cell = _splitmix64_np(values.astype(np.int64).view(np.uint64))
    with np.errstate(over="ignore"):
        return (start * np.uint64(GOLDEN)) ^ _splitmix64_np(cell)


# ---------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------

# kind -> (numpy storage dtype, class, DataType factory)
_KINDS = {
    "int8": (np.int8, "int", DataType.int8),
    "int16": (np.int16, "int", DataType.int16),
    "int32": (np.int32, "int", DataType.int32),
    "int64": (np.int64, "int", DataType.int64),
    "uint8": (np.uint8, "int", DataType.uint8),
    "uint16": (np.uint16, "int", DataType.uint16),
    "uint32": (np.uint32, "int", DataType.uint32),
    "uint64": (np.uint64, "int", DataType.uint64),
    "bool": (np.bool_, "int", DataType.bool),
    "date": (np.int32, "int", DataType.date),
    "decimal": (np.int64, "int", lambda: DataType.decimal128(18, 2)),
    "float32": (np.float32, "float", DataType.float32),
    "float64": (np.float64, "float", DataType.float64),
    "string": (None, "bytes", DataType.string),
    "binary": (None, "bytes", DataType.binary),
    "dict": (None, "bytes", DataType.string),
}
FIXED_KINDS = [k for k, v in _KINDS.items() if v[0] is not None]
_SIGNED_VIEW = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}


class Col:
    """One test column.  `data` is the physical storage with whatever lies
    under the null rows left in: a numpy array for fixed-width kinds, a list
    of bytes for string/binary, int32 codes into `vocab` for dict.  `window`
    (lo, hi) makes to_series() build the whole column and slice it, so that
    the rows start inside the buffers."""

    def __init__(self, kind: str, data, valid: Optional[np.ndarray] = None,
                 vocab: Optional[List[bytes]] = None, window=None):
        self.kind = kind
        self.data = data
        self.valid = valid
        self.vocab = vocab
        self.window = window

    def __len__(self):
        if self.window is not None:
            return self.window[1] - self.window[0]
        return len(self.data)

    def cells(self) -> list:
        """Python values of the rows: None for null, int (unsigned kinds as
        non-negative ints, decimals as the scaled integer), float (float32
        widened to double), bytes."""
        np_dt, cls, _ = _KINDS[self.kind]
        if self.kind == "dict":
            vals = [self.vocab[c] for c in self.data.tolist()]
        elif cls == "bytes":
            vals = list(self.data)
        elif cls == "float":
            with np.errstate(invalid="ignore"):   # signalling float32 NaNs
                vals = self.data.astype(np.float64).tolist()
        else:
            vals = [int(v) for v in self.data.tolist()]
        if self.valid is not None:
            vals = [v if ok else None
                    for v, ok in zip(vals, self.valid.tolist())]
        if self.window is not None:
            vals = vals[self.window[0]:self.window[1]]
        return vals

    def width(self) -> int:
        return np.dtype(_KINDS[self.kind][0]).itemsize

    def cell_hashes(self) -> list:
        """col_value_hash of every row.  A dict column hashes as its
        strings: the user-visible hash does not depend on the encoding."""
        cls = _KINDS[self.kind][1]
        cells = self.cells()
        if cls == "bytes":
            f = hash_bytes
        elif cls == "float":
            def f(v):
                return splitmix64(canon_f64_bits(v))
        else:
            mask = (1 << (8 * self.width())) - 1   # zero-extension

            def f(v):
                return splitmix64(v & mask)
        return [K_NULL_HASH if v is None else f(v) for v in cells]


def _bytes_series(name, dtype, rows: List[bytes]) -> Series:
    lens = np.fromiter((len(b) for b in rows), dtype=np.int64,
                       count=len(rows))
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return Series(name, dtype, data=torch.from_numpy(buf),
                  offsets=torch.from_numpy(off))


def to_series(col: Col, device="cpu", name: str = "c") -> Series:
    np_dt, cls, mk = _KINDS[col.kind]
    if col.kind == "dict":
        vocab = _bytes_series("vocab", DataType.string(), col.vocab)
        s = Series.make_dict(name, vocab, torch.from_numpy(
            np.ascontiguousarray(col.data, dtype=np.int32)))
    elif cls == "bytes":
        s = _bytes_series(name, mk(), col.data)
    else:
        arr = np.ascontiguousarray(col.data)
        if np_dt in _SIGNED_VIEW:
            t = torch.from_numpy(arr.view(_SIGNED_VIEW[np_dt])).view(
                getattr(torch, col.kind))
        else:
            t = torch.from_numpy(arr)
        s = Series(name, mk(), data=t)
    if col.valid is not None:
        s = s.with_validity(torch.from_numpy(col.valid.copy()))
    if col.window is not None:
        s = s.slice(*col.window)
    return s if str(device) == "cpu" else s.to(device)


def oracle_hash(cols: Sequence[Col], seed: int) -> list:
    return fold_rows([c.cell_hashes() for c in cols], len(cols[0]), seed)


def u64_list(t: torch.Tensor) -> list:
    """int64 or uint64 tensor -> list of unsigned Python ints."""
    if t.dtype == torch.uint64:
        t = t.view(torch.int64)
    return t.cpu().numpy().view(np.uint64).tolist()


# ---------------------------------------------------------------------------
# value generators
# ---------------------------------------------------------------------------

def _f64_bits(*bits) -> np.ndarray:
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _f32_bits(*bits) -> np.ndarray:
    return np.array(bits, dtype=np.uint32).view(np.float32)


# +-0, +-inf, quiet/signalling NaNs of both signs with payloads, the
# smallest denormals, the largest finite values, and a few plain numbers
F64_SPECIALS = np.concatenate([_f64_bits(
    0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000,
    0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000,
    0x7FF8000000000001, 0xFFF0000000000001, 0x7FF4000000ABCDEF,
    0xFFFFFFFFFFFFFFFF, 0x0000000000000001, 0x8000000000000001,
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF),
    np.array([1.0, -1.0, 1.5, -2.25, 1e300, -1e-300])])
F32_SPECIALS = np.concatenate([_f32_bits(
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
    0x7FC00001, 0xFF800001, 0x7FA0BCDE, 0xFFFFFFFF, 0x00000001, 0x80000001,
    0x7F7FFFFF, 0xFF7FFFFF),
    np.array([1.0, -1.0, 1.5, -2.25, 3e38, -1e-38], dtype=np.float32)])

_CHARS = ["a", "b", "B", " ", "\0", "é", "ß", "€", "漢", "😀"]


def _int_specials(kind: str) -> np.ndarray:
    np_dt = _KINDS[kind][0]
    if kind == "bool":
        return np.array([False, True])
    if kind == "decimal":
        top = 10**18 - 1
        return np.array([0, 1, -1, top, -top, 100, -100, 12345], np.int64)
    info = np.iinfo(np_dt)
    if info.min < 0:
        vals = [0, 1, -1, info.min, info.max, info.min + 1, info.max - 1,
                -2, 2, info.max // 2]
    else:
        half = (info.max + 1) // 2      # the bit a sign extension would smear
        vals = [0, 1, info.max, info.max - 1, half, half - 1, half + 1, 2]
    return np.array(vals, dtype=np_dt)


def _random_bytes(rng, ln: int) -> bytes:
    b = bytearray(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
    if ln >= 2:                 # an embedded NUL and a byte >= 0x80
        b[rng.integers(0, ln)] = 0
        b[rng.integers(0, ln)] = 0x80 | int(rng.integers(0, 128))
    return bytes(b)


def _random_text(rng, nchars: int) -> bytes:
    return "".join(_CHARS[i] for i in
                   rng.integers(0, len(_CHARS), nchars)).encode()


def _bytes_pool(kind: str, rng) -> List[bytes]:
    """A few values with prefixes of each other and zero-padded twins."""
    if kind == "binary":
        return [b"", b"\0", b"\0\0", b"a", b"a\0", b"ab", b"\xff", b"\x80a",
                b"abcdefgh", b"abcdefgh\0", b"abcdefghi", _random_bytes(rng, 64)]
    return [b"", b"a", b"a\0", b"ab", b"b", "é".encode(), "é€".encode(),
            "漢😀".encode(), b"abcdefgh", b"abcdefghi", b"abcdefgh\0",
            _random_text(rng, 64)]


_KIND_ID = {k: i for i, k in enumerate(_KINDS)}


def gen_col(kind: str, n: int, nullable: bool, ties: bool = False,
            sliced: bool = False, salt: int = 0) -> Col:
    """`n` deterministic rows of `kind`.  The first rows walk the special
    values (rotated by n, so that the tiny sizes see different ones); the
    rest are full-range random with specials mixed in, or, with `ties`,
    draws from a pool of about a dozen values.  With `nullable` about a
    fifth of the rows is null, and the value drawn for such a row stays in
    the buffer.  `sliced` puts 3 rows in front and 2 behind the window."""
    rng = np.random.default_rng([_KIND_ID[kind], n, int(nullable),
                                 int(ties), salt])
    m = n + 5 if sliced else n
    np_dt, cls, _ = _KINDS[kind]
    vocab = None
    if kind == "dict":
        vocab = _bytes_pool("string", rng)
        order = rng.permutation(len(vocab))          # vocab is not sorted
        vocab = [vocab[i] for i in order]
        data = rng.integers(0, len(vocab), m).astype(np.int32)
        if m:
            k = min(m, len(vocab))
            data[:k] = (np.arange(k) + n) % len(vocab)
    elif cls == "bytes":
        pool = _bytes_pool(kind, rng)
        mk = _random_bytes if kind == "binary" else _random_text
        data = []
        for i in range(m):
            if ties or rng.random() < 0.15:
                data.append(pool[int(rng.integers(0, len(pool)))])
            else:
                data.append(mk(rng, STRING_LENS[(i + n) % len(STRING_LENS)]))
        if sliced and m >= 3:
            data[0], data[1], data[2] = b"x", b"", b"yz"   # odd byte start
    else:
        if cls == "float":
            sp = F64_SPECIALS if kind == "float64" else F32_SPECIALS
            rnd = (rng.standard_normal(m) *
                   10.0 ** rng.integers(-6, 7, m)).astype(np_dt)
        else:
            sp = _int_specials(kind)
            if kind == "bool":
                rnd = rng.integers(0, 2, m).astype(np.bool_)
            elif kind == "decimal":
                rnd = rng.integers(-10**18 + 1, 10**18, m, dtype=np.int64)
            else:
                info = np.iinfo(np_dt)
                rnd = rng.integers(info.min, info.max, m, dtype=np_dt,
                                   endpoint=True)
        pool = np.concatenate([sp, rnd[:4]]) if m >= 4 else sp
        picks = pool[rng.integers(0, len(pool), m)]
        data = picks if ties else np.where(rng.random(m) < 0.3, picks, rnd)
        data = np.ascontiguousarray(data, dtype=np_dt)
        k = min(m, len(sp))
        data[:k] = sp[(np.arange(k) + n) % len(sp)]
    valid = None
    if nullable:
        valid = rng.random(m) > 0.2
    window = (3, 3 + n) if sliced else None
    return Col(kind, data, valid, vocab, window)


# ---------------------------------------------------------------------------
# hash case table
# ---------------------------------------------------------------------------

# (id, kind, sliced)
HASH_COLUMNS = [(k, k, False) for k in FIXED_KINDS + ["string", "binary"]] \
    + [("string_sliced", "string", True), ("binary_sliced", "binary", True),
       ("int8_sliced", "int8", True)]
# 1-, 2- and 4-column rows of mixed kinds: (kind, nullable) per column
HASH_ROWS = {
    "i64": [("int64", False)],
    "i32n_str": [("int32", True), ("string", False)],
    "f64_i8n": [("float64", False), ("int8", True)],
    "u16_bin_f32_bool": [("uint16", True), ("binary", True),
                         ("float32", True), ("bool", False)],
}


@functools.lru_cache(maxsize=None)
def hash_col(kind: str, n: int, nullable: bool, sliced: bool = False,
             salt: int = 0) -> Col:
    return gen_col(kind, n, nullable, sliced=sliced, salt=salt)


@functools.lru_cache(maxsize=None)
def hash_row_cols(name: str, n: int) -> tuple:
    return tuple(hash_col(k, n, nullable, salt=j + 1)
                 for j, (k, nullable) in enumerate(HASH_ROWS[name]))


@functools.lru_cache(maxsize=None)
def _cell_hashes_cached(col: Col) -> tuple:
    return tuple(col.cell_hashes())


def expected_hash(cols: Sequence[Col], seed: int) -> list:
    """oracle_hash with the per-column part computed once per column."""
    return fold_rows([_cell_hashes_cached(c) for c in cols],
                     len(cols[0]), seed)


@functools.lru_cache(maxsize=None)
def large_int64() -> np.ndarray:
    rng = np.random.default_rng(600_001)
    v = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max,
                     LARGE_N, dtype=np.int64, endpoint=True)
    v[:10] = _int_specials("int64")
    return v


# ---------------------------------------------------------------------------
# key equality and the grouping oracles
# ---------------------------------------------------------------------------

def eq_key(v):
    """Hashable stand-in for a cell under grouping equality."""
    if v is None:
        return ("null",)
    if isinstance(v, float):
        if v != v:
            return ("nan",)
        return ("f", 0.0 if v == 0.0 else v)
    return ("v", v)


def key_codes(cols: Sequence[Col]) -> np.ndarray:
    """Equality class of every row, numbered by first appearance."""
    rows = zip(*[[eq_key(v) for v in c.cells()] for c in cols])
    seen = {}
    return np.fromiter((seen.setdefault(r, len(seen)) for r in rows),
                       dtype=np.int64, count=len(cols[0]))


def assert_partition(ids, reps, codes: np.ndarray):
    """`ids` are dense in [0, G), two rows share an id iff they share an
    equality class, and reps[g] is a row of group g.  Id order is free."""
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    reps = np.asarray(reps.cpu() if isinstance(reps, torch.Tensor) else reps)
    n, G = len(codes), len(reps)
    assert ids.shape == (n,)
    want_g = len(np.unique(codes))
    assert G == want_g, f"{G} groups, expected {want_g}"
    if n == 0:
        return
    assert ids.min() >= 0 and ids.max() < G
    pairs = np.unique(np.stack([ids, codes], axis=1), axis=0)
    # G distinct (id, class) pairs with G ids and G classes: a bijection
    assert len(pairs) == G
    assert len(np.unique(pairs[:, 0])) == G
    assert len(np.unique(pairs[:, 1])) == G
    assert reps.min() >= 0 and reps.max() < n
    assert np.array_equal(ids[reps], np.arange(G))


GROUP_KEY_SETS = ["float64", "float32_null", "int32_null", "string_null",
                  "two_col", "one_group", "all_distinct"]
GROUP_ROW_COUNTS = [1, 2, 32, 33, 257, 4099]   # 32 -> 33: 64 -> 128 slots


@functools.lru_cache(maxsize=None)
def group_keys(name: str, n: int) -> tuple:
    if name == "float64":
        return (gen_col("float64", n, False, ties=True),)
    if name == "float32_null":
        return (gen_col("float32", n, True, ties=True),)
    if name == "int32_null":
        return (gen_col("int32", n, True, ties=True),)
    if name == "string_null":
        return (gen_col("string", n, True, ties=True),)
    if name == "two_col":
        return (gen_col("int16", n, True, ties=True, salt=1),
                gen_col("string", n, False, ties=True, salt=2))
    if name == "one_group":
        return (Col("int64", np.full(n, -7, dtype=np.int64)),)
    if name == "all_distinct":
        v = (np.arange(n, dtype=np.int64) - n // 2) * 0x1000003
        return (Col("int64", v),)
    raise KeyError(name)


N_COLLIDE = 2000          # table_capacity(2000) == 4096
CAP_COLLIDE = 4096


@functools.lru_cache(maxsize=None)
def colliding_keys():
    """50 distinct two-column keys over 2000 rows, one class per `code`:
    a nullable int32 (code % 10; class 3 is the null, with garbage under it)
    and a string (code // 10).  Returns (cols, code)."""
    rng = np.random.default_rng(50)
    code = rng.integers(0, 50, N_COLLIDE)
    code[:50] = np.arange(50)
    a = (code % 10).astype(np.int32) * 1000 - 4000
    valid = (code % 10) != 3
    a[~valid] = rng.integers(-99, 99, int((~valid).sum()))
    names = [b"", b"a", b"a\0", "é".encode(), b"abcdefghi"]
    b = [names[c // 10] for c in code.tolist()]
    return (Col("int32", a, valid), Col("string", b)), code


def colliding_hashes(code: np.ndarray, mode: str) -> np.ndarray:
    """Caller-supplied hashes (uint64) that stay a function of the key:
    "equal" gives every key one hash; "slot" gives every key its own hash,
    all of them equal modulo the table capacity."""
    if mode == "equal":
        return np.full(len(code), 0x0123456789ABCDEF, dtype=np.uint64)
    with np.errstate(over="ignore"):
        hi = (code.astype(np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
    return (hi & ~np.uint64(CAP_COLLIDE - 1)) | np.uint64(5)


def expected_count_distinct(gids: np.ndarray, num_groups: int,
                            col: Col) -> list:
    """Distinct non-null values per group under eq_key."""
    sets = [set() for _ in range(num_groups)]
    for g, v in zip(gids.tolist(), col.cells()):
        if v is not None:
            sets[g].add(eq_key(v))
    return [len(s) for s in sets]


def expected_first_index(packed: np.ndarray, rng: int, sentinel: int):
    first = np.full(rng, sentinel, dtype=np.int64)
    np.minimum.at(first, packed, np.arange(len(packed), dtype=np.int64))
    return first


DENSE_RANGES = [1, 255, 8192, 8193, 70_000]   # LDS kernel up to 8192 slots
DENSE_ROW_COUNTS = [1, 257, LARGE_N]


@functools.lru_cache(maxsize=None)
def dense_packed(n: int, rng: int) -> np.ndarray:
    """Keys in [0, rng); key rng // 2 never occurs once rng > 2."""
    g = np.random.default_rng([n, rng])
    p = g.integers(0, rng, n)
    if rng > 2:
        p[p == rng // 2] = rng - 1
    return p


# ---------------------------------------------------------------------------
# selection masks, radix keys, modulo
# ---------------------------------------------------------------------------

MASKS = ["none", "all", "alternating", "first", "last", "one_wave",
         "random_1pct", "random_99pct"]


def mask(name: str, n: int) -> np.ndarray:
    m = np.zeros(n, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "alternating":
        m[1::2] = True
    elif name == "first":
        m[:1] = True
    elif name == "last":
        m[n - 1:] = True
    elif name == "one_wave":          # exactly one full wave, mid-column
        lo = (n // 2) // 64 * 64
        m[lo:lo + 64] = True
    elif name.startswith("random"):
        p = 0.01 if name == "random_1pct" else 0.99
        m = np.random.default_rng(n).random(n) < p
    return m


RADIX_KEYS = ["random", "all_equal", "two_valued", "four_valued", "sorted",
              "reversed", "bit63"] + [f"byte{b}" for b in range(8)]


def radix_keys(name: str, n: int) -> np.ndarray:
    """uint64 keys.  Every set but "random" has ties above one tile."""
    rng = np.random.default_rng(n + 17)
    i = np.arange(n, dtype=np.uint64)
    if name == "random":
        return rng.integers(0, M64, n, dtype=np.uint64, endpoint=True)
    if name == "all_equal":
        return np.full(n, 0xDEADBEEF00C0FFEE, dtype=np.uint64)
    if name == "two_valued":
        return np.where(rng.random(n) < 0.5, np.uint64(M64), np.uint64(0))
    if name == "four_valued":
        return rng.integers(0, 4, n).astype(np.uint64)
    if name == "sorted":
        return i // np.uint64(3)
    if name == "reversed":
        return (np.uint64(n) - i) // np.uint64(3)
    if name == "bit63":
        return (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)) \
            | np.uint64(0x00FF00FF00FF00FF)
    b = int(name[4:])
    return ((i * np.uint64(37)) % np.uint64(256)) << np.uint64(8 * b)


MOD_HASHES = [0, 1, 2, 2**31 - 1, 2**31, 2**32 + 1, 2**63 - 1, 2**63,
              2**63 + 1, 0x9E3779B97F4A7C15, 2**64 - 2, 2**64 - 1]
MOD_DIVISORS = [1, 2, 3, 7, 16, 2**31 - 1]


# ---------------------------------------------------------------------------
# sort oracle
# ---------------------------------------------------------------------------

def _cmp_values(a, b) -> int:
    """NaNs are equal to each other and greater than any number; the two
    zeros are equal; ints (unsigned kinds are non-negative here) and bytes
    compare naturally."""
    if isinstance(a, float):
        an, bn = a != a, b != b
        if an or bn:
            return int(an) - int(bn)
    return (a > b) - (a < b)


def sort_perm(cols: Sequence[Col], descending: Sequence[bool],
              nulls_first: Sequence[bool]) -> list:
    """The stable lexicographic argsort.  A null is placed first or last by
    `nulls_first` alone; `descending` reverses only the value order."""
    cells = [c.cells() for c in cols]

    def cmp(i, j):
        for vals, desc, nf in zip(cells, descending, nulls_first):
            a, b = vals[i], vals[j]
            if a is None or b is None:
                if a is None and b is None:
                    continue
                first = a is None
                return -1 if first == nf else 1
            c = _cmp_values(a, b)
            if c:
                return -c if desc else c
        return 0

    return sorted(range(len(cols[0])), key=functools.cmp_to_key(cmp))


SORT_KINDS = FIXED_KINDS + ["dict"]
SORT_FLAGS = [(d, nf) for d in (False, True) for nf in (False, True)]
TWO_KEY_SORTS = ["composed", "wide", "float_int"]


@functools.lru_cache(maxsize=None)
def sort_col(kind: str, n: int, nullable: bool, salt: int = 0) -> Col:
    return gen_col(kind, n, nullable, ties=True, salt=salt)


@functools.lru_cache(maxsize=None)
def two_key_sort(name: str, n: int) -> tuple:
    """"composed": two small-range nullable ints, which fit the single-pass
    packed key.  "wide": two nullable full-range int32 (33 + 33 bits), so
    the per-key loop runs.  "float_int": the float NaN and zero variants,
    then an int."""
    if name == "composed":
        g = np.random.default_rng([n, 5])
        a = Col("int8", g.integers(-3, 4, n).astype(np.int8),
                g.random(n) > 0.2)
        b = Col("int16", g.integers(-300, 300, n).astype(np.int16),
                g.random(n) > 0.2)
        return a, b
    if name == "wide":
        return (sort_col("int32", n, True, salt=1),
                sort_col("int32", n, True, salt=2))
    if name == "float_int":
        return (sort_col("float64", n, True, salt=1),
                sort_col("int16", n, False, salt=2))
    raise KeyError(name)

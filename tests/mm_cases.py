"""Oracles and case tables for the dedup, tokenization and image kernels:
minhash, simhash, hll_update and image_resize (csrc/multimodal.hip), BPE
encode (csrc/bpe.hip) and Levenshtein (csrc/editdist.hip).  Used by
test_mm_parity.py on the CPU paths and by test_gpu_mm.py on the HIP paths.
A plain helper module: no fixtures, and from daft_amd.functions only what
builds inputs (`_perms`, `_bytes_to_unicode`, `BPETokenizer`,
`_image_struct`).

Everything is exact (Python integers, fractions of integers, float64 numpy)
except two stated rules: the HyperLogLog estimate may differ from the
oracle's by 1 (a `.5` that two `log` implementations round apart), and a
resized pixel whose exact value lies within RESIZE_NEAR of a rounding
boundary may differ by 1, unless fp32 computes that image exactly
(resize_is_dyadic).
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from daft_amd import Series
from daft_amd.functions.image import _image_struct
from daft_amd.functions.minhash import _perms
from daft_amd.functions.tokenize import BPETokenizer, _bytes_to_unicode

from rowops_cases import (Col, M64, expected_hash, hash_bytes, to_series)

MERSENNE61 = (1 << 61) - 1
U32 = 0xFFFFFFFF

# one wave per row, 4 waves per block: 3, 4, 5 straddle a block, and 8193 is
# more than 2048 blocks x 4 waves, so the row-stride loop runs
ROW_COUNTS = [1, 3, 4, 5, 8193]


# ---------------------------------------------------------------------------
# text columns
# ---------------------------------------------------------------------------

_UNDER_NULL = b"under a null row"
LAYOUTS = ["plain", "sliced", "offset", "dict"]


def text_series(rows: Sequence[Optional[bytes]], dev, kind: str = "string",
                layout: str = "plain") -> Series:
    """A string/binary column of `rows` (None = null; bytes are left in the
    buffer under a null row).

    * plain:  offsets start at 0
    * sliced: Series.slice of a longer column: 3 rows in front, 2 behind; the
      data tensor starts at an odd byte of its storage
    * offset: the same window kept as raw offsets into the whole buffer, so
      offsets[0] != 0
    * dict:   dictionary-encoded, vocabulary in shuffled order
    """
    valid = None
    if any(r is None for r in rows):
        valid = np.array([r is not None for r in rows])
    data = [_UNDER_NULL if r is None else r for r in rows]
    if layout == "dict":
        vocab = sorted(set(data), key=lambda b: (hash_bytes(b), b))
        where = {b: i for i, b in enumerate(vocab)}
        codes = np.array([where[b] for b in data], dtype=np.int32)
        return to_series(Col("dict", codes, valid, vocab=vocab), dev)
    if layout == "plain":
        return to_series(Col(kind, data, valid), dev)
    front, back = [b"abc", b"", b"\xc3\xa9 front"], [b"back", b"b"]
    full = front + data + back
    fvalid = None
    if valid is not None:
        fvalid = np.concatenate([[True, False, True], valid, [True, True]])
    lo, hi = 3, 3 + len(data)
    if layout == "sliced":
        return to_series(Col(kind, full, fvalid, window=(lo, hi)), dev)
    assert layout == "offset"
    s = to_series(Col(kind, full, fvalid), "cpu")
    out = Series(s.name, s.dtype, data=s.data, offsets=s.offsets[lo:hi + 1],
                 validity=None if s.validity is None else s.validity[lo:hi])
    assert int(out.offsets[0]) != 0
    return out if str(dev) == "cpu" else out.to(dev)


# ---------------------------------------------------------------------------
# minhash
# ---------------------------------------------------------------------------

MINHASH_NUM_HASHES = [1, 63, 64, 65, 128, 512]
MINHASH_NGRAMS = [1, 2, 3, 16]
MINHASH_SEED = 7
# (num_hashes, ngram_size) that must raise ValueError before any launch
MINHASH_BAD_ARGS = [(513, 2), (64, 17), (64, 0), (0, 2)]


def word_spans(row: bytes) -> List[Tuple[int, int]]:
    """Words: maximal runs of bytes other than 0x20."""
    spans, start = [], None
    for i, c in enumerate(row):
        if c != 0x20 and start is None:
            start = i
        elif c == 0x20 and start is not None:
            spans.append((start, i))
            start = None
    if start is not None:
        spans.append((start, len(row)))
    return spans


def minhash_oracle(row: Optional[bytes], ngram: int, a: Sequence[int],
                   b: Sequence[int]) -> List[int]:
    """Signature of one row.  The gram of words j .. j+n-1 is the raw byte
    span from the start of word j to the end of word j+n-1."""
    spans = word_spans(row) if row is not None else []
    mins = [None] * len(a)
    for j in range(len(spans) - ngram + 1):
        h = hash_bytes(row[spans[j][0]:spans[j + ngram - 1][1]]) & MERSENNE61
        for i in range(len(a)):
            v = (a[i] * h + b[i]) % MERSENNE61
            if mins[i] is None or v < mins[i]:
                mins[i] = v
    return [U32 if v is None else v & U32 for v in mins]


def minhash_perms(num_hashes: int, seed: int = MINHASH_SEED):
    a, b = _perms(num_hashes, seed)         # inputs of the operation
    return [int(v) for v in a], [int(v) for v in b]


def expected_minhash(rows, num_hashes: int, ngram: int,
                     seed: int = MINHASH_SEED) -> np.ndarray:
    """[len(rows), num_hashes] uint32, all 0xFFFFFFFF for a null row (the
    drivers do not compare what lies under a null)."""
    a, b = minhash_perms(num_hashes, seed)
    memo: Dict[Optional[bytes], List[int]] = {}
    out = np.zeros((len(rows), num_hashes), dtype=np.uint32)
    for i, r in enumerate(rows):
        if r not in memo:
            memo[r] = minhash_oracle(r, ngram, a, b)
        out[i] = memo[r]
    return out


def _words(k: int, salt: int = 0) -> List[bytes]:
    return [b"w%d" % ((i * 7 + salt) % 23) for i in range(k)]


def _gram_of_len(n: int, total: int) -> bytes:
    """n words and n-1 single spaces, `total` bytes in all."""
    letters = total - (n - 1)
    assert letters >= n
    each, extra = divmod(letters, n)
    ws = [bytes([97 + (i % 26)]) * (each + (1 if i < extra else 0))
          for i in range(n)]
    out = b" ".join(ws)
    assert len(out) == total
    return out


@functools.lru_cache(maxsize=None)
def minhash_rows(n: int) -> tuple:
    """The row shapes for ngram_size n."""
    rows: List[Optional[bytes]] = [
        b"", b" ", b"     ",
        b" lead", b"trail ", b"  both  ", b"a  b", b"a b", b"a   b  c d",
        b"tab\tis no\nseparator here\r\nat all",
        b"\t", b"\n \n",
        None,
        b" ".join(_words(max(n - 1, 0))),
        b" ".join(_words(n)),
        b" ".join(_words(n + 1)),
        b"  ".join(_words(n + 1, 3)) + b" ",
        b"x" * 300,
        b" ".join([b"y" * 300] * n),
        "€漢😀".encode(),
        "€漢😀 é ß nbsp 漢 😀😀 a€ €漢😀".encode(),
        " ".join("é€漢😀"[i % 4] * (1 + i % 3) for i in range(n + 2)).encode(),
        None,
    ]
    if n == 16:
        # 17 and 40 words wrap the 16-entry ring of word starts
        rows += [b" ".join(_words(17)), b" ".join(_words(40, 5)),
                 b"  ".join(_words(40, 9))]
    # gram lengths around the 8-byte words of hash_bytes and its tail
    for total in (7, 8, 9, 16, 31, 32, 33, 40):
        if total >= 2 * n - 1:
            rows.append(_gram_of_len(n, total))
            rows.append(_gram_of_len(n, total) + b" " +
                        _gram_of_len(n, total)[::-1])
    return tuple(rows)


_SHORT_POOL = [b"a b c", b"", b"a  b", None, b"zz", b"q w", b" ",
               "é 漢".encode(), b"a b c d", b"one", None, b"b a", b"a b"]


def short_rows(n: int, salt: int = 0) -> list:
    return [_SHORT_POOL[(i * 5 + i // 13 + salt) % len(_SHORT_POOL)]
            for i in range(n)]


# ---------------------------------------------------------------------------
# simhash
# ---------------------------------------------------------------------------

SIMHASH_NGRAMS = [1, 4, 8, 9]
# numbers of n-grams: none, one, a tie of two, around one and two passes of
# the 64-lane wave, and many passes
SIMHASH_M = [0, 1, 2, 63, 64, 65, 128, 129, 1000]


def simhash_oracle(row: Optional[bytes], ngram: int) -> int:
    """Bit i is set iff strictly more than half of the m = len - n + 1 byte
    n-grams have bit i of hash_bytes set; m <= 0 gives 0."""
    if row is None:
        return 0
    m = len(row) - ngram + 1
    if m <= 0:
        return 0
    cnt = [0] * 64
    for j in range(m):
        h = hash_bytes(row[j:j + ngram])
        for i in range(64):
            cnt[i] += (h >> i) & 1
    return sum(1 << i for i in range(64) if 2 * cnt[i] > m)


def _ascii_text(rng, ln: int) -> bytes:
    return bytes(rng.integers(32, 127, ln, dtype=np.uint8).tolist())


@functools.lru_cache(maxsize=None)
def simhash_rows(ngram: int, kind: str) -> tuple:
    rng = np.random.default_rng([ngram, kind == "binary"])
    rows: List[Optional[bytes]] = [b"", None]
    for m in SIMHASH_M:
        ln = m + ngram - 1
        if kind == "binary":
            rows.append(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
        else:
            rows.append(_ascii_text(rng, ln))
        rows.append(b"a" * ln)                      # all n-grams equal
    rows += [None, ("€漢😀é" * 9).encode(), b"ab" * 40]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def expected_simhash(rows: tuple, ngram: int) -> tuple:
    memo: Dict[Optional[bytes], int] = {}
    for r in rows:
        if r not in memo:
            memo[r] = simhash_oracle(r, ngram)
    return tuple(memo[r] for r in rows)


# ---------------------------------------------------------------------------
# HyperLogLog
# ---------------------------------------------------------------------------

HLL_BITS = 14
HLL_REGS = 1 << HLL_BITS


def hll_slot(h: int) -> Tuple[int, int]:
    """(register index, rank) of one 64-bit hash."""
    rest = (h << HLL_BITS) & M64
    rank = 64 - HLL_BITS + 1 if rest == 0 else (64 - rest.bit_length()) + 1
    return h >> (64 - HLL_BITS), rank


def hll_registers(hashes, gids=None, valid=None,
                  num_groups: int = 1) -> np.ndarray:
    """[num_groups, 16384] registers: the per-group maximum rank."""
    regs = np.zeros((num_groups, HLL_REGS), dtype=np.int64)
    for i, h in enumerate(hashes):
        if valid is not None and not valid[i]:
            continue
        idx, rank = hll_slot(int(h))
        g = 0 if gids is None else int(gids[i])
        if rank > regs[g, idx]:
            regs[g, idx] = rank
    return regs


def hll_registers_np(hashes: np.ndarray, gids=None, valid=None,
                     num_groups: int = 1) -> np.ndarray:
    """hll_registers for the large shape; checked against the scalar form."""
    h = hashes.astype(np.uint64)
    idx = (h >> np.uint64(64 - HLL_BITS)).astype(np.int64)
    x = h << np.uint64(HLL_BITS)
    zero = x == 0
    bits = np.zeros(len(h), dtype=np.int64)         # bit_length by halving
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> np.uint64(s)) != 0
        bits += np.where(big, s, 0)
        x = np.where(big, x >> np.uint64(s), x)
    bits += (x != 0)
    rank = np.where(zero, 64 - HLL_BITS + 1, 64 - bits + 1)
    g = np.zeros(len(h), dtype=np.int64) if gids is None else gids
    keep = np.ones(len(h), dtype=bool) if valid is None else valid
    regs = np.zeros(num_groups * HLL_REGS, dtype=np.int64)
    np.maximum.at(regs, (g * HLL_REGS + idx)[keep], rank[keep])
    return regs.reshape(num_groups, HLL_REGS)


def hll_estimate(regs: Sequence[int]) -> float:
    """The textbook estimator (Flajolet et al. 2007) for m = 2^14 registers,
    with linear counting in the small range."""
    m = float(HLL_REGS)
    alpha = 0.7213 / (1.0 + 1.079 / m)
    est = alpha * m * m / math.fsum(2.0 ** -int(r) for r in regs)
    zeros = sum(1 for r in regs if r == 0)
    if est < 2.5 * m and zeros > 0:
        est = m * math.log(m / zeros)
    return est


def round_half_up_int(x: float) -> int:
    return math.floor(x + 0.5)


HLL_4SIGMA = 4 * 1.04 / math.sqrt(HLL_REGS)      # about 3.3 %


def _raw(hashes, gids=None, valid=None, groups=1):
    return (np.array(hashes, dtype=np.uint64),
            None if gids is None else np.array(gids, dtype=np.int64),
            None if valid is None else np.array(valid, dtype=bool), groups)


def _hll_large(n: int):
    rng = np.random.default_rng(n)
    h = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    h[::7] &= np.uint64((1 << 56) - 1)     # few registers, so maxima compete
    gids = rng.integers(0, 3, n).astype(np.int64)
    valid = rng.random(n) < 0.9
    return h, gids, valid, 3


# name -> (hashes, gids, valid, num_groups); None is passed as an empty tensor
HLL_RAW: Dict[str, tuple] = {
    "zero": _raw([0]),
    "all_ones": _raw([M64]),
    "idx_edges": _raw([v for idx in (0, 1, 16383)
                       for v in (idx << 50, (idx << 50) | 1)]),
    "idx_edges_low_bit_only": _raw([(idx << 50) | 1
                                    for idx in (0, 1, 16383)]),
    "bit49": _raw([1 << 49]),
    "equal_run": _raw([0x0123456789ABCDEF] * 300),
    # group 1 is empty; group 0 writes its last register and group 2 its
    # first, so a register block that bleeds into its neighbour shows
    "three_groups": _raw([(16383 << 50) | (1 << 40), 1 << 30,
                          (16383 << 50) | 1],
                         gids=[0, 2, 0], groups=3),
    # the masked row would win both registers
    "valid_masks_largest": _raw([5 << 50, (5 << 50) | (1 << 49),
                                 (5 << 50) | (1 << 20), 9 << 50, 9 << 50 | 7],
                                gids=[0, 0, 0, 1, 1],
                                valid=[False, True, True, False, True],
                                groups=2),
    "no_gids_no_valid_257": _raw(
        np.random.default_rng(257).integers(0, 1 << 64, 257,
                                            dtype=np.uint64)),
    "one_row_grouped": _raw([(77 << 50) | (1 << 10)], gids=[1], valid=[True],
                            groups=2),
    "n257": _hll_large(257),
    "n600001": _hll_large(600_001),
}

# distinct counts: nothing, one, small, the old test's size, either side of
# the switch to the raw estimate at 2.5 * m = 40 960, and large
HLL_DISTINCT = [0, 1, 100, 5000, 39_000, 41_000, 43_000, 200_000]


class HllColumn:
    """One column for approx_count_distinct: `col` for to_series and
    expected_hash, `true` distinct valid values per group, `gids`."""

    def __init__(self, col: Col, gids: Optional[np.ndarray], groups: int):
        self.col = col
        self.gids = gids
        self.groups = groups

    @functools.cached_property
    def registers(self) -> np.ndarray:
        h = np.array(expected_hash([self.col], 0), dtype=np.uint64)
        return hll_registers_np(h, self.gids, self.col.valid, self.groups)

    @functools.cached_property
    def estimates(self) -> List[float]:
        return [hll_estimate(r) for r in self.registers.tolist()]

    @functools.cached_property
    def true(self) -> List[int]:
        sets = [set() for _ in range(self.groups)]
        for i, v in enumerate(self.col.cells()):
            if v is not None:
                sets[0 if self.gids is None else int(self.gids[i])].add(v)
        return [len(s) for s in sets]


def _distinct_values(kind: str, d: int, rng) -> list:
    if kind == "string":
        return [b"key-%d-\xe2\x82\xac" % i for i in range(d)]
    v = np.unique(rng.integers(np.iinfo(np.int64).min,
                               np.iinfo(np.int64).max, d + 64))
    assert len(v) >= d
    return rng.permutation(v)[:d].tolist()


@functools.lru_cache(maxsize=None)
def hll_column(kind: str, distinct: int, nullable: bool = False) -> HllColumn:
    """`distinct` different values, each at least once, plus repeats, in
    shuffled order.  With `nullable` a fifth of the rows is null and hides
    values that occur nowhere else.  distinct = 0 gives an empty column, or
    an all-null one."""
    rng = np.random.default_rng([distinct, kind == "string", int(nullable)])
    vals = _distinct_values(kind, distinct, rng)
    n = distinct + min(distinct, 3000)
    pick = np.concatenate([np.arange(distinct),
                           rng.integers(0, max(distinct, 1),
                                        n - distinct)]).astype(np.int64)
    pick = rng.permutation(pick)
    rows = [vals[i] for i in pick]
    valid = None
    if nullable:
        k = max(n // 5, 3)
        hidden = [b"hidden-%d" % i if kind == "string" else 10**15 + i
                  for i in range(k)]
        at = np.sort(rng.choice(n + k, k, replace=False))
        valid = np.ones(n + k, dtype=bool)
        valid[at] = False
        it, ih = iter(rows), iter(hidden)
        rows = [next(it) if ok else next(ih) for ok in valid]
    data = rows if kind == "string" else np.array(rows, dtype=np.int64)
    return HllColumn(Col(kind, data, valid), None, 1)


@functools.lru_cache(maxsize=None)
def hll_grouped(kind: str) -> HllColumn:
    """Groups 0..3 interleaved: 100 distinct, 5000 distinct, all null, and 1
    distinct value repeated."""
    rng = np.random.default_rng([99, kind == "string"])
    parts = [hll_column(kind, 100, True).col, hll_column(kind, 5000).col]
    rows, valid, gids = [], [], []
    for g, c in enumerate(parts):
        data = list(c.data) if kind == "string" else c.data.tolist()
        rows += data
        valid += [True] * len(data) if c.valid is None else c.valid.tolist()
        gids += [g] * len(data)
    null_vals = _distinct_values(kind, 50, rng)
    rows += null_vals
    valid += [False] * 50
    gids += [2] * 50
    rows += [rows[0]] * 40
    valid += [True] * 40
    gids += [3] * 40
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    data = rows if kind == "string" else np.array(rows, dtype=np.int64)
    return HllColumn(Col(kind, data, np.array(valid)[order]),
                     np.array(gids, dtype=np.int64)[order], 4)


# ---------------------------------------------------------------------------
# BPE
# ---------------------------------------------------------------------------

BPE_MAX_LEN = 4096            # longer rows take the host fallback
BPE_LENS = [0, 1, 2, 63, 64, 65, 66, 128, 129, 130,
            4095, 4096, 4097, 5000]
_B2U = _bytes_to_unicode()


def _u(tok: bytes) -> str:
    return "".join(_B2U[c] for c in tok)


class BpeTable:
    """A merge table in two forms: `tokenizer` for the code under test, and
    `ranks` {(left bytes, right bytes): rank} with `ids` {bytes: id} for the
    oracle."""

    def __init__(self, merges: List[Tuple[bytes, bytes]]):
        assert len(set(merges)) == len(merges)
        self.ids = {bytes([b]): b for b in range(256)}
        todo = list(merges)     # ids in order of construction, not of rank
        while todo:
            ready = [(l, r) for l, r in todo
                     if l in self.ids and r in self.ids]
            assert ready
            for l, r in ready:
                assert l + r not in self.ids
                self.ids[l + r] = len(self.ids)
            todo = [m for m in todo if m not in ready]
        self._memo: Dict[bytes, tuple] = {}
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.tokenizer = BPETokenizer(
            {_u(t): i for t, i in self.ids.items()},
            [(_u(l), _u(r)) for l, r in merges])

    def encode(self, text: bytes) -> List[int]:
        """Byte-string tokens; merge the pair of lowest rank, the leftmost
        one on ties, until no adjacent pair has a rank; ids at the end."""
        toks = [text[i:i + 1] for i in range(len(text))]
        while True:
            best = None
            for i in range(len(toks) - 1):
                r = self.ranks.get((toks[i], toks[i + 1]))
                if r is not None and (best is None or r < best[0]):
                    best = (r, i)
            if best is None:
                return [self.ids[t] for t in toks]
            i = best[1]
            toks = toks[:i] + [toks[i] + toks[i + 1]] + toks[i + 2:]


_HOT = [b"a", b"b", b" ", b"\x00", b"\xff", b"\xe2", b"\x82", b"\xac",
        b"\xe6", b"\xbc", b"\xa2", b"\xf0", b"\x9f", b"\x98", b"\x80",
        b"\xc3", b"\xa9"]                       # bytes of "ab \0", 0xFF, "€漢😀é"
BPE_RANDOM_MERGES = 3000
# a seed at which one key of the device hash table wraps from the last
# slot to the first (test_mm_parity.py asserts it)
BPE_RANDOM_SEED = 23


def _random_merges(seed: int) -> List[Tuple[bytes, bytes]]:
    """Merges over all 256 byte symbols.  They alternate between two kinds:
    a pair that stands side by side in a sample text over the hot bytes,
    merged there at once as a BPE trainer would, so that text over those
    bytes merges deeply; and a pair led by each byte value in turn."""
    rng = np.random.default_rng(seed)
    have = {bytes([b]) for b in range(256)}
    pool, merges, seen = sorted(have), [], set()
    sample = [_HOT[i] for i in rng.integers(0, len(_HOT), 6000)]
    while len(merges) < BPE_RANDOM_MERGES:
        trained = len(merges) % 2 == 0 and len(sample) > 1000
        if trained:
            i = int(rng.integers(0, len(sample) - 1))
            l, r = sample[i], sample[i + 1]
        else:
            l = bytes([(len(merges) // 2) % 256])
            r = pool[int(rng.integers(0, len(pool)))]
        if (l, r) in seen or l + r in have or len(l + r) > 12:
            continue
        seen.add((l, r))
        have.add(l + r)
        merges.append((l, r))
        pool.append(l + r)
        if trained:
            out, k = [], 0
            while k < len(sample):
                if k + 1 < len(sample) and (sample[k], sample[k + 1]) == (l, r):
                    out.append(l + r)
                    k += 2
                else:
                    out.append(sample[k])
                    k += 1
            sample = out
    return merges


@functools.lru_cache(maxsize=None)
def bpe_table(name: str) -> BpeTable:
    if name == "none":
        return BpeTable([])
    if name == "aa":
        return BpeTable([(b"a", b"a")])
    if name == "chain":
        # every merge makes a pair of lower rank than any pair present
        return BpeTable([(b"abc", b"d"), (b"ab", b"c"), (b"a", b"b")])
    if name == "right":
        # in "abc" the pair of lower rank lies to the right of the other
        return BpeTable([(b"b", b"c"), (b"a", b"b")])
    assert name == "random"
    return BpeTable(_random_merges(BPE_RANDOM_SEED))


BPE_TABLES = ["none", "aa", "chain", "right", "random"]
_UTF8 = "ab \0é€漢😀"


def _hot_text(rng, ln: int, utf8: bool) -> bytes:
    """Text over the hot bytes.  With `utf8` whole characters, cut or padded
    with 'a' to `ln` bytes; otherwise raw bytes with 0x00 and 0xFF."""
    if not utf8:
        return b"".join(_HOT[i] for i in rng.integers(0, len(_HOT), ln))
    out = ""
    while len(out.encode()) < ln:
        out += _UTF8[int(rng.integers(0, len(_UTF8)))]
    while len(out.encode()) > ln:
        out = out[:-1]
    return out.encode() + b"a" * (ln - len(out.encode()))


def _sparse_text(rng, ln: int, burst, utf8: bool) -> bytes:
    """A long row that needs few merges, so that the plain oracle stays
    quick: filler that takes part in no hot merge, with a burst every 47
    bytes, and one at the very start and at the very end."""
    fill = b"z" if utf8 else bytes([0x31 + int(rng.integers(0, 8))])
    out = bytearray()
    while len(out) < ln:
        out += burst(rng) + fill * 40
    out = out[:ln]
    tail = burst(rng)[:ln]
    out[ln - len(tail):] = tail
    return bytes(out)


@functools.lru_cache(maxsize=None)
def bpe_texts(name: str, utf8: bool) -> tuple:
    """One text of every length in BPE_LENS and the named special rows.
    `utf8` texts are valid UTF-8 (for a string column); the others hold any
    byte (for a binary column)."""
    rng = np.random.default_rng([BPE_TABLES.index(name), int(utf8)])
    out = []
    for ln in BPE_LENS:
        short = ln <= 130
        if name == "none":
            t = _hot_text(rng, ln, utf8)
        elif name == "aa":
            # runs of `a`: ties across lanes and across 64-wide strides, and
            # a shift that crosses chunks
            t = b"a" * ln if short else _sparse_text(
                rng, ln, lambda r: b"a" * int(r.integers(2, 8)), True)
        elif name in ("chain", "right"):
            t = (b"abcdabcabd" * (ln // 10 + 1))[:ln] if short else \
                _sparse_text(rng, ln, lambda r: b"abcdabc"[
                    int(r.integers(0, 3)):], True)
        else:
            t = _hot_text(rng, ln, utf8) if short else _sparse_text(
                rng, ln, lambda r: _hot_text(r, 8, utf8), utf8)
        assert len(t) == ln
        out.append(t)
    if name == "aa":
        out += [b"aaa", b"aaaa", b"aaaaa", b"baab", b"a" * 63 + b"b" + b"a" * 66,
                b"b" * 4000 + b"a" * 91, b"a" * 5 + b"b" * 4091]
    if name == "chain":
        out += [b"abcd", b"abc", b"ab", b"dabcd", b"aabcdd", b"abcabcd"]
    if name == "right":
        out += [b"abc", b"abcbc", b"aabcc", b"ababc", b"bcab"]
    if name == "random":
        out += [_hot_text(rng, 300, utf8), _hot_text(rng, 1000, utf8)]
        if utf8:
            out += ["€漢😀 é".encode() * 9]
        else:
            out += [bytes(range(256)), b"\x00\xff" * 70, b"\xff" * 65]
    return tuple(out)


def expected_bpe(name: str, texts: Sequence[Optional[bytes]]) -> tuple:
    """Token ids per text, None for None; each text is encoded once."""
    t = bpe_table(name)
    for x in texts:
        if x is not None and x not in t._memo:
            t._memo[x] = tuple(t.encode(x))
    return tuple(None if x is None else t._memo[x] for x in texts)


@functools.lru_cache(maxsize=None)
def bpe_short_rows(n: int = 4100) -> tuple:
    """More rows than the 4096-block grid, so a block takes a second row
    into the LDS its first row used; the second is the shorter one."""
    rng = np.random.default_rng(n)
    return tuple(_hot_text(rng, 8 if i < 4096 else 3, True) if i % 11
                 else None for i in range(n))


def bpe_table_slots(t: BpeTable):
    """(home slot, actual slot) of every key of the device hash table, from
    the tensors `tokenizer.tables` builds; the hash is that of pair_lookup in
    csrc/bpe.hip."""
    _b2i, keys, _vals = t.tokenizer.tables("cpu")
    size = int(keys.numel())
    out = []
    for slot, k in enumerate(keys.tolist()):
        if k == -1:
            continue
        x = k & M64
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & M64
        x ^= x >> 29
        out.append((x & (size - 1), slot))
    return size, out


# ---------------------------------------------------------------------------
# Levenshtein
# ---------------------------------------------------------------------------

LEV_MAX_LEN = 512             # longer rows take the host fallback
LEV_LENS = [0, 1, 2, 511, 512, 513]


def levenshtein_oracle(a, b) -> int:
    """Full-matrix Wagner-Fischer over the items of `a` and `b` (code points
    for str, bytes for bytes)."""
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        ai, row, up = a[i - 1], d[i], d[i - 1]
        for j in range(1, len(b) + 1):
            sub = up[j - 1] + (0 if ai == b[j - 1] else 1)
            dele = up[j] + 1
            ins = row[j - 1] + 1
            row[j] = sub if sub <= dele and sub <= ins else \
                dele if dele <= ins else ins
    return d[len(a)][len(b)]


def _alpha_text(rng, ln: int, alphabet: str) -> str:
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), ln))


@functools.lru_cache(maxsize=None)
def lev_pairs() -> tuple:
    """(a, b) pairs of str or None."""
    rng = np.random.default_rng(31)
    pairs: List[Tuple[Optional[str], Optional[str]]] = []
    for la in LEV_LENS:
        for lb in LEV_LENS:
            pairs.append((_alpha_text(rng, la, "abcd"),
                          _alpha_text(rng, lb, "abcd")))
    x512 = _alpha_text(rng, 512, "abcdefgh")
    pairs += [
        ("", ""), ("kitten", "sitting"), ("flaw", "lawn"),
        ("same text", "same text"), (x512, x512),                 # equal
        ("abcabc", "xyzxyz"), ("a" * 512, "b" * 512),             # disjoint
        ("abcdef", "abcxef"), ("abcdef", "abcef"), ("abcdef", "abcXdef"),
        (x512, x512[:100] + "Z" + x512[101:]),                    # one edit
        (x512, x512[:300] + x512[301:]), (x512[:511], x512),
        ("prefix", "prefix and more"), ("a suffix", "suffix"),
        (x512, x512[:7]), (x512[500:], x512),
        ("naïve café", "naive cafe"),                             # a only
        ("naive cafe", "naïve café"),                             # b only
        ("cafe", "café"), ("café", "cafe"), ("abc€", "abc€"),     # last only
        ("é", "e"),                        # 1 in characters, 2 in bytes
        ("漢字😀", "漢😀字"), ("€", ""), ("", "😀😀"),
        ("x" * 510 + "é", "x" * 512),      # 512 bytes, not ASCII
        ("x" * 511 + "é", "x" * 513),
        (None, "abc"), ("abc", None), (None, None),
    ]
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def expected_lev() -> tuple:
    return tuple(None if a is None or b is None else levenshtein_oracle(a, b)
                 for a, b in lev_pairs())


LEV_RAW_N = 600_001
LEV_RAW_MAX_LEN = 8


@functools.lru_cache(maxsize=None)
def lev_raw_pool() -> tuple:
    """64 pairs of 0-8 byte rows, and what the raw binding returns for them
    with max_len = 8: the byte distance, or -1 for a pair with a byte >=
    0x80 (such rows are left to the host)."""
    rng = np.random.default_rng(64)
    pool = [(b"", b""), (b"", b"abcdefgh"), (b"abcdefgh", b""),
            (b"abcdefgh", b"abcdefgh"), (b"abcdefgh", b"hgfedcba"),
            (b"aaaaaaaa", b"bbbbbbbb"), (b"a", b"b"), (b"ab", b"ba"),
            ("é".encode(), b"e"), (b"abc", b"ab\xff")]
    while len(pool) < 64:
        pool.append((_alpha_text(rng, int(rng.integers(0, 9)), "abc").encode(),
                     _alpha_text(rng, int(rng.integers(0, 9)), "abc").encode()))
    want = [-1 if max(a + b + b"\0") >= 0x80 else levenshtein_oracle(a, b)
            for a, b in pool]
    return tuple(pool), tuple(want)


# ---------------------------------------------------------------------------
# image resize
# ---------------------------------------------------------------------------

# A pixel may differ by 1 from the oracle only where the oracle's unrounded
# value is this close to a rounding boundary k + 0.5.  The kernel works in
# fp32: a source coordinate up to 64 carries an error of about 64 * 2^-23,
# which moves the interpolated value by at most that times the largest
# difference of neighbouring pixels, 255: about 2e-3.  The constant is about
# 5 times that bound.
RESIZE_NEAR = 0.01
RESIZE_NEAR_SHARE = 0.05      # at most this share of a case's pixels


def _axis(out: int, src: int):
    """Per output index: the two clamped source indices and the weight of
    the second.  Source coordinate ((2*o + 1) * src - out) / (2 * out)."""
    o = np.arange(out, dtype=np.int64)
    num, den = (2 * o + 1) * src - out, 2 * out
    i0 = num // den                                   # floor, exact
    frac = (num - i0 * den).astype(np.float64) / den
    return np.maximum(i0, 0), np.minimum(i0 + 1, src - 1), frac


def resize_oracle(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """Unrounded bilinear resize of one [h, w, c] uint8 image, float64."""
    h, w, _c = img.shape
    y0, y1, dy = _axis(oh, h)
    x0, x1, dx = _axis(ow, w)
    f = img.astype(np.float64)
    dy, dx = dy[:, None, None], dx[None, :, None]
    top = f[y0][:, x0] * (1 - dx) + f[y0][:, x1] * dx
    bot = f[y1][:, x0] * (1 - dx) + f[y1][:, x1] * dx
    return top * (1 - dy) + bot * dy


def round_half_up(v: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def resize_is_dyadic(h: int, w: int, oh: int, ow: int) -> bool:
    """Every interpolation weight is a multiple of 1/16.  Then fp32 is
    exact: coordinates and weights are representable, a product of a pixel
    and two weights has at most 8 + 4 + 4 bits, and so has the sum.  Such an
    image gets no allowance, exact ties included (64x48 -> 16x16 has them
    in half of its pixels)."""
    fracs = np.concatenate([_axis(oh, h)[2], _axis(ow, w)[2]])
    return bool(np.array_equal(fracs * 16, np.round(fracs * 16)))


def resize_near_boundary(v: np.ndarray, dyadic: bool = False) -> np.ndarray:
    """The pixels that may differ by 1: none of a dyadic image."""
    if dyadic:
        return np.zeros(v.shape, dtype=bool)
    t = v + 0.5
    return np.abs(t - np.round(t)) < RESIZE_NEAR


class ResizeCase:
    """`images`: [h, w, 3] uint8 arrays, or None for a null row (h = w = 0,
    no bytes)."""

    def __init__(self, images, oh: int, ow: int, exact: bool):
        self.images, self.oh, self.ow, self.exact = images, oh, ow, exact

    def series(self, dev) -> Series:
        datas = [b"" if a is None else a.tobytes() for a in self.images]
        hs = [0 if a is None else a.shape[0] for a in self.images]
        ws = [0 if a is None else a.shape[1] for a in self.images]
        cs = [0 if a is None else 3 for a in self.images]
        valid = None
        if any(a is None for a in self.images):
            valid = torch.tensor([a is not None for a in self.images])
        return _image_struct("img", datas, hs, ws, cs, cs, valid, dev)

    @functools.cached_property
    def unrounded(self) -> List[Optional[np.ndarray]]:
        return [None if a is None else resize_oracle(a, self.oh, self.ow)
                for a in self.images]

    @functools.cached_property
    def near(self) -> List[Optional[np.ndarray]]:
        """Per image, the mask of pixels that may differ by 1."""
        return [None if a is None else resize_near_boundary(
            v, self.exact or resize_is_dyadic(*a.shape[:2], self.oh, self.ow))
            for a, v in zip(self.images, self.unrounded)]


def _steps16(rng, h: int, w: int) -> np.ndarray:
    return (rng.integers(0, 16, (h, w, 3)) * 16).astype(np.uint8)


def _any(rng, h: int, w: int) -> np.ndarray:
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)


def _tie() -> np.ndarray:
    return np.repeat(np.array([[0, 1], [0, 1]], np.uint8)[:, :, None], 3, 2)


@functools.lru_cache(maxsize=None)
def resize_cases() -> Dict[str, ResizeCase]:
    rng = np.random.default_rng(2024)
    s16 = _steps16(rng, 16, 16)
    const = np.full((5, 9, 3), 0, np.uint8)
    const[:] = (0, 144, 255)
    cases = {
        # pixel values are multiples of 16 and the size ratios powers of two:
        # every weight and product is a small dyadic fraction, exact in fp32
        "identity_16": ResizeCase([s16], 16, 16, True),
        "up2": ResizeCase([s16], 32, 32, True),
        "up4": ResizeCase([s16], 64, 64, True),
        "down2": ResizeCase([s16], 8, 8, True),
        "down4": ResizeCase([s16], 4, 4, True),
        "down2_to_1x9": ResizeCase([_steps16(rng, 2, 18)], 1, 9, True),
        "tie_rounds_up": ResizeCase([_tie()], 1, 1, True),
        "tie_rounds_up_wide": ResizeCase(
            [np.concatenate([_tie(), _tie() * 3], 1)], 1, 2, True),
        "constant": ResizeCase([const, const[:1, :1], const], 7, 11, True),
        "constant_255": ResizeCase([np.full((3, 5, 3), 255, np.uint8)],
                                   16, 16, True),
        "src_1x1": ResizeCase([_any(rng, 1, 1)], 16, 16, True),
        "src_1x7": ResizeCase([_steps16(rng, 1, 7)], 16, 16, True),
        "src_7x1": ResizeCase([_steps16(rng, 7, 1)], 16, 16, True),
        "src_1x7_to_1x1": ResizeCase([_steps16(rng, 1, 7)], 1, 1, True),
        "src_7x1_to_1x9": ResizeCase([_steps16(rng, 7, 1)], 1, 9, True),
        "out_1x1": ResizeCase([s16], 1, 1, True),
        "null_first": ResizeCase([None, s16, s16[:8]], 8, 8, True),
        "null_last": ResizeCase([s16, s16[:, :8], None], 8, 8, True),
        "null_between": ResizeCase([s16, None, None, s16[:4, :4]], 4, 4,
                                   True),
        "all_null": ResizeCase([None, None, None], 4, 4, True),
    }
    for h, w in ((5, 3), (3, 5), (64, 48), (37, 53)):
        for oh, ow in ((16, 16), (7, 11)):
            cases[f"random_{h}x{w}_to_{oh}x{ow}"] = ResizeCase(
                [_any(rng, h, w)], oh, ow, False)
    sizes = [(5, 3), (64, 48), (1, 1), (37, 53), (2, 60), (60, 2), (16, 16),
             (33, 31)]
    cases["mixed_batch_of_8"] = ResizeCase(
        [_any(rng, h, w) for h, w in sizes], 16, 16, False)
    # 12 * 128 * 128 * 3 = 589 824 outputs, more than 2048 blocks x 256
    # threads, so the grid-stride loop runs
    cases["grid_stride_12x128x128"] = ResizeCase(
        [_any(rng, 20 + 3 * i, 50 - 2 * i) for i in range(12)], 128, 128,
        False)
    return cases


RESIZE_CASES = list(resize_cases())


def image_series_with_channels(channels: int, dev, valid: bool = True):
    """Two RGB rows and one `channels`-channel row."""
    rgb = np.zeros((2, 2, 3), np.uint8)
    odd = np.zeros((2, 2, channels), np.uint8)
    validity = None if valid else torch.tensor([True, False, True])
    return _image_struct("img", [rgb.tobytes(), odd.tobytes(), rgb.tobytes()],
                         [2, 2, 2], [2, 2, 2], [3, channels, 3],
                         [3, channels, 3], validity, dev)

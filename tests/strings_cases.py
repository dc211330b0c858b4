"""Shared corpus, column variants, Python oracle and check drivers for the
string-kernel tests (test_strings_parity.py on the CPU path,
test_gpu_strings.py on the HIP path).  A plain helper module: no fixtures.

The oracle functions use Python `str` / `bytes` / `re` only and never call
into daft_amd.kernels; the check drivers below them call the code under
test and compare it with the oracle."""
from __future__ import annotations

import functools
import random
import re
from typing import List, Optional

import numpy as np
import pytest
import torch

from daft_amd import DataType, Series
from daft_amd.kernels import compare_op, if_else, rowops
from daft_amd.kernels import strings as strk

# ---------------------------------------------------------------------------
# corpus
# ---------------------------------------------------------------------------

ALPHABET = ["a", "b", "A", "B", " ", "\n", "é", "ß", "€", "漢", "😀"]
MULTIBYTE = ["é", "ß", "€", "漢", "😀"]
ALL_MULTIBYTE_40 = "é€漢😀ß" * 8

# Every string draws from ONE of these sub-alphabets, so that the needles
# below hit at the start, at the end and inside often enough (the weights
# are cumulative percent; the first three kinds are pure ASCII, 35%).
_KINDS = [
    (24, ["a", "b"]),
    (29, ["a", "b", "A", "B", " ", "\n"]),
    (35, ["\n", "a"]),
    (50, ["€", "a"]),
    (60, ["é", "a", "b"]),
    (70, ["😀", "\n", "a"]),
    (78, MULTIBYTE),
    (100, ALPHABET),
]

SIZES = [0, 1, 255, 256, 257, 4099]
MAX_CHARS = 40


def _corpus(n: int, seed: int) -> list:
    rng = random.Random(seed * 1_000_003 + n)
    out = []
    for _ in range(n):
        if rng.random() < 0.10:
            out.append(None)
            continue
        pick = rng.random() * 100
        chars = next(c for w, c in _KINDS if pick < w)
        ln = int(rng.random() * (MAX_CHARS + 1))
        out.append("".join(chars[int(rng.random() * len(chars))]
                           for _ in range(ln)))
    # fixed rows (inside the slice(3, n-2) window): the empty string, a
    # single 4-byte character, 40 characters that are all multi-byte
    if n == 1:
        out[0] = "😀"
    elif n >= 16:
        out[5] = ""
        out[n // 2] = "😀"
        out[n - 5] = ALL_MULTIBYTE_40
    return out


@functools.lru_cache(maxsize=None)
def _corpus_cached(n: int, seed: int) -> tuple:
    return tuple(_corpus(n, seed))


def corpus(n: int, seed: int = 0) -> list:
    """`n` deterministic values: str of 0..40 characters, None for ~10%."""
    return list(_corpus_cached(n, seed))


# ---------------------------------------------------------------------------
# parameter lists
# ---------------------------------------------------------------------------

LONG_NEEDLE = "ab" * 20 + "a"        # 41 characters: longer than any row
NEEDLES = ["", "a", "ab", "aab", "é", "€a", "😀", "\n", LONG_NEEDLE]
LIKE_PATTERNS = ["%", "%%", "%a%", "%ab%ab%", "%é%😀%", "%ab",
                 "a%", "ab%", "a%a", "a%b%a", "ab", "_%", "a_", "%_b"]
SUBSTR_ARGS = [(s, l) for s in (0, 1, 2, 39, 40, 41)
               for l in (None, 0, 1, 2, 100)]
LEFT_ARGS = [0, 1, 3, 100]
VARIANTS = ["plain", "slice", "dict", "masked"]
COMPARE_OPS = ["eq", "ne", "lt", "le", "gt", "ge"]


# ---------------------------------------------------------------------------
# oracle: Python str / bytes / re only
# ---------------------------------------------------------------------------

def _map(values, f):
    return [None if v is None else f(v) for v in values]


def o_contains(values, p):
    return _map(values, lambda v: p in v)


def o_startswith(values, p):
    return _map(values, lambda v: v.startswith(p))


def o_endswith(values, p):
    return _map(values, lambda v: v.endswith(p))


def _like_rx(pattern: str, ci: bool):
    rx = "".join(".*" if c == "%" else "." if c == "_" else re.escape(c)
                 for c in pattern)
    return re.compile(rx, re.DOTALL | (re.IGNORECASE if ci else 0))


def o_like(values, pattern, ci=False):
    rx = _like_rx(pattern, ci)
    return _map(values, lambda v: rx.fullmatch(v) is not None)


def o_find(values, p):
    pb = p.encode()
    return _map(values, lambda v: v.encode().find(pb))


def o_length(values):
    return _map(values, len)


def o_length_bytes(values):
    return _map(values, lambda v: len(v.encode()))


def o_substr(values, start, length):
    if length is None:
        return _map(values, lambda v: v[start:])
    return _map(values, lambda v: v[start:start + length])


def o_left(values, n):
    return _map(values, lambda v: v[:n])


def o_lower(values):
    return _map(values, str.lower)


def o_upper(values):
    return _map(values, str.upper)


def o_concat(*cols):
    return [None if any(v is None for v in vs) else "".join(vs)
            for vs in zip(*cols)]


def o_compare3(a, b):
    """-1 / 0 / 1 on the UTF-8 bytes (None where either side is null)."""
    out = []
    for x, y in zip(a, b):
        if x is None or y is None:
            out.append(None)
        else:
            xb, yb = _bytes(x), _bytes(y)
            out.append((xb > yb) - (xb < yb))
    return out


def o_compare(a, b, op):
    f = {"eq": lambda c: c == 0, "ne": lambda c: c != 0,
         "lt": lambda c: c < 0, "le": lambda c: c <= 0,
         "gt": lambda c: c > 0, "ge": lambda c: c >= 0}[op]
    return [None if c is None else f(c) for c in o_compare3(a, b)]


def _bytes(v) -> bytes:
    return v if isinstance(v, bytes) else v.encode()


def o_sort_perm(values, descending=False, nulls_first=False) -> List[int]:
    """Stable byte-order argsort: equal values keep their row order in
    both directions, and so do the nulls, which go last unless
    `nulls_first`."""
    nulls = [i for i, v in enumerate(values) if v is None]
    rows = [i for i, v in enumerate(values) if v is not None]
    rows = sorted(rows, key=lambda i: _bytes(values[i]), reverse=descending)
    return nulls + rows if nulls_first else rows + nulls


def o_chunk_key(values, chunk: int) -> List[int]:
    """Big-endian u64 of bytes [8c, 8c+8), zero padded."""
    return [int.from_bytes(_bytes(v)[8 * chunk:8 * chunk + 8]
                           .ljust(8, b"\0"), "big") for v in values]


# ---------------------------------------------------------------------------
# corpus guards: the conditions that keep the tests from being vacuous
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def corpus_guards(n: int = 4099, seed: int = 0) -> dict:
    """Assert the conditions on the corpus and return the measured shares."""
    vals = [v for v in corpus(n, seed) if v is not None]
    assert 0.05 < 1 - len(vals) / n < 0.15
    total_bytes = sum(len(v.encode()) for v in vals)
    assert total_bytes / n >= 20 and total_bytes > 64 * 1024
    ascii_share = sum(v.isascii() for v in vals) / len(vals)
    assert 0.25 <= ascii_share <= 0.45, ascii_share
    assert "" in vals and "😀" in vals and ALL_MULTIBYTE_40 in vals
    assert max(len(v) for v in vals) == MAX_CHARS
    shares = {}
    for name, f in (("contains", o_contains), ("startswith", o_startswith),
                    ("endswith", o_endswith)):
        for p in NEEDLES:
            if p in ("", LONG_NEEDLE):
                continue
            t = sum(f(vals, p)) / len(vals)
            shares[(name, p)] = t
            assert 0.02 <= t <= 0.98, (name, p, t)
    offsets = {}
    for p in NEEDLES:
        if p in ("", LONG_NEEDLE):
            continue
        offsets[p] = len({x for x in o_find(vals, p) if x >= 0})
        assert offsets[p] >= 3, (p, offsets[p])
    early = sum(any(len(c.encode()) > 1 for c in v[:2]) for v in vals) \
        / len(vals)
    assert early >= 0.25, early
    return {"true_share": shares, "ascii_share": ascii_share,
            "multibyte_before_cp2": early, "total_bytes": total_bytes,
            "find_offsets": offsets}


# ---------------------------------------------------------------------------
# column variants, all holding the same values
# ---------------------------------------------------------------------------

def _plain(values, device, dtype=None):
    return Series.from_pylist("s", list(values), dtype or DataType.string(),
                              device=device)


def make_variant(values: list, variant: str, device="cpu"):
    """(Series on `device`, the values it holds)."""
    n = len(values)
    if variant == "plain":
        return _plain(values, device), list(values)
    if variant == "slice":
        # sliced on the device: `data` is a view at a non-zero storage offset
        return _plain(values, device).slice(3, n - 2), \
            list(values[3:max(3, n - 2)])
    if variant == "dict":
        vocab = list(dict.fromkeys(v for v in values if v is not None)) \
            or [""]
        code = {v: i for i, v in enumerate(vocab)}
        codes = torch.tensor([code.get(v, 0) for v in values],
                             dtype=torch.int32)
        validity = torch.tensor([v is not None for v in values],
                                dtype=torch.bool)
        s = Series.make_dict("s", _plain(vocab, "cpu"), codes,
                             None if bool(validity.all()) else validity)
        return s.to(device), list(values)
    if variant == "masked":
        # nulls laid over non-empty rows: null rows have bytes under them
        hide = [bool(v) and i % 7 == 3 for i, v in enumerate(values)]
        s = _plain(values, device)
        keep = torch.tensor([v is not None and not h
                             for v, h in zip(values, hide)],
                            dtype=torch.bool).to(device)
        return s.with_validity(keep), \
            [None if h else v for v, h in zip(values, hide)]
    raise ValueError(variant)


@functools.lru_cache(maxsize=None)
def column(n: int, variant: str, device: str = "cpu", seed: int = 0):
    s, vals = make_variant(corpus(n, seed), variant, device)
    assert len(s) == len(vals)
    return s, tuple(vals)


def shuffled(values, seed: int = 1) -> list:
    out = list(values)
    random.Random(seed).shuffle(out)
    return out


# ---------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------

def assert_bool(out: Series, expected, src: Optional[Series] = None):
    """A predicate result: values, and the input's validity passed on."""
    assert out.to_pylist() == list(expected)
    if src is not None:
        if src.validity is None:
            assert out.validity is None
        else:
            assert torch.equal(out.validity.cpu(), src.validity.cpu())


def assert_ints(out: Series, expected):
    assert out.to_pylist() == list(expected)


def assert_strings(out: Series, expected):
    """A string result, as Python values and as raw offsets + bytes (so
    invalid UTF-8 cannot hide behind a decode)."""
    out = out.dict_decode().cpu()
    expected = list(expected)
    assert len(out) == len(expected)
    off = out.offsets.numpy()
    buf = out.data.numpy().tobytes() if out.data.numel() else b""
    assert off[0] == 0 and off[-1] == len(buf)
    assert (np.diff(off) >= 0).all()
    valid = None if out.validity is None else out.validity.numpy()
    for i, e in enumerate(expected):
        ok = valid is None or bool(valid[i])
        assert ok == (e is not None), f"row {i}: validity {ok}, want {e!r}"
        if e is not None:
            got = buf[off[i]:off[i + 1]]
            assert got == _bytes(e), f"row {i}: {got!r} != {_bytes(e)!r}"
    assert out.to_pylist() == expected


# ---------------------------------------------------------------------------
# string columns that every native entry point refuses on the host
# ---------------------------------------------------------------------------

REFUSED_VALUES = ["ab", "€", "abc"]       # the 3-row column of these tests


def bad_columns(offsets, data) -> list:
    """(what, offsets, bytes): a valid device column with one thing wrong.
    None of them reaches a kernel, so none can fault."""
    return [
        ("offsets on the CPU", offsets.cpu(), data),
        ("int32 offsets", offsets.to(torch.int32), data),
        ("strided offsets", offsets[::2], data),
        ("offsets without elements", offsets[:0], data),
        ("int8 bytes", offsets, data.to(torch.int8)),
        ("bytes on the CPU", offsets, data.cpu()),
    ]


def assert_refuses_bad_columns(binding: str, call, offsets, data):
    """`call(offsets, bytes)` raises RuntimeError, worded by the binding's
    own check, for every bad column."""
    assert not offsets[::2].is_contiguous()
    for what, o, d in bad_columns(offsets, data):
        with pytest.raises(RuntimeError, match=binding + ": "):
            call(o, d)
            raise AssertionError(f"{binding} accepted {what}")


# ---------------------------------------------------------------------------
# check drivers: the same matrix runs on the CPU path and on the HIP path
# ---------------------------------------------------------------------------

def check_find_family(n, variant, device):
    s, vals = column(n, variant, device)
    for p in NEEDLES:
        assert_bool(strk.contains(s, p), o_contains(vals, p), s)
        assert_bool(strk.startswith(s, p), o_startswith(vals, p), s)
        assert_bool(strk.endswith(s, p), o_endswith(vals, p), s)
        assert_ints(strk.find(s, p), o_find(vals, p))


def check_like(n, variant, device):
    s, vals = column(n, variant, device)
    for pat in LIKE_PATTERNS:
        assert_bool(strk.like(s, pat), o_like(vals, pat), s)
        assert_bool(strk.like(s, pat, case_insensitive=True),
                    o_like(vals, pat, ci=True), s)


def check_lengths(n, variant, device):
    s, vals = column(n, variant, device)
    assert_ints(strk.length(s), o_length(vals))
    assert_ints(strk.length_bytes(s), o_length_bytes(vals))


def check_substr(n, variant, device):
    s, vals = column(n, variant, device)
    for start, length in SUBSTR_ARGS:
        assert_strings(strk.substr(s, start, length),
                       o_substr(vals, start, length))
    for k in LEFT_ARGS:
        assert_strings(strk.left(s, k), o_left(vals, k))


def check_substr_binary(device):
    """BINARY columns slice bytes, not code points."""
    vals = [None if v is None else v.encode() for v in corpus(257)]
    s = _plain(vals, device, DataType.binary())
    for start, length in ((0, 1), (1, 2), (3, None), (2, 100), (200, 1)):
        out = strk.substr(s, start, length)
        assert out.dtype == DataType.binary()
        assert out.to_pylist() == o_substr(vals, start, length)


def check_substr_rejects_negative(device):
    """Raises before any launch: nothing here reaches a kernel."""
    s, _ = column(257, "plain", device)
    for start, length in ((-1, None), (-1, 2), (0, -1), (-3, -3)):
        with pytest.raises(ValueError):
            strk.substr(s, start, length)
    with pytest.raises(ValueError):
        strk.left(s, -1)


def check_case(n, variant, device):
    s, vals = column(n, variant, device)
    assert_strings(strk.lower(s), o_lower(vals))
    assert_strings(strk.upper(s), o_upper(vals))


def check_case_ascii(n, device):
    """All-ASCII column: on the GPU this is the byte-parallel kernel."""
    vals = [None if v is None else
            "".join(c for c in v if c.isascii()) for v in corpus(n)]
    for variant in VARIANTS:
        s, held = make_variant(vals, variant, device)
        assert_strings(strk.lower(s), o_lower(held))
        assert_strings(strk.upper(s), o_upper(held))


def check_concat(n, variant, device):
    s, vals = column(n, variant, device)
    other_vals = shuffled(vals)
    other = _plain(other_vals, device)
    lit = _plain(["€-"], device)
    m = len(vals)
    assert_strings(strk.concat_str([s]), o_concat(vals))
    assert_strings(strk.concat_str([s, other]), o_concat(vals, other_vals))
    assert_strings(strk.concat_str([s, lit, other]),
                   o_concat(vals, ["€-"] * m, other_vals))
    assert_strings(strk.concat_str([lit, s]), o_concat(["€-"] * m, vals))


def check_compare(n, variant, device):
    s, vals = column(n, variant, device)
    other_vals = shuffled(vals)
    # a shuffled copy is rarely equal: put equal rows and prefixes in too
    for i in range(0, len(vals), 5):
        other_vals[i] = vals[i]
    for i in range(1, len(vals), 5):
        if vals[i]:
            other_vals[i] = vals[i][:-1]
    other = _plain(other_vals, device)
    for op in COMPARE_OPS:
        assert_bool(compare_op(s, other, op), o_compare(vals, other_vals, op))
        assert_bool(compare_op(other, s, op), o_compare(other_vals, vals, op))


def check_if_else(n, variant, device):
    """merge_strings on the GPU: rows of two corpus columns by a mask."""
    t, tv = column(n, variant, device)
    fv = shuffled(tv, seed=4)
    f = _plain(fv, device)
    rng = random.Random(5)
    mask = [rng.random() < 0.5 for _ in tv]
    cond = Series.from_pylist("c", mask, DataType.bool(), device=device)
    assert_strings(if_else(cond, t, f),
                   [a if c else b for c, a, b in zip(mask, tv, fv)])
    assert_strings(if_else(cond, f, t),
                   [b if c else a for c, a, b in zip(mask, tv, fv)])


SORT_ORDERS = [(False, False), (True, False), (False, True), (True, True)]


def _perm(s, descending, nulls_first):
    return rowops.argsort_multi([s], [descending], [nulls_first]) \
        .cpu().tolist()


def check_sort(n, variant, device):
    s, vals = column(n, variant, device)
    for desc, nf in SORT_ORDERS:
        assert _perm(s, desc, nf) == o_sort_perm(vals, desc, nf)


LONG_SORT_VALUES = [
    "é" * 20 + t for t in ("", "a", "b", "aa")] + [
    "ab" * 4 + t for t in ("", "a", "b", "\n")] + [
    "ab" * 8 + t for t in ("", "a", "😀")] + [
    "ab" * 16 + t for t in ("", "a", "€", "€a")] + [
    "ab" * 16, "ab" * 4, None, "", "a"]


def check_sort_long(device):
    """Strings over 8, 16 and 32 bytes that share their first chunks."""
    vals = shuffled(LONG_SORT_VALUES * 3, seed=2)
    s = _plain(vals, device)
    for desc, nf in SORT_ORDERS:
        assert _perm(s, desc, nf) == o_sort_perm(vals, desc, nf)


NUL_TAIL_VALUES = ["a\0", "a", "a\0\0", "a", "", "\0", None, "a\0b",
                   "a" * 8, "a" * 8 + "\0", "a" * 7 + "\0", "a" * 7]


def check_sort_nul_tail(device):
    """A value that is another value plus trailing 0x00 bytes sorts after
    it, for STRING and for BINARY."""
    assert o_sort_perm(["a\0", "a", "a\0\0", "a"]) == [1, 3, 0, 2]
    for dtype, conv in ((DataType.string(), lambda v: v),
                        (DataType.binary(),
                         lambda v: None if v is None else v.encode())):
        vals = [conv(v) for v in NUL_TAIL_VALUES]
        s = _plain(vals, device, dtype)
        for desc, nf in SORT_ORDERS:
            assert _perm(s, desc, nf) == o_sort_perm(vals, desc, nf)
        four = _plain(vals[:4], device, dtype)
        assert _perm(four, False, False) == [1, 3, 0, 2]

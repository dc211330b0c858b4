"""Corpus, Python oracles and check drivers for the text-cleanup functions
(normalize, strip / lstrip / rstrip, right, reverse, capitalize, lpad / rpad,
repeat, split): test_strtransform_parity.py runs the drivers on the CPU path,
test_gpu_strtransform.py on the HIP path.  A plain helper module: no
fixtures.

The oracles use Python `str`, `re` and `unicodedata` only and never call
into daft_amd.kernels; the drivers below them call the code under test and
compare it with the oracle through strings_cases.assert_strings (values,
validity, raw offsets and bytes)."""
from __future__ import annotations

import functools
import itertools
import random
import re
import string
import unicodedata

import pytest

from daft_amd import DataType, Series, col
from daft_amd.functions import strings_extra as fx
from daft_amd.kernels import strings as strk

import strings_cases as sc

# ---------------------------------------------------------------------------
# corpus
# ---------------------------------------------------------------------------

# Python's str.isspace set, all 29 (corpus_guards checks it is that set)
ASCII_SPACE = "\t\n\x0b\x0c\r\x1c\x1d\x1e\x1f "
WIDE_SPACE = ("\x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006"
              "\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000")
SPACES = ASCII_SPACE + WIDE_SPACE
PUNCT = string.punctuation.replace("_", "")
CONTROL = "\x00\x1b\x7f"
WORD = string.ascii_letters + string.digits + "_"
MULTIBYTE = "éß€漢😀"
COMBINING = "\u0301"
# characters one byte or one bit away from a space character
NEAR_SPACE = "\x84\xa1\u1681\u200b\u2027\u2030\u2060\u3001\u2014"

SIZES = sc.SIZES
VARIANTS = sc.VARIANTS

_PATTERN = "Ab, c\t\tD_9!  x\x1by?Z \n"


def _pattern_row(length: int) -> str:
    """`length` ASCII bytes of words, punctuation and whitespace runs."""
    return (_PATTERN * (length // len(_PATTERN) + 1))[:length]


NORMALIZE_ROWS = [
    "",
    " \t\n\x1c ",                               # only whitespace
    "!?.,;",                                    # only punctuation
    " ",
    "x" * 64 + " y",                            # a word ending at byte 63
    "a" * 62 + " \t\n\r " + "b",                # whitespace over bytes 62-66
    "a" * 61 + " !?.,; b",                      # punctuation over bytes 62-66
    "a ! b",
] + [_pattern_row(k) for k in (1, 63, 64, 65, 127, 128, 129, 4099)]

STRIP_ROWS = [
    "\xa0\u2003\u3000\u1680\x85",               # only multi-byte whitespace
    "a\u2014",                                  # ends E2 80 94: no space
    "\u2014a",
    " \u2010b\u2010 ",
    "\u200b a \u200b",                          # U+200B is not a space
    "\U0001f600 a b \U0001f600",                # 4-byte first and last
    " \U0001f600x\U0001f600 ",
    "e" + COMBINING + " \u00e9",
]

FIXED_ROWS = NORMALIZE_ROWS + STRIP_ROWS
FIXED_FROM = 255        # sizes from here on hold the fixed rows, from row 5

assert len(NORMALIZE_ROWS[4].encode()) == 66
assert NORMALIZE_ROWS[5][62:67].isspace() and NORMALIZE_ROWS[5][61] == "a"
assert all(c in PUNCT for c in NORMALIZE_ROWS[6][62:67])
assert NORMALIZE_ROWS[6][61] == " " == NORMALIZE_ROWS[6][67]
assert len(NORMALIZE_ROWS[-1]) == 4099 and NORMALIZE_ROWS[-1].isascii()


def _token(rng, ascii_only: bool) -> str:
    kind = rng.random()
    k = 1 + int(rng.random() * 8)
    if kind < 0.60:
        pool = WORD
    elif kind < 0.75:
        pool = PUNCT
    elif kind < 0.80:
        pool = CONTROL + WORD
    elif ascii_only:
        pool = WORD + PUNCT
    elif kind < 0.92:
        pool = MULTIBYTE + "ab"
    elif kind < 0.96:
        pool = "e" + COMBINING + "é"
    else:
        pool = NEAR_SPACE + "a"
    return "".join(pool[int(rng.random() * len(pool))] for _ in range(k))


def _gap(rng, ascii_only: bool, may_be_empty: bool) -> str:
    if may_be_empty and rng.random() < 0.5:
        return ""
    pool = ASCII_SPACE if ascii_only or rng.random() < 0.6 else SPACES
    k = 1 + int(rng.random() * 3)
    return "".join(pool[int(rng.random() * len(pool))] for _ in range(k))


def _corpus(n: int, seed: int) -> list:
    rng = random.Random(seed * 1_000_003 + n + 17)
    out = []
    for _ in range(n):
        if rng.random() < 0.10:
            out.append(None)
            continue
        ascii_only = rng.random() < 0.65
        words = int(rng.random() * 13)
        row = [_gap(rng, ascii_only, True)]
        for _ in range(words):
            row.append(_token(rng, ascii_only))
            row.append(_gap(rng, ascii_only, False))
        if words and rng.random() < 0.5:
            row.pop()                               # no trailing whitespace
        out.append("".join(row))
    if n == 1:
        out[0] = " 😀x "
    elif n >= FIXED_FROM:
        out[5:5 + len(FIXED_ROWS)] = FIXED_ROWS
    return out


@functools.lru_cache(maxsize=None)
def _corpus_cached(n: int, seed: int) -> tuple:
    return tuple(_corpus(n, seed))


def corpus(n: int, seed: int = 0) -> list:
    """`n` deterministic values, None for ~10%."""
    return list(_corpus_cached(n, seed))


def ascii_corpus(n: int, seed: int = 0) -> list:
    """The corpus with every non-ASCII character taken out."""
    return [None if v is None else "".join(c for c in v if c.isascii())
            for v in corpus(n, seed)]


@functools.lru_cache(maxsize=None)
def column(n: int, variant: str, device: str = "cpu", seed: int = 0):
    s, vals = sc.make_variant(corpus(n, seed), variant, device)
    assert len(s) == len(vals)
    return s, tuple(vals)


@functools.lru_cache(maxsize=None)
def ascii_column(n: int, variant: str, device: str = "cpu"):
    s, vals = sc.make_variant(ascii_corpus(n), variant, device)
    return s, tuple(vals)


# ---------------------------------------------------------------------------
# parameter lists
# ---------------------------------------------------------------------------

NORMALIZE_FLAGS = list(itertools.product([False, True], repeat=4))
# (remove_punct, lowercase, nfd_unicode, white_space)
RIGHT_ARGS = [0, 1, 2, 5, 1000]
PAD_ARGS = [(0, " "), (1, "*"), (7, " "), (20, "é"), (40, "😀"), (200, "0")]
REPEAT_ARGS = [0, 1, 3]
SEPARATORS = ["a", "ab", "aa", "€", " "]


# ---------------------------------------------------------------------------
# oracle: Python only
# ---------------------------------------------------------------------------

_map = sc._map


def o_strip(values):
    return _map(values, str.strip)


def o_lstrip(values):
    return _map(values, str.lstrip)


def o_rstrip(values):
    return _map(values, str.rstrip)


def o_right(values, n):
    return _map(values, lambda v: v[-n:] if n else "")


def o_reverse(values):
    return _map(values, lambda v: v[::-1])


def o_capitalize(values):
    return _map(values, str.capitalize)


def o_lpad(values, width, fill):
    return _map(values, lambda v: v.rjust(width, fill)[:width])


def o_rpad(values, width, fill):
    return _map(values, lambda v: v.ljust(width, fill)[:width])


def o_repeat(values, n):
    return _map(values, lambda v: v * n)


def o_split(values, sep):
    return _map(values, lambda v: v.split(sep))


def normalize_value(v, remove_punct, lowercase, nfd_unicode, white_space):
    """The body of daft_amd's normalize as it stood before it had a kernel."""
    if nfd_unicode:
        v = unicodedata.normalize("NFD", v)
        v = "".join(c for c in v if not unicodedata.combining(c))
    if lowercase:
        v = v.lower()
    if remove_punct:
        v = re.sub(r"[^\w\s]", "", v)
    if white_space:
        v = " ".join(v.split())
    return v


def o_normalize(values, remove_punct, lowercase, nfd_unicode, white_space):
    return _map(values, lambda v: normalize_value(
        v, remove_punct, lowercase, nfd_unicode, white_space))


_WS_BYTES = frozenset(ASCII_SPACE.encode())
_WORD_BYTES = frozenset(WORD.encode())


def machine(row: bytes, remove_punct, lowercase, white_space) -> bytes:
    """The per-byte state machine that the normalize kernel implements for
    rows without a byte >= 0x80."""
    out = bytearray()
    state = "none"
    for b in row:
        ws = b in _WS_BYTES
        if remove_punct and not ws and b not in _WORD_BYTES:
            continue
        if white_space and ws:
            if state == "word":
                state = "pending"
            continue
        if white_space and state == "pending":
            out.append(0x20)
        out.append(b + 32 if lowercase and 0x41 <= b <= 0x5A else b)
        state = "word"
    return bytes(out)


# ---------------------------------------------------------------------------
# corpus guards
# ---------------------------------------------------------------------------

def _changed(before, after) -> float:
    pairs = [(b, a) for b, a in zip(before, after) if b is not None]
    return sum(a != b for b, a in pairs) / len(pairs)


@functools.lru_cache(maxsize=None)
def corpus_guards(n: int = 4099) -> dict:
    """Assert the conditions that keep the tests from being vacuous and
    return the measured shares."""
    assert sorted(SPACES) == [chr(c) for c in range(0x110000)
                              if chr(c).isspace()] and len(SPACES) == 29
    assert not any(c.isspace() for c in NEAR_SPACE)
    vals = corpus(n)
    assert all(r in vals for r in FIXED_ROWS)
    live = [v for v in vals if v is not None]
    assert 0.05 < 1 - len(live) / n < 0.15
    for chars in (SPACES, PUNCT, CONTROL, "_", string.digits, "aZ",
                  MULTIBYTE, COMBINING, "é"):
        for c in chars:
            assert any(c in v for v in live), repr(c)
    ascii_share = sum(v.isascii() for v in live) / len(live)
    assert 0.40 <= ascii_share <= 0.90, ascii_share
    assert sum(len(v.encode()) > 64 for v in live) / len(live) > 0.05
    changed = {
        "strip": _changed(vals, o_strip(vals)),
        "lstrip": _changed(vals, o_lstrip(vals)),
        "rstrip": _changed(vals, o_rstrip(vals)),
        "capitalize": _changed(vals, o_capitalize(vals)),
    }
    for w, f in PAD_ARGS:
        changed["lpad", w] = _changed(vals, o_lpad(vals, w, f))
        changed["rpad", w] = _changed(vals, o_rpad(vals, w, f))
    for flags in NORMALIZE_FLAGS:
        if any(flags):
            changed["normalize", flags] = _changed(
                vals, o_normalize(vals, *flags))
    for what, share in changed.items():
        assert share >= 0.10, (what, share)
    # rows trimmed on one side only, and pads that cut as well as fill
    ls, rs = o_lstrip(live), o_rstrip(live)
    assert sum(a != v and b == v for v, a, b in zip(live, ls, rs)) > 50
    assert sum(a == v and b != v for v, a, b in zip(live, ls, rs)) > 50
    assert sum(len(v) > 7 for v in live) > 50 < sum(len(v) < 7 for v in live)
    for sep in SEPARATORS:
        pieces = {len(x) for x in o_split(live, sep)}
        assert 1 in pieces and max(pieces) >= 3, sep
    return {"ascii_share": ascii_share, "changed": changed}


# ---------------------------------------------------------------------------
# check drivers: the same matrix runs on the CPU path and on the HIP path
# ---------------------------------------------------------------------------

def _on(s: Series, device) -> None:
    assert str(s.device).startswith(str(device).split(":")[0])


def check_strip(n, variant, device):
    s, vals = column(n, variant, device)
    for f, o in ((strk.strip, o_strip), (strk.lstrip, o_lstrip),
                 (strk.rstrip, o_rstrip)):
        out = f(s)
        _on(out, device)
        sc.assert_strings(out, o(vals))


def check_right(n, variant, device):
    s, vals = column(n, variant, device)
    for k in RIGHT_ARGS:
        sc.assert_strings(strk.right(s, k), o_right(vals, k))


def check_reverse(n, variant, device):
    s, vals = column(n, variant, device)
    out = strk.reverse(s)
    _on(out, device)
    sc.assert_strings(out, o_reverse(vals))


def check_capitalize(n, variant, device):
    """The UTF-8 corpus (host path everywhere) and the all-ASCII one (on the
    GPU: the case kernel)."""
    for s, vals in (column(n, variant, device),
                    ascii_column(n, variant, device)):
        sc.assert_strings(strk.capitalize(s), o_capitalize(vals))


def check_pad(n, variant, device):
    s, vals = column(n, variant, device)
    for width, fill in PAD_ARGS:
        sc.assert_strings(strk.lpad(s, width, fill),
                          o_lpad(vals, width, fill))
        sc.assert_strings(strk.rpad(s, width, fill),
                          o_rpad(vals, width, fill))


def check_repeat(n, variant, device):
    s, vals = column(n, variant, device)
    for k in REPEAT_ARGS:
        sc.assert_strings(strk.repeat(s, k), o_repeat(vals, k))


def assert_lists(out: Series, expected):
    """A list<string> result: values, row validity, and the child as raw
    offsets + bytes."""
    expected = list(expected)
    assert out.dtype == DataType.list(DataType.string())
    assert out.to_pylist() == expected
    off = [0]
    for e in expected:
        off.append(off[-1] + (0 if e is None else len(e)))
    assert out.offsets.cpu().tolist() == off
    valid = [True] * len(out) if out.validity is None \
        else out.validity.cpu().tolist()
    assert valid == [e is not None for e in expected]
    sc.assert_strings(out.children[0],
                      [x for e in expected if e is not None for x in e])


def check_split(n, variant, device):
    s, vals = column(n, variant, device)
    for sep in SEPARATORS:
        out = strk.split(s, sep)
        _on(out, device)
        assert_lists(out, o_split(vals, sep))


def run_normalize(s: Series, remove_punct, lowercase, nfd_unicode,
                  white_space) -> Series:
    """normalize through its public free function."""
    node = fx.normalize(col("s"), remove_punct=remove_punct,
                        lowercase=lowercase, nfd_unicode=nfd_unicode,
                        white_space=white_space)._node
    return node.fn(s, *node.literal_args, **node.kwargs)


def check_normalize(n, variant, device, flags_list=NORMALIZE_FLAGS):
    s, vals = column(n, variant, device)
    for flags in flags_list:
        out = run_normalize(s, *flags)
        _on(out, device)
        sc.assert_strings(out, o_normalize(vals, *flags))


def check_negative_counts(device):
    """A negative count keeps the meaning Python gives it."""
    s, vals = column(257, "plain", device)
    sc.assert_strings(strk.right(s, -2), _map(vals, lambda v: v[2:]))
    sc.assert_strings(strk.repeat(s, -1), _map(vals, lambda v: ""))
    sc.assert_strings(strk.lpad(s, -2, "*"),
                      _map(vals, lambda v: v.rjust(-2, "*")[:-2]))
    sc.assert_strings(strk.rpad(s, -2, "*"),
                      _map(vals, lambda v: v.ljust(-2, "*")[:-2]))
    assert any(v and v[:-2] != "" for v in vals)


def check_errors(device):
    s, _ = column(257, "plain", device)
    for fill in ("", "ab", "é€"):
        with pytest.raises(TypeError):
            strk.lpad(s, 5, fill)
        with pytest.raises(TypeError):
            strk.rpad(s, 5, fill)
    with pytest.raises(ValueError):
        strk.split(s, "")

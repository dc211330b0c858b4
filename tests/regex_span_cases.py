"""Patterns and `re` oracles for the match-position tests (test_regex_spans.py
on the host table walk and the CPU Series path, test_gpu_regex_spans.py on
the HIP kernels).  A plain helper module: no fixtures.  The oracle is Python
`re` on `str`, with character spans turned into UTF-8 byte offsets, and never
calls into daft_amd."""
from __future__ import annotations

import functools
import random
import re

import regex_cases as rc
import strings_cases as sc

# (pattern, needs_ascii): needs_ascii exactly where the pattern uses a
# \d \w \s class or (?i)
SPAN_SUPPORTED = [
    (r"a", False), (r"ab|b", False), (r"a|ab", False),
    (r"(a|ab)(c|bcd)", False),
    (r"a+", False), (r"a+?", False), (r"a+?b", False), (r"a{2,3}", False),
    (r"a{1,2}?", False),
    (r"(ab)+", False), (r"[ab]+B", False), (r"[^a]", False),
    (r"[^a\n]b", False),
    (r"a.b", False), (r"(?s)a.b", False), (r"a.*b", False), (r"a.*?b", False),
    (r"é+", False), (r"[é€]a", False), (r"😀.", False), (r".😀", False),
    (r"(?:a|é)(?P<x>b|\n)", False),
    (r"\d+", True), (r"\w+", True), (r"\s+", True), (r"(?i)ab", True),
    (r"(?i)[^a-c]+", True),
    # beyond the required list: a lazy bounded repeat inside a greedy one, a
    # scoped flag, an alternation whose later branch is longer
    (r"(?:ab??)+", False), (r"(?s:a.)b", False), (r"b|ba+|a", False),
]

# outside the span-mode scope: the empty match, a repeat over a body that can
# be empty, anchors, and what the boolean engine refuses too
EMPTY_BODY = r"[ab](?:c*|[ab]+?)*"
SPAN_UNSUPPORTED = [r"a*", r"x?", r"(?:a|)b?", r"(a*)+b", EMPTY_BODY,
                    r"^a", r"a$", r"a\Z", r"\bab", r"(a)\1", r"a(?=b)",
                    rc.STATE_BOMB]


# The shared corpora have no `d` and seldom a `c`, so `(a|ab)(c|bcd)` never
# takes its second branch there and never matches twice in a row.  These
# rows (all ASCII) are added to both corpora wherever spans are compared.
EXTRA_ROWS = ["abcd", "abcdabc", "acabcd", "abcdac x abcd", "abbcd", "ab\ncd",
              "abc", "dcba"]


def byte_spans(rx, v: str) -> list:
    """`re.finditer` spans of one value, as offsets into its UTF-8 bytes."""
    out = []
    for m in rx.finditer(v):
        a, b = m.span()
        out.append((len(v[:a].encode()), len(v[:b].encode())))
    return out


def o_spans(values, pattern):
    rx = re.compile(pattern)
    return [None if v is None else byte_spans(rx, v) for v in values]


def _map(values, f):
    return [None if v is None else f(v) for v in values]


def o_count(values, pattern):
    rx = re.compile(pattern)
    return _map(values, lambda v: len(rx.findall(v)))


def o_extract(values, pattern, group=0):
    rx = re.compile(pattern)

    def one(v):
        m = rx.search(v)
        return m.group(group) if m else None
    return _map(values, one)


def o_extract_all(values, pattern, group=0):
    rx = re.compile(pattern)
    return _map(values, lambda v: [m.group(group) for m in rx.finditer(v)])


def o_replace(values, pattern, replacement):
    rx = re.compile(pattern)
    return _map(values, lambda v: rx.sub(replacement, v))


def o_split(values, pattern):
    rx = re.compile(pattern)
    return _map(values, rx.split)


def list_offsets(lists) -> list:
    """Arrow list offsets of a column of lists (a null row holds nothing)."""
    off = [0]
    for v in lists:
        off.append(off[-1] + (0 if v is None else len(v)))
    return off


@functools.lru_cache(maxsize=None)
def raw_spans(n: int, ascii_only: bool, pattern: str) -> tuple:
    """Per row of `rc.raw_values(n, ascii_only)`, its byte spans."""
    return tuple(tuple(s) for s in
                 o_spans(rc.raw_values(n, ascii_only), pattern))


# ---------------------------------------------------------------------------
# random patterns for the property test
# ---------------------------------------------------------------------------

ATOMS = ["a", "b", "c", ".", "[ab]", "[^a]", "é"]
QUANTIFIERS = ["*", "+", "?", "*?", "+?", "??", "{2}", "{1,2}", "{0,2}?"]
TEXT_ALPHABET = "abc\né"
MAX_DEPTH = 4


def random_pattern(rng: random.Random, depth: int = 1) -> str:
    r = rng.random()
    if depth >= MAX_DEPTH or r < 0.3:
        return rng.choice(ATOMS)
    if r < 0.5:
        return random_pattern(rng, depth + 1) + random_pattern(rng, depth + 1)
    if r < 0.65:
        return "(?:" + random_pattern(rng, depth + 1) + "|" + \
            random_pattern(rng, depth + 1) + ")"
    if r < 0.9:
        return "(?:" + random_pattern(rng, depth + 1) + ")" + \
            rng.choice(QUANTIFIERS)
    return "(" + random_pattern(rng, depth + 1) + ")"


def random_text(rng: random.Random) -> str:
    return "".join(rng.choice(TEXT_ALPHABET)
                   for _ in range(rng.randrange(0, 13)))

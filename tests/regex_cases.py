"""Patterns, corpora and `re` oracles shared by the regex-engine tests
(test_regex_dfa.py on the host table walk, test_gpu_regex.py on the HIP
kernel).  A plain helper module: no fixtures.  The oracle is Python `re` on
`str` and never calls into daft_amd."""
from __future__ import annotations

import functools
import random
import re

import strings_cases as sc

# (pattern, needs_ascii): needs_ascii exactly where the pattern uses a
# \d \w \s class or (?i)
SUPPORTED = [
    (r"a", False), (r"ab|b", False), (r"a.b", False), (r"(?s)a.b", False),
    (r"a.*b", False), (r"^a", False), (r"a$", False), (r"a\Z", False),
    (r"^$", False), (r"^a|b$", False),
    (r"[ab]+B", False), (r"[^a]", False), (r"[^a\n]b", False),
    (r"[é€]a", False), (r"é+", False), (r"😀.", False), (r".😀", False),
    (r"€a?", False),
    (r"(ab){2,3}", False), (r"a{,2}b", False), (r"(a|b)*abb", False),
    (r"a+?b", False), (r"(?:a|é)(?P<x>b|\n)", False), (r"x*", False),
    (r"(?i)ab", True), (r"(?i)[Z-a]", True), (r"(?i)[^a-c]", True),
    (r"\d+", True), (r"\w\W", True), (r"\s", True), (r"\S\s\S", True),
    (r"[\d_]x", True),
    # beyond the required list: scoped flags, a trie with several excluded
    # characters, `$` alone, nested stars
    (r"(?s:a.)b", False), (r"[^é€😀a]+$", False), (r"$", False),
    (r"(a*)*b", False), (r"(?i:A)b", True), (r"^[A-Z][a-z]+ \d{2,4}$", True),
]
# always True (every row has the empty match), so no False to look for
ALWAYS_TRUE = {r"x*", r"$"}

STATE_BOMB = r"(a|b)*a(a|b){12}"
UNSUPPORTED = [r"(a)\1", r"a(?=b)", r"(?<!a)b", r"\bab", r"(?m)^a", "a$\\n",
               r"a^b", r"[α-ω]", r"(a)(?(1)b|c)", STATE_BOMB]

LIKE_EXTRA = ["_", "__%", "%_😀", "a_b"]

_ASCII_ALPHABET = list("abcABZz019_ x.!-`[") + ["\t", "\x1c", "\n"]
_ASCII_FIXED = ["a\n", "a\n\n", "\n", "", "ab1_x", "Hello 2024",
                "Hello 2024\n", "hello 12", "A\tb", "a\x1cb", "1x", "_x",
                "xabbx", "abab", "ababab", "B", "`", "Zed 99999", "a b"]


@functools.lru_cache(maxsize=None)
def _ascii_cached(n: int, nulls: bool) -> tuple:
    rng = random.Random(77 * 1_000_003 + n)
    out = []
    for i in range(n):
        if i < len(_ASCII_FIXED) and n >= 16:
            out.append(_ASCII_FIXED[i])
            continue
        if nulls and rng.random() < 0.10:
            out.append(None)
            continue
        ln = rng.randrange(0, 21)
        v = "".join(rng.choice(_ASCII_ALPHABET) for _ in range(ln))
        if rng.random() < 0.2:
            v += "\n"
        out.append(v)
    return tuple(out)


def ascii_corpus(n: int, nulls: bool = False) -> list:
    """`n` deterministic all-ASCII values: digits, `_`, punctuation, tab,
    0x1c, both cases, a trailing newline on a fifth of them; the rows
    "a\\n", "a\\n\\n", "\\n" and "" come first."""
    return list(_ascii_cached(n, nulls))


def o_search(values, pattern):
    rx = re.compile(pattern)
    return [None if v is None else rx.search(v) is not None for v in values]


@functools.lru_cache(maxsize=None)
def raw_values(n: int, ascii_only: bool) -> tuple:
    """Null-free values: the shared corpus with nulls as empty rows, or
    the ASCII corpus."""
    if ascii_only:
        return tuple(ascii_corpus(n))
    return tuple("" if v is None else v for v in sc.corpus(n))


@functools.lru_cache(maxsize=None)
def raw_expected(n: int, ascii_only: bool, pattern: str) -> tuple:
    return tuple(o_search(raw_values(n, ascii_only), pattern))

"""Regex / LIKE pattern -> DFA tables for the device match kernel
(csrc/regex.hip).

Boolean matching only: "does the pattern match somewhere" (`search`) or
"does the whole value match" (`full`).  That needs no backtracking, so a
pattern compiles to a byte-level DFA: the standard library's own parser reads
the pattern (it is then read exactly as `re` reads it), the op tree becomes a
Thompson NFA over UTF-8 bytes, subset construction gives the DFA, and the 256
byte values collapse into equivalence classes.  Anything the translation does
not handle explicitly raises `Unsupported` and the caller stays on the host
`re` path: unknown means host, never a guess.

`Program.match_host` walks the tables in Python exactly as the kernel does;
the CPU tests hold it to `re`.

Where the pattern matches (`re.finditer` spans) is a second entry point,
`compile_spans`, further down: a forward automaton with thread priorities
and a reverse one, with `SpanProgram.spans_host` as the kernels' walk.

Columns hold valid UTF-8, so one code point is an ASCII byte or a lead byte
followed by its 1-3 continuation bytes."""
from __future__ import annotations

import functools
import re
import warnings
from typing import Dict, FrozenSet, List, Tuple

import numpy as np

try:  # Python >= 3.11
    from re import _constants as _c, _parser as _parser
except ImportError:  # Python 3.10
    import sre_constants as _c
    import sre_parse as _parser


class Unsupported(Exception):
    """The pattern (or its size) is outside what the DFA engine handles."""


# state flags, shared with csrc/regex.hip
MATCHED = 1   # sticky: the answer is True whatever follows
END = 2       # the answer is True if the input ends in this state
DEAD = 4      # no continuation can match

# Subset construction stops as soon as it has this many states.  Together
# with the byte cap below: 2048 states x 6 classes x 2 bytes is already 24 KiB.
MAX_STATES = 2048
# table + byte_class + flags.  32 KiB lets five 256-thread blocks share a
# CU's 160 KiB of LDS; one block can never have more than 64 KiB.
MAX_TABLE_BYTES = 32 * 1024
assert MAX_TABLE_BYTES <= 64 * 1024
# a{1000}-style repeats are unrolled; bound the NFA as well
MAX_NFA_NODES = 20000

_I = _c.SRE_FLAG_IGNORECASE
_S = _c.SRE_FLAG_DOTALL
_U = _c.SRE_FLAG_UNICODE


def _bit(b: int) -> int:
    return 1 << b


def _span(lo: int, hi: int) -> int:
    """Byte set lo..hi inclusive, as a 256-bit mask."""
    return ((1 << (hi - lo + 1)) - 1) << lo


_ALL = _span(0x00, 0xFF)
_ASCII = _span(0x00, 0x7F)
_CONT = _span(0x80, 0xBF)
# lead bytes by sequence length (lenient: valid UTF-8 never has C0, C1, F5+)
_LEAD = {2: _span(0xC0, 0xDF), 3: _span(0xE0, 0xEF), 4: _span(0xF0, 0xF7)}
_NL = _bit(0x0A)


def _ascii_table(rx: str) -> int:
    """ASCII membership of a category, asked of `re` itself."""
    p = re.compile(rx)
    m = 0
    for c in range(128):
        if p.fullmatch(chr(c)):
            m |= _bit(c)
    return m


_CATEGORY = {
    _c.CATEGORY_DIGIT: _ascii_table(r"\d"),
    _c.CATEGORY_NOT_DIGIT: _ascii_table(r"\D"),
    _c.CATEGORY_SPACE: _ascii_table(r"\s"),
    _c.CATEGORY_NOT_SPACE: _ascii_table(r"\S"),
    _c.CATEGORY_WORD: _ascii_table(r"\w"),
    _c.CATEGORY_NOT_WORD: _ascii_table(r"\W"),
}


def _swapcase(mask: int) -> int:
    """mask | swapcase(mask) over ASCII letters."""
    up = mask & _span(0x41, 0x5A)
    lo = mask & _span(0x61, 0x7A)
    return mask | (up << 32) | (lo >> 32)


class Program:
    """DFA tables.  `table[s, byte_class[b]]` is the state after byte `b`."""

    def __init__(self, table: np.ndarray, byte_class: np.ndarray,
                 flags: np.ndarray, start: int, needs_ascii: bool):
        self.table = table            # int16 [n_states, n_classes]
        self.byte_class = byte_class  # uint8 [256]
        self.flags = flags            # uint8 [n_states]
        self.start = start
        self.needs_ascii = needs_ascii
        self._lists = None

    @property
    def n_states(self) -> int:
        return self.table.shape[0]

    @property
    def n_classes(self) -> int:
        return self.table.shape[1]

    @property
    def nbytes(self) -> int:
        return self.table.nbytes + self.byte_class.nbytes + self.flags.nbytes

    def match_host(self, data: bytes) -> bool:
        """The kernel's walk, in Python."""
        if self._lists is None:
            self._lists = (self.table.ravel().tolist(),
                           self.byte_class.tolist(), self.flags.tolist())
        table, byte_class, flags = self._lists
        nc = self.n_classes
        s = self.start
        f = flags[s]
        for b in data:
            if f & (MATCHED | DEAD):
                break
            s = table[s * nc + byte_class[b]]
            f = flags[s]
        return bool(f & (MATCHED | END))


# ---------------------------------------------------------------------------
# Thompson NFA over bytes
# ---------------------------------------------------------------------------

class _Builder:
    def __init__(self, mode: str):
        assert mode in ("search", "full", "spans"), mode
        self.mode = mode
        self.eps: List[List[int]] = []
        self.beg: List[List[int]] = []   # epsilon only at input position 0
        self.edges: List[List[Tuple[int, int]]] = []
        self.end_acc = set()             # accepts if the input ends here
        self.sticky = -1                 # accepts whatever follows
        self.needs_ascii = False

    def new(self) -> int:
        if len(self.eps) >= MAX_NFA_NODES:
            raise Unsupported("pattern too large")
        self.eps.append([])
        self.beg.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def edge(self, s: int, mask: int, t: int) -> None:
        if mask:
            self.edges[s].append((mask, t))

    # -- pieces ------------------------------------------------------------

    def bytes_(self, s: int, data: bytes) -> int:
        for b in data:
            t = self.new()
            self.edge(s, _bit(b), t)
            s = t
        return s

    def literal(self, s: int, code: int, fl: int) -> int:
        if code < 128:
            mask = _bit(code)
            if fl & _I:
                mask = _swapcase(mask)
            t = self.new()
            self.edge(s, mask, t)
            return t
        t = self.bytes_(s, _encode(code))
        if fl & _I:
            self.edge(s, _ascii_fold(code), t)
        return t

    def charset(self, s: int, ascii_mask: int, extras: List[bytes],
                negate: bool, fl: int) -> int:
        """One code point in (or, negated, not in) ASCII set + extras."""
        if fl & _I:
            ascii_mask = _swapcase(ascii_mask)
            for seq in extras:
                ascii_mask |= _ascii_fold(ord(seq.decode("utf-8")))
        e = self.new()
        if not negate:
            self.edge(s, ascii_mask, e)
            for seq in dict.fromkeys(extras):
                self.eps[self.bytes_(s, seq)].append(e)
            return e
        self.edge(s, _ASCII & ~ascii_mask, e)
        # every multi-byte code point except `extras`: a trie of the
        # excluded sequences, everything off the trie goes to the generic
        # "k more continuation bytes" chain g[k]
        g = [e]
        for _ in range(3):
            t = self.new()
            self.edge(t, _CONT, g[-1])
            g.append(t)
        excluded = set(extras)

        def grow(node: int, prefix: bytes, allowed: int, length: int):
            k = len(prefix)
            nxt = sorted({q[k] for q in excluded
                          if len(q) == length and q[:k] == prefix})
            special = 0
            for b in nxt:
                special |= _bit(b)
                if k + 1 < length:
                    child = self.new()
                    self.edge(node, _bit(b), child)
                    grow(child, prefix + bytes([b]), _CONT, length)
            self.edge(node, allowed & ~special, g[length - k - 1])

        for length, lead in _LEAD.items():
            grow(s, b"", lead, length)
        return e

    # -- op tree -----------------------------------------------------------

    def seq(self, items, s: int, fl: int, cb: bool, ce: bool) -> int:
        items = list(items)
        last = len(items) - 1
        for i, (op, av) in enumerate(items):
            s = self.item(op, av, s, fl, cb and i == 0, ce and i == last)
        return s

    def item(self, op, av, s: int, fl: int, cb: bool, ce: bool) -> int:
        if op is _c.LITERAL:
            return self.literal(s, av, fl)
        if op is _c.NOT_LITERAL:
            return self.class_items([(_c.NEGATE, None), (_c.LITERAL, av)],
                                    s, fl)
        if op is _c.ANY:
            return self.charset(s, 0 if fl & _S else _NL, [], True, 0)
        if op is _c.IN:
            return self.class_items(av, s, fl)
        if op is _c.BRANCH:
            out = self.new()
            for alt in av[1]:
                a = self.new()
                self.eps[s].append(a)
                self.eps[self.seq(alt, a, fl, cb, ce)].append(out)
            return out
        if op is _c.SUBPATTERN:
            if len(av) != 4:
                raise Unsupported("group shape")
            _, add, dele, sub = av
            if (add | dele) & ~(_I | _S):
                raise Unsupported("scoped flag")
            if add & _I:
                self.needs_ascii = True
            return self.seq(sub, s, (fl | add) & ~dele, False, False)
        if (op is _c.MAX_REPEAT or op is _c.MIN_REPEAT) and \
                self.mode == "spans":
            return self.repeat_ordered(op is _c.MAX_REPEAT, av, s, fl)
        if op is _c.MAX_REPEAT or op is _c.MIN_REPEAT:
            # lazy and greedy agree on whether a match exists
            lo, hi, sub = av
            for _ in range(lo):
                s = self.seq(sub, s, fl, False, False)
            out = self.new()
            self.eps[s].append(out)
            if hi == _c.MAXREPEAT:
                self.eps[self.seq(sub, out, fl, False, False)].append(out)
            else:
                for _ in range(hi - lo):
                    s = self.seq(sub, s, fl, False, False)
                    self.eps[s].append(out)
            return out
        if op is _c.AT and self.mode == "spans":
            raise Unsupported("anchor in span mode")
        if op is _c.AT:
            if av in (_c.AT_BEGINNING, _c.AT_BEGINNING_STRING):
                if not cb:
                    raise Unsupported("^ not at the start of an alternative")
                t = self.new()
                self.beg[s].append(t)
                return t
            if av in (_c.AT_END, _c.AT_END_STRING):
                if not ce:
                    raise Unsupported("$ not at the end of an alternative")
                m = self.new()
                self.end_acc.add(m)
                self.eps[s].append(m)
                if av is _c.AT_END and self.mode == "search":
                    self.edge(s, _NL, m)    # `$` is `\n?` + end of input
                return self.new()           # nothing follows: unreachable
        raise Unsupported(f"opcode {op}")

    def repeat_ordered(self, greedy: bool, av, s: int, fl: int) -> int:
        """Span mode: the order of a node's epsilon edges is thread
        priority.  A greedy repeat tries its body before its exit, a lazy
        one its exit before its body."""
        lo, hi, sub = av
        if _can_be_empty(sub):
            # sre ends a repeat on an empty iteration; the automaton has no
            # such rule
            raise Unsupported("repeat whose body can match the empty string")
        for _ in range(lo):
            s = self.seq(sub, s, fl, False, False)
        out = self.new()
        if hi == _c.MAXREPEAT:
            loop = self.new()
            body = self.new()
            self.eps[s].append(loop)
            self.eps[loop] += [body, out] if greedy else [out, body]
            self.eps[self.seq(sub, body, fl, False, False)].append(loop)
            return out
        for _ in range(hi - lo):
            body = self.new()
            self.eps[s] += [body, out] if greedy else [out, body]
            s = self.seq(sub, body, fl, False, False)
        self.eps[s].append(out)
        return out

    def class_items(self, items, s: int, fl: int) -> int:
        negate = False
        mask = 0
        extras: List[bytes] = []
        for j, (op, av) in enumerate(items):
            if op is _c.NEGATE and j == 0:
                negate = True
            elif op is _c.LITERAL:
                if av < 128:
                    mask |= _bit(av)
                else:
                    extras.append(_encode(av))
            elif op is _c.RANGE:
                lo, hi = av
                if hi >= 128:
                    raise Unsupported("range with a non-ASCII endpoint")
                mask |= _span(lo, hi)
            elif op is _c.CATEGORY:
                if av not in _CATEGORY:
                    raise Unsupported(f"category {av}")
                # ASCII rows only: the caller checks the column
                self.needs_ascii = True
                mask |= _CATEGORY[av]
            else:
                raise Unsupported(f"class item {op}")
        return self.charset(s, mask, extras, negate, fl)

    # -- subset construction -----------------------------------------------

    def finish(self, start: int) -> Program:
        n = len(self.eps)
        masks = sorted({m for es in self.edges for m, _ in es})
        sig: Dict[tuple, int] = {}
        byte_class = np.zeros(256, dtype=np.uint8)
        reps: List[int] = []
        for b in range(256):
            key = tuple((m >> b) & 1 for m in masks)
            if key not in sig:
                sig[key] = len(reps)
                reps.append(b)
            byte_class[b] = sig[key]
        ncls = len(reps)
        mask_classes = {m: [c for c, b in enumerate(reps) if (m >> b) & 1]
                        for m in masks}

        closures: List = [None] * n

        def closure(node: int, at_start: bool = False) -> FrozenSet[int]:
            if not at_start and closures[node] is not None:
                return closures[node]
            seen = {node}
            stack = [node]
            while stack:
                x = stack.pop()
                for y in (self.eps[x] + self.beg[x]) if at_start \
                        else self.eps[x]:
                    if y not in seen:
                        seen.add(y)
                        stack.append(y)
            out = frozenset(seen)
            if not at_start:
                closures[node] = out
            return out

        moves: List = [None] * n

        def move(node: int) -> Dict[int, FrozenSet[int]]:
            if moves[node] is None:
                acc: Dict[int, set] = {}
                for m, t in self.edges[node]:
                    ct = closure(t)
                    for c in mask_classes[m]:
                        acc.setdefault(c, set()).update(ct)
                moves[node] = {c: frozenset(v) for c, v in acc.items()}
            return moves[node]

        matched_key = frozenset([self.sticky])

        def canon(nodes) -> FrozenSet[int]:
            # once matched, always matched: one absorbing state
            return matched_key if self.sticky in nodes else frozenset(nodes)

        first = canon(closure(start, at_start=True))
        ids = {first: 0}
        order = [first]
        rows: List[List[int]] = []
        i = 0
        while i < len(order):
            cur = order[i]
            if cur == matched_key:
                rows.append([i] * ncls)
                i += 1
                continue
            row = []
            node_moves = [move(x) for x in cur]
            for c in range(ncls):
                tgt = set()
                for mv in node_moves:
                    t = mv.get(c)
                    if t:
                        tgt |= t
                key = canon(tgt)
                j = ids.get(key)
                if j is None:
                    if len(order) >= MAX_STATES:
                        raise Unsupported(
                            f"more than {MAX_STATES} DFA states")
                    j = ids[key] = len(order)
                    order.append(key)
                row.append(j)
            rows.append(row)
            i += 1

        table = np.asarray(rows, dtype=np.int16).reshape(len(order), ncls)
        accept = np.array([st == matched_key or not self.end_acc.isdisjoint(st)
                           for st in order], dtype=bool)
        # MATCHED: no rejecting state can be reached; DEAD: no accepting one
        matched = ~_reaches(table, ~accept)
        dead = ~_reaches(table, accept)
        flags = (matched * MATCHED + accept * END + dead * DEAD) \
            .astype(np.uint8)

        # bytes that no DFA state tells apart share a class
        cols, inverse = np.unique(table.T, axis=0, return_inverse=True)
        table = np.ascontiguousarray(cols.T)
        byte_class = inverse.reshape(-1).astype(np.uint8)[byte_class]
        prog = Program(table, byte_class, flags, 0, self.needs_ascii)
        if prog.nbytes > MAX_TABLE_BYTES:
            raise Unsupported(f"tables need {prog.nbytes} bytes, "
                              f"limit {MAX_TABLE_BYTES}")
        return prog


def _reaches(table: np.ndarray, target: np.ndarray) -> np.ndarray:
    """Per state: is a state of `target` reachable (in >= 0 steps)?"""
    reach = target.copy()
    while True:
        nxt = reach | reach[table].any(axis=1)
        if (nxt == reach).all():
            return reach
        reach = nxt


@functools.lru_cache(maxsize=None)
def _ascii_fold(code: int) -> int:
    """ASCII characters that a non-ASCII literal matches under IGNORECASE
    (`ſ` matches `s`), asked of `re` itself.  Its non-ASCII case variants
    are not looked for: IGNORECASE programs are `needs_ascii`."""
    p = re.compile(re.escape(chr(code)), re.IGNORECASE)
    m = 0
    for c in range(128):
        if p.fullmatch(chr(c)):
            m |= _bit(c)
    return m


def _encode(code: int) -> bytes:
    try:
        return chr(code).encode("utf-8")
    except UnicodeEncodeError:
        raise Unsupported("literal that is not a Unicode scalar value")


# ---------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------

def _parse(pattern: str, flags: int):
    """(op tree, global flags) as `re` itself reads the pattern."""
    if not isinstance(pattern, str):
        raise Unsupported("bytes pattern")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            tree = _parser.parse(pattern, flags)
    except (re.error, Warning, RecursionError, OverflowError) as e:
        raise Unsupported(f"parser: {e}")
    gflags = tree.state.flags
    if gflags & ~(_I | _S | _U):
        raise Unsupported("flag")
    return tree, gflags


def _build_regex(pattern: str, mode: str, flags: int) -> Program:
    tree, gflags = _parse(pattern, flags)
    b = _Builder(mode)
    if gflags & _I:
        b.needs_ascii = True
    top = b.new()
    if mode == "search":
        b.edge(top, _ALL, top)      # the match may start at any position
    first = b.new()
    b.eps[top].append(first)
    last = b.seq(tree, first, gflags & (_I | _S), True, True)
    fin = b.new()
    b.eps[last].append(fin)
    if mode == "search":
        b.sticky = fin
    else:
        b.end_acc.add(fin)
    return b.finish(top)


def _build_like(pattern: str, ci: bool) -> Program:
    b = _Builder("full")
    b.needs_ascii = bool(ci)
    fl = _I if ci else 0
    s = top = b.new()
    for ch in pattern:
        if ch == "%":           # any run of bytes, `\n` included
            t = b.new()
            b.eps[s].append(t)
            b.edge(t, _ALL, t)
            s = t
        elif ch == "_":         # one code point, `\n` included
            s = b.charset(s, 0, [], True, 0)
        else:
            s = b.literal(s, ord(ch), fl)
    b.end_acc.add(s)
    return b.finish(top)


def _cached(build):
    """lru_cache that also remembers `Unsupported` (a pattern that hits the
    state cap is not compiled again on every call)."""
    @functools.lru_cache(maxsize=256)
    def inner(*key):
        try:
            return build(*key)
        except Unsupported as e:
            return Unsupported(*e.args)

    @functools.wraps(build)
    def outer(*key):
        res = inner(*key)
        if isinstance(res, Unsupported):
            raise Unsupported(*res.args)    # fresh: no traceback kept alive
        return res
    outer.cache_clear = inner.cache_clear
    return outer


_compile_cached = _cached(_build_regex)
_like_cached = _cached(_build_like)


# ---------------------------------------------------------------------------
# match spans: where the pattern matches, as `re.finditer` reports it
# ---------------------------------------------------------------------------
#
# Two automata, as in RE2.  The forward one keeps its NFA threads in priority
# order and finds where the leftmost-first match ends; the reverse one is a
# plain subset construction over the reversed NFA and finds where that match
# starts.  Scope (everything else raises `Unsupported`): the pattern cannot
# match the empty string, no repeat body can match the empty string (sre
# ends a repeat on an empty iteration, an automaton does not), and no
# anchors (a conditional accept does not compose with the priority cut).

SPAN_MATCH = 1  # forward: a match ends on entering; reverse: one starts here


def _can_be_empty(items) -> bool:
    """Can this op sequence match the empty string?  Unknown ops raise."""
    for op, av in items:
        if op in (_c.LITERAL, _c.NOT_LITERAL, _c.ANY, _c.IN):
            return False
        if op is _c.BRANCH:
            if not any(_can_be_empty(a) for a in av[1]):
                return False
        elif op is _c.SUBPATTERN:
            if len(av) != 4:
                raise Unsupported("group shape")
            if not _can_be_empty(av[3]):
                return False
        elif op is _c.MAX_REPEAT or op is _c.MIN_REPEAT:
            if av[0] > 0 and not _can_be_empty(av[2]):
                return False
        else:
            raise Unsupported(f"opcode {op}")
    return True


class SpanProgram:
    """Forward (priority) and reverse DFA tables over one byte-class map.
    `fwd_table[s, byte_class[b]]` / `rev_table[...]` is the state after
    byte `b`; both start in state 0."""

    def __init__(self, fwd_table: np.ndarray, fwd_flags: np.ndarray,
                 rev_table: np.ndarray, rev_flags: np.ndarray,
                 byte_class: np.ndarray, needs_ascii: bool, n_groups: int):
        self.fwd_table = fwd_table    # int16 [n_fwd_states, n_classes]
        self.fwd_flags = fwd_flags    # uint8: SPAN_MATCH | DEAD
        self.rev_table = rev_table    # int16 [n_rev_states, n_classes]
        self.rev_flags = rev_flags    # uint8: SPAN_MATCH | DEAD
        self.byte_class = byte_class  # uint8 [256], shared
        self.start = 0
        self.rev_start = 0
        self.needs_ascii = needs_ascii
        self.n_groups = n_groups      # capturing groups in the pattern
        self._lists = None

    @property
    def n_classes(self) -> int:
        return self.fwd_table.shape[1]

    @property
    def nbytes(self) -> int:
        return (self.fwd_table.nbytes + self.rev_table.nbytes +
                self.byte_class.nbytes + self.fwd_flags.nbytes +
                self.rev_flags.nbytes)

    def _walk(self, data: bytes, limit: int, starts: bool) -> list:
        """The kernels' walk, in Python: ends, or (start, end) pairs."""
        if self._lists is None:
            self._lists = (self.fwd_table.ravel().tolist(),
                           self.fwd_flags.tolist(),
                           self.rev_table.ravel().tolist(),
                           self.rev_flags.tolist(),
                           self.byte_class.tolist())
        ft, ff, rt, rf, cls = self._lists
        nc = self.n_classes
        out = []
        p, b = 0, len(data)
        while p < b and len(out) != limit:
            s = self.start
            last = -1
            for q in range(p, b):
                s = ft[s * nc + cls[data[q]]]
                f = ff[s]
                if f & SPAN_MATCH:
                    last = q + 1
                if f & DEAD:
                    break
            if last < 0:
                break
            if starts:
                s = self.rev_start
                first = last
                for q in range(last - 1, p - 1, -1):
                    s = rt[s * nc + cls[data[q]]]
                    f = rf[s]
                    if f & SPAN_MATCH:
                        first = q
                    if f & DEAD:
                        break
                out.append((first, last))
            else:
                out.append(last)
            p = last
        return out

    def spans_host(self, data: bytes, limit: int = -1) -> list:
        """Byte spans of the first `limit` matches (all when -1)."""
        return self._walk(data, limit, True)

    def count_host(self, data: bytes, limit: int = -1) -> int:
        return len(self._walk(data, limit, False))


def _build_spans(pattern: str, flags: int) -> SpanProgram:
    tree, gflags = _parse(pattern, flags)
    if _can_be_empty(tree):
        raise Unsupported("pattern can match the empty string")
    b = _Builder("spans")
    if gflags & _I:
        b.needs_ascii = True
    first = b.new()
    fin = b.new()
    b.eps[b.seq(tree, first, gflags & (_I | _S), False, False)].append(fin)
    n = len(b.eps)
    if any(b.beg[x] or (b.eps[x] and b.edges[x]) for x in range(n)) or \
            b.eps[fin] or b.edges[fin] or b.end_acc:
        raise Unsupported("NFA shape")      # priority would be ambiguous

    masks = sorted({m for es in b.edges for m, _ in es})
    sig: Dict[tuple, int] = {}
    byte_class = np.zeros(256, dtype=np.uint8)
    reps: List[int] = []
    for byte in range(256):
        key = tuple((m >> byte) & 1 for m in masks)
        if key not in sig:
            sig[key] = len(reps)
            reps.append(byte)
        byte_class[byte] = sig[key]
    ncls = len(reps)
    mask_classes = {m: [c for c, r in enumerate(reps) if (m >> r) & 1]
                    for m in masks}

    # -- forward: ordered thread lists ---------------------------------------
    oclosures: Dict[int, tuple] = {}

    def oclosure(node: int) -> tuple:
        """Nodes with byte edges (and `fin`) reachable by epsilon moves, in
        priority order: depth first, a node's epsilon edges in order."""
        got = oclosures.get(node)
        if got is None:
            out, seen, stack = [], set(), [node]
            while stack:
                x = stack.pop()
                if x in seen:
                    continue
                seen.add(x)
                if x == fin or b.edges[x]:
                    out.append(x)
                stack.extend(reversed(b.eps[x]))
            got = oclosures[node] = tuple(out)
        return got

    omoves: Dict[int, Dict[int, tuple]] = {}

    def omove(node: int) -> Dict[int, tuple]:
        got = omoves.get(node)
        if got is None:
            acc: Dict[int, list] = {}
            for m, t in b.edges[node]:
                ct = oclosure(t)
                for c in mask_classes[m]:
                    lst = acc.setdefault(c, [])
                    lst.extend(x for x in ct if x not in lst)
            got = omoves[node] = {c: tuple(v) for c, v in acc.items()}
        return got

    restart = oclosure(first)
    # state: (threads in priority order, a match was seen, one ends here)
    first_key = (restart, False, False)
    ids = {first_key: 0}
    order = [first_key]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        threads, seen_match, _ = order[i]
        node_moves = [omove(x) for x in threads]
        row = []
        for c in range(ncls):
            nxt: List[int] = []
            have = set()
            for mv in node_moves:
                for x in mv.get(c, ()):
                    if x not in have:
                        have.add(x)
                        nxt.append(x)
            if not seen_match:
                # the search is unanchored until its first match: a new
                # thread starts here, below every running one
                nxt.extend(x for x in restart if x not in have)
            hit = fin in nxt
            if hit:
                nxt = nxt[:nxt.index(fin)]  # lower priorities lose
            key = (tuple(nxt), seen_match or hit, hit)
            j = ids.get(key)
            if j is None:
                if len(order) >= MAX_STATES:
                    raise Unsupported(f"more than {MAX_STATES} DFA states")
                j = ids[key] = len(order)
                order.append(key)
            row.append(j)
        rows.append(row)
        i += 1
    fwd = np.asarray(rows, dtype=np.int16).reshape(len(order), ncls)
    fwd_hit = np.array([k[2] for k in order], dtype=bool)
    fwd_flags = (fwd_hit * SPAN_MATCH + ~_reaches(fwd, fwd_hit) * DEAD) \
        .astype(np.uint8)

    # -- reverse: subset construction over the reversed NFA ------------------
    reps_of: List[List[int]] = [[] for _ in range(n)]
    redges: List[List[Tuple[int, int]]] = [[] for _ in range(n)]
    for x in range(n):
        for y in b.eps[x]:
            reps_of[y].append(x)
        for m, t in b.edges[x]:
            redges[t].append((m, x))

    def rclosure(nodes) -> FrozenSet[int]:
        seen = set(nodes)
        stack = list(seen)
        while stack:
            x = stack.pop()
            for y in reps_of[x]:
                if y not in seen:
                    seen.add(y)
                    stack.append(y)
        return frozenset(seen)

    r0 = rclosure([fin])
    rids = {r0: 0}
    rorder = [r0]
    rrows: List[List[int]] = []
    i = 0
    while i < len(rorder):
        acc: List[set] = [set() for _ in range(ncls)]
        for x in rorder[i]:
            for m, t in redges[x]:
                for c in mask_classes[m]:
                    acc[c].add(t)
        row = []
        for c in range(ncls):
            key = rclosure(acc[c])
            j = rids.get(key)
            if j is None:
                if len(rorder) >= MAX_STATES:
                    raise Unsupported(f"more than {MAX_STATES} DFA states")
                j = rids[key] = len(rorder)
                rorder.append(key)
            row.append(j)
        rrows.append(row)
        i += 1
    rev = np.asarray(rrows, dtype=np.int16).reshape(len(rorder), ncls)
    rev_hit = np.array([first in st for st in rorder], dtype=bool)
    rev_flags = (rev_hit * SPAN_MATCH + ~_reaches(rev, rev_hit) * DEAD) \
        .astype(np.uint8)

    # bytes that no state of either automaton tells apart share a class
    cols, inverse = np.unique(np.concatenate([fwd, rev]).T, axis=0,
                              return_inverse=True)
    both = np.ascontiguousarray(cols.T)
    byte_class = inverse.reshape(-1).astype(np.uint8)[byte_class]
    prog = SpanProgram(np.ascontiguousarray(both[:len(order)]), fwd_flags,
                       np.ascontiguousarray(both[len(order):]), rev_flags,
                       byte_class, b.needs_ascii, tree.state.groups - 1)
    if prog.nbytes > MAX_TABLE_BYTES:
        raise Unsupported(f"tables need {prog.nbytes} bytes, "
                          f"limit {MAX_TABLE_BYTES}")
    return prog


_spans_cached = _cached(_build_spans)


def compile(pattern: str, mode: str = "search", flags: int = 0) -> Program:
    """DFA for `re.search` (mode "search") or `re.fullmatch` (mode "full")
    of `pattern`; raises `Unsupported`.  Cached on (pattern, mode, flags)."""
    if mode not in ("search", "full"):
        raise ValueError(f"mode must be 'search' or 'full', got {mode!r}")
    return _compile_cached(pattern, mode, int(flags))


def compile_spans(pattern: str, flags: int = 0) -> SpanProgram:
    """Tables that give the `re.finditer` spans of `pattern`; raises
    `Unsupported` outside the span-mode scope.  Cached on (pattern, flags)."""
    return _spans_cached(pattern, int(flags))


def like_program(pattern: str, ci: bool = False) -> Program:
    """DFA for SQL LIKE / ILIKE: `%` any run, `_` one code point, the rest
    literal, the whole value must match.  Built from the LIKE pattern
    itself, not through regex source text."""
    return _like_cached(pattern, bool(ci))

"""String kernels over Arrow offsets+bytes layout (ref capability:
/root/reference/src/daft-functions-utf8/src/*.rs — 45 kernels; the hot
predicates run as HIP kernels over offsets+bytes on GPU, CPU falls back to
python/numpy for the test tier)."""
from __future__ import annotations

import functools
import re
import unicodedata
from typing import List, Optional

import numpy as np
import torch

from ..schema import DataType, TypeKind
from ..series import Series
from . import _is_gpu, native_required, regex_dfa


def _bytes_tensor(pat: bytes, device) -> torch.Tensor:
    return torch.frombuffer(bytearray(pat), dtype=torch.uint8).to(device) \
        if pat else torch.zeros(0, dtype=torch.uint8, device=device)


def _pylist_str(s: Series) -> list:
    return s.to_pylist()


def _bool_out(s: Series, data: torch.Tensor) -> Series:
    return Series(s.name, DataType.bool(), data=data, validity=s.validity)


def _dict_pred(s: Series, fn) -> Optional[Series]:
    """Dictionary fast path for predicates: evaluate on the vocab, gather the
    boolean by codes."""
    if not s.is_dict():
        return None
    vres = fn(s.children[0])
    out = vres.data[s.data.to(torch.int64)]
    return Series(s.name, DataType.bool(), data=out, validity=s.validity)


def _dict_map(s: Series, fn) -> Optional[Series]:
    """Dictionary fast path for string->string maps: transform the vocab."""
    if not s.is_dict():
        return None
    vres = fn(s.children[0])
    return Series.make_dict(s.name, vres, s.data, s.validity)


# --- predicates -----------------------------------------------------------

def contains(s: Series, pat: str) -> Series:
    d = _dict_pred(s, lambda v: contains(v, pat))
    if d is not None:
        return d
    if _is_gpu(s):
        p = _bytes_tensor(pat.encode(), s.device)
        return _bool_out(s, native_required().str_find(
            s.offsets, s.data, p, 0) >= 0)
    vals = _pylist_str(s)
    out = torch.tensor([False if v is None else pat in v for v in vals],
                       dtype=torch.bool)
    return _bool_out(s, out)


def startswith(s: Series, pat: str) -> Series:
    d = _dict_pred(s, lambda v: startswith(v, pat))
    if d is not None:
        return d
    if _is_gpu(s):
        p = _bytes_tensor(pat.encode(), s.device)
        return _bool_out(s, native_required().str_find(
            s.offsets, s.data, p, 1) >= 0)
    vals = _pylist_str(s)
    out = torch.tensor([False if v is None else v.startswith(pat)
                        for v in vals], dtype=torch.bool)
    return _bool_out(s, out)


def endswith(s: Series, pat: str) -> Series:
    d = _dict_pred(s, lambda v: endswith(v, pat))
    if d is not None:
        return d
    if _is_gpu(s):
        p = _bytes_tensor(pat.encode(), s.device)
        return _bool_out(s, native_required().str_find(
            s.offsets, s.data, p, 2) >= 0)
    vals = _pylist_str(s)
    out = torch.tensor([False if v is None else v.endswith(pat)
                        for v in vals], dtype=torch.bool)
    return _bool_out(s, out)


def like(s: Series, pattern: str, case_insensitive: bool = False) -> Series:
    """SQL LIKE: % = any run, _ = any single char.

    Patterns without `_` (every TPC-H LIKE) run as a single ordered
    multi-substring HIP kernel on GPU; patterns with `_` and ILIKE run the
    DFA kernel on GPU (csrc/regex.hip), or a host regex pass where that
    does not apply."""
    d = _dict_pred(s, lambda v: like(v, pattern, case_insensitive))
    if d is not None:
        return d
    if "_" not in pattern and not case_insensitive:
        parts = pattern.split("%")
        if len(parts) == 1:
            return _eq_literal(s, pattern, case_insensitive)
        if _is_gpu(s):
            anchored_prefix = bool(parts[0])
            anchored_suffix = bool(parts[-1])
            needles = [p for p in parts if p]
            blob = b"".join(p.encode() for p in needles)
            lens = torch.tensor([len(p.encode()) for p in needles],
                                dtype=torch.int64, device=s.device)
            out = native_required().str_like(
                s.offsets, s.data, _bytes_tensor(blob, s.device), lens,
                anchored_prefix, anchored_suffix)
            return _bool_out(s, out)
        # CPU fast path: ordered substring scan
        vals = _pylist_str(s)
        ap, asfx = bool(parts[0]), bool(parts[-1])
        needles = [p for p in parts if p]
        out = torch.tensor(
            [False if v is None else _ordered_match(v, needles, ap, asfx)
             for v in vals], dtype=torch.bool)
        return _bool_out(s, out)
    return _like_general(s, pattern, case_insensitive)


def _ordered_match(v: str, needles: List[str], anchored_prefix: bool,
                   anchored_suffix: bool) -> bool:
    if not needles:
        return True
    pos = 0
    for i, nd in enumerate(needles):
        if i == 0 and anchored_prefix:
            if not v.startswith(nd):
                return False
            pos = len(nd)
            continue
        if i == len(needles) - 1 and anchored_suffix:
            return len(v) - pos >= len(nd) and v.endswith(nd) and \
                (v.rfind(nd) >= pos)
        j = v.find(nd, pos)
        if j < 0:
            return False
        pos = j + len(nd)
    return True


def _eq_literal(s: Series, value: str, ci: bool) -> Series:
    if ci:
        return _like_general(s, value, True)
    from . import compare_op
    lit = Series.from_pylist(s.name, [value], DataType.string(),
                             device=s.device)
    return compare_op(s, lit.broadcast(len(s)), "eq")


def _host_regex_pred(s: Series, rx, full: bool) -> Series:
    """Host path of every regex predicate: one `re` call per row."""
    hit = rx.fullmatch if full else rx.search
    vals = _pylist_str(s.cpu())
    out = torch.tensor([False if v is None else hit(v) is not None
                        for v in vals], dtype=torch.bool).to(s.device)
    return _bool_out(s, out)


@functools.lru_cache(maxsize=64)
def _device_tables(prog, device: str):
    return tuple(torch.from_numpy(a).to(device)
                 for a in (prog.table, prog.byte_class, prog.flags))


def _device_dfa_pred(s: Series, pattern: str, build) -> Optional[Series]:
    """Run `build()`'s DFA over a device column with the HIP kernel.  None
    when the column is not on the device, the pattern is outside the DFA
    engine, or the program is ASCII-only and pattern or column is not."""
    if not _is_gpu(s):
        return None
    try:
        prog = build()
    except regex_dfa.Unsupported:
        return None
    if prog.needs_ascii and not (pattern.isascii() and _all_ascii(s)):
        return None
    table, byte_class, flags = _device_tables(prog, str(s.device))
    out = native_required().regex_match(
        s.offsets, s.data, table, byte_class, flags, prog.n_classes,
        prog.start)
    return _bool_out(s, out)


def _like_general(s: Series, pattern: str, ci: bool) -> Series:
    """LIKE with `_`, and every ILIKE: DFA kernel on the device, else the
    host regex."""
    d = _device_dfa_pred(s, pattern,
                         lambda: regex_dfa.like_program(pattern, ci))
    return d if d is not None else _like_regex(s, pattern, ci)


def _like_regex(s: Series, pattern: str, ci: bool) -> Series:
    # `%` and `_` match newlines too, and the whole value must match
    rx = re.escape(pattern).replace("%", ".*").replace("_", ".")
    rx = re.compile(rx, re.DOTALL | (re.IGNORECASE if ci else 0))
    return _host_regex_pred(s, rx, True)


def regexp_match(s: Series, pattern: str) -> Series:
    """`re.search` semantics.  Device columns run the DFA kernel where the
    pattern compiles to one (see regex_dfa.py); everything else is `re`."""
    d = _dict_pred(s, lambda v: regexp_match(v, pattern))
    if d is not None:
        return d
    d = _device_dfa_pred(s, pattern,
                         lambda: regex_dfa.compile(pattern, "search"))
    if d is not None:
        return d
    return _host_regex_pred(s, re.compile(pattern), False)


# --- regex match positions: count / extract / replace / split ---------------
#
# Device columns whose pattern compiles to a span program (regex_dfa.py
# compile_spans) stay on the device: count matches per row, scan, write the
# spans, turn them into byte segments with index arithmetic and copy those
# with one ragged-copy kernel.  Everything else (CPU columns, patterns
# outside the span scope, ASCII-only programs over non-ASCII data, capture
# groups, replacement templates) takes the `_host_regexp_*` helper: one `re`
# call per row.

_LIST_OF_STRING = DataType.list(DataType.string())


def _host_rows(s: Series, f, dtype) -> Series:
    vals = s.cpu().to_pylist()
    out = [None if v is None else f(v) for v in vals]
    r = Series.from_pylist(s.name, out, dtype)
    return r.to(s.device) if s.is_gpu() else r


def _host_regexp_count(s: Series, pattern: str) -> Series:
    p = re.compile(pattern)
    return _host_rows(s, lambda v: len(p.findall(v)), DataType.int64())


def _host_regexp_extract(s: Series, pattern: str, group: int) -> Series:
    p = re.compile(pattern)

    def one(v):
        m = p.search(v)
        return m.group(group) if m else None
    return _host_rows(s, one, DataType.string())


def _host_regexp_extract_all(s: Series, pattern: str, group: int) -> Series:
    p = re.compile(pattern)
    return _host_rows(s, lambda v: [m.group(group) for m in p.finditer(v)],
                      _LIST_OF_STRING)


def _host_regexp_replace(s: Series, pattern: str, replacement: str) -> Series:
    p = re.compile(pattern)
    return _host_rows(s, lambda v: p.sub(replacement, v), DataType.string())


def _host_regexp_split(s: Series, pattern: str) -> Series:
    p = re.compile(pattern)
    return _host_rows(s, p.split, _LIST_OF_STRING)


@functools.lru_cache(maxsize=64)
def _span_tables(prog, device: str):
    return tuple(torch.from_numpy(a).to(device)
                 for a in (prog.fwd_table, prog.byte_class, prog.fwd_flags,
                           prog.rev_table, prog.rev_flags))


def _span_program(s: Series, pattern: str):
    """The span program for a device column (for a dictionary column: for
    its vocab), or None when the call belongs on the host."""
    if not _is_gpu(s) or not isinstance(pattern, str):
        return None
    try:
        prog = regex_dfa.compile_spans(pattern)
    except regex_dfa.Unsupported:
        return None
    strings = s.children[0] if s.is_dict() else s
    if prog.needs_ascii and not (pattern.isascii() and _all_ascii(strings)):
        return None
    return prog


def _device_counts(s: Series, prog, limit: int) -> torch.Tensor:
    fwd, cls, fflags, _, _ = _span_tables(prog, str(s.device))
    return native_required().regex_count(
        s.offsets, s.data, s.validity, fwd, cls, fflags, prog.n_classes,
        prog.start, limit)


def _device_spans(s: Series, prog, limit: int):
    """(counts [n], match_offsets [n + 1], starts [m], ends [m]); starts and
    ends are absolute positions in `s.data`."""
    counts = _device_counts(s, prog, limit)
    mo = torch.zeros(len(s) + 1, dtype=torch.int64, device=s.device)
    torch.cumsum(counts, 0, out=mo[1:])
    fwd, cls, fflags, rev, rflags = _span_tables(prog, str(s.device))
    starts, ends = native_required().regex_spans(
        s.offsets, s.data, s.validity, fwd, cls, fflags, prog.n_classes,
        prog.start, rev, rflags, prog.rev_start, mo, limit)
    return counts, mo, starts, ends


def _copy_strings(src: torch.Tensor, seg_start: torch.Tensor,
                  seg_len: torch.Tensor):
    """(offsets [k + 1], bytes) of the segments, copied in order."""
    off = torch.zeros(seg_len.numel() + 1, dtype=torch.int64,
                      device=src.device)
    torch.cumsum(seg_len, 0, out=off[1:])
    return off, native_required().copy_segments(
        src, seg_start.contiguous(), off)


def _gaps(s: Series, counts, mo, starts, ends):
    """The text around the matches.  Per match, (row, rank in its row, where
    the gap before it starts); per row, where the gap after its last match
    starts."""
    n, m = len(s), starts.numel()
    dev = s.device
    row = torch.repeat_interleave(
        torch.arange(n, dtype=torch.int64, device=dev), counts,
        output_size=m)
    j = torch.arange(m, dtype=torch.int64, device=dev)
    rank = j - mo[row]
    ends_p = torch.cat([ends.new_zeros(1), ends])     # ends_p[j] = ends[j-1]
    before = torch.where(rank == 0, s.offsets[row], ends_p[:-1])
    tail = torch.where(counts > 0, ends_p[mo[1:]], s.offsets[:-1])
    return row, rank, before, tail


def regexp_count(s: Series, pattern: str) -> Series:
    """Non-overlapping matches per row (`len(re.findall)`)."""
    prog = _span_program(s, pattern)
    if prog is None:
        return _host_regexp_count(s, pattern)
    validity = s.validity
    if s.is_dict():
        vocab = s.children[0]
        codes = s.data.to(torch.int64)
        counts = _device_counts(vocab, prog, -1)[codes]
        if vocab.validity is not None:
            vv = vocab.validity[codes]
            validity = vv if validity is None else (validity & vv)
    else:
        counts = _device_counts(s, prog, -1)
    return Series(s.name, DataType.int64(), data=counts, validity=validity)


def regexp_extract(s: Series, pattern: str, group: int = 0) -> Series:
    """The first match (`re.search(...).group(group)`); null where there is
    none."""
    prog = _span_program(s, pattern) if group == 0 else None
    if prog is None:
        return _host_regexp_extract(s, pattern, group)
    if s.is_dict():
        return _dict_map(s, lambda v: regexp_extract(v, pattern, group))
    counts, mo, starts, ends = _device_spans(s, prog, 1)
    hit = counts > 0
    # at most one match per row: match k belongs to the k-th row that hit
    seg_start = torch.zeros_like(counts)
    seg_len = torch.zeros_like(counts)
    seg_start[hit] = starts
    seg_len[hit] = ends - starts
    off, data = _copy_strings(s.data, seg_start, seg_len)
    return Series(s.name, DataType.string(), data=data, offsets=off,
                  validity=hit)


def regexp_extract_all(s: Series, pattern: str, group: int = 0) -> Series:
    """Every match of a row as list<string> (`re.finditer`)."""
    prog = _span_program(s, pattern) if group == 0 else None
    if prog is None:
        return _host_regexp_extract_all(s, pattern, group)
    s = s.dict_decode()
    counts, mo, starts, ends = _device_spans(s, prog, -1)
    off, data = _copy_strings(s.data, starts, ends - starts)
    child = Series("item", DataType.string(), data=data, offsets=off)
    return Series(s.name, _LIST_OF_STRING, offsets=mo, children=[child],
                  validity=s.validity)


def regexp_replace(s: Series, pattern: str, replacement: str) -> Series:
    """`re.sub(pattern, replacement, value)`.  A replacement with a backslash
    is a template to `re`, not a literal: host."""
    literal = isinstance(replacement, str) and "\\" not in replacement
    prog = _span_program(s, pattern) if literal else None
    if prog is None:
        return _host_regexp_replace(s, pattern, replacement)
    if s.is_dict():
        return _dict_map(s, lambda v: regexp_replace(v, pattern, replacement))
    n = len(s)
    counts, mo, starts, ends = _device_spans(s, prog, -1)
    m = starts.numel()
    row, rank, before, tail = _gaps(s, counts, mo, starts, ends)
    # row i is gap, replacement, gap, ..., gap: 2 * counts[i] + 1 segments,
    # the first of them at 2 * mo[i] + i; the replacement's bytes sit
    # behind the column's in the copy source
    rep = _bytes_tensor(replacement.encode(), s.device)
    src = torch.cat([s.data, rep])
    k = 2 * m + n
    seg_start = torch.zeros(k, dtype=torch.int64, device=s.device)
    seg_len = torch.zeros(k, dtype=torch.int64, device=s.device)
    gap = 2 * torch.arange(m, dtype=torch.int64, device=s.device) + row
    seg_start[gap] = before
    seg_len[gap] = starts - before
    seg_start[gap + 1] = s.data.numel()
    seg_len[gap + 1] = rep.numel()
    last = 2 * mo[1:] + torch.arange(n, dtype=torch.int64, device=s.device)
    tail_len = s.offsets[1:] - tail
    if s.validity is not None:
        tail_len = torch.where(s.validity, tail_len,
                               torch.zeros_like(tail_len))
    seg_start[last] = tail
    seg_len[last] = tail_len
    off, data = _copy_strings(src, seg_start, seg_len)
    first = torch.cat([last.new_zeros(1), last + 1])
    return Series(s.name, DataType.string(), data=data,
                  offsets=off[first].contiguous(), validity=s.validity)


def regexp_split(s: Series, pattern: str) -> Series:
    """`re.split(pattern, value)` as list<string>.  With a capturing group
    `re.split` puts the groups between the pieces: host."""
    prog = _span_program(s, pattern)
    if prog is None or prog.n_groups:
        return _host_regexp_split(s, pattern)
    s = s.dict_decode()
    n = len(s)
    counts, mo, starts, ends = _device_spans(s, prog, -1)
    row, rank, before, tail = _gaps(s, counts, mo, starts, ends)
    # a row is counts[i] + 1 pieces; a null row none
    pieces = counts + 1
    if s.validity is not None:
        pieces = torch.where(s.validity, pieces, torch.zeros_like(pieces))
    lo = torch.zeros(n + 1, dtype=torch.int64, device=s.device)
    torch.cumsum(pieces, 0, out=lo[1:])
    k = int(lo[-1].item())
    seg_start = torch.zeros(k, dtype=torch.int64, device=s.device)
    seg_len = torch.zeros(k, dtype=torch.int64, device=s.device)
    gap = lo[row] + rank
    seg_start[gap] = before
    seg_len[gap] = starts - before
    has = pieces > 0
    last = lo[1:][has] - 1
    seg_start[last] = tail[has]
    seg_len[last] = (s.offsets[1:] - tail)[has]
    off, data = _copy_strings(s.data, seg_start, seg_len)
    child = Series("item", DataType.string(), data=data, offsets=off)
    return Series(s.name, _LIST_OF_STRING, offsets=lo, children=[child],
                  validity=s.validity)


# --- length / manipulation ------------------------------------------------

def length(s: Series) -> Series:
    """Length in UTF-8 characters."""
    if s.is_dict():
        vlen = length(s.children[0]).data.view(torch.int64)
        out = vlen[s.data.to(torch.int64)]
        return Series(s.name, DataType.uint64(), data=out.view(torch.uint64),
                      validity=s.validity)
    if _is_gpu(s):
        out = native_required().str_char_length(s.offsets, s.data)
        return Series(s.name, DataType.uint64(),
                      data=out.view(torch.uint64), validity=s.validity)
    vals = _pylist_str(s)
    out = torch.tensor([0 if v is None else len(v) for v in vals],
                       dtype=torch.int64)
    return Series(s.name, DataType.uint64(), data=out.view(torch.uint64),
                  validity=s.validity)


def length_bytes(s: Series) -> Series:
    if s.is_dict():
        vlen = length_bytes(s.children[0]).data.view(torch.int64)
        out = vlen[s.data.to(torch.int64)]
        return Series(s.name, DataType.uint64(), data=out.view(torch.uint64),
                      validity=s.validity)
    lens = (s.offsets[1:] - s.offsets[:-1])
    return Series(s.name, DataType.uint64(), data=lens.view(torch.uint64),
                  validity=s.validity)


def substr(s: Series, start: int, length: Optional[int]) -> Series:
    """`length` characters from character `start` (0-based), to the end when
    `length` is None.  STRING columns count UTF-8 code points, BINARY
    columns bytes.  A start past the end, or `length == 0`, gives ""; a
    negative `start` or `length` raises ValueError."""
    if start < 0 or (length is not None and length < 0):
        raise ValueError(
            f"substr: start and length must be >= 0, got start={start}, "
            f"length={length}")
    d = _dict_map(s, lambda v: substr(v, start, length))
    if d is not None:
        return d
    if _is_gpu(s):
        new_off, new_bytes = native_required().str_substr(
            s.offsets, s.data, start, -1 if length is None else length,
            s.dtype.kind == TypeKind.STRING)
        return Series(s.name, s.dtype, data=new_bytes, offsets=new_off,
                      validity=s.validity)
    vals = _pylist_str(s)
    out = [None if v is None else
           (v[start:] if length is None else v[start:start + length])
           for v in vals]
    return Series.from_pylist(s.name, out, s.dtype) \
        .with_validity(s.validity)


def _map_python(s: Series, f) -> Series:
    s = s.dict_decode()
    vals = _pylist_str(s.cpu())
    out = [None if v is None else f(v) for v in vals]
    res = Series.from_pylist(s.name, out, DataType.string())
    return res.to(s.device) if s.is_gpu() else res


def _all_ascii(s: Series) -> bool:
    """One device reduction: the byte-parallel case kernel maps ASCII
    letters only, and Unicode case mapping can change a value's length, so
    a column with any byte >= 0x80 takes the host path."""
    return not bool((s.data >= 0x80).any().item())


def lower(s: Series) -> Series:
    d = _dict_map(s, lambda v: lower(v))
    if d is not None:
        return d
    if _is_gpu(s) and _all_ascii(s):
        out = native_required().str_case(s.offsets, s.data, 0)
        return Series(s.name, s.dtype, data=out, offsets=s.offsets,
                      validity=s.validity)
    return _map_python(s, str.lower)


def upper(s: Series) -> Series:
    d = _dict_map(s, lambda v: upper(v))
    if d is not None:
        return d
    if _is_gpu(s) and _all_ascii(s):
        out = native_required().str_case(s.offsets, s.data, 1)
        return Series(s.name, s.dtype, data=out, offsets=s.offsets,
                      validity=s.validity)
    return _map_python(s, str.upper)


def _device_strings(s: Series) -> bool:
    """A plain STRING column on the device: what the text kernels take."""
    return _is_gpu(s) and s.dtype.kind == TypeKind.STRING and \
        s.offsets is not None


def _strip(s: Series, mode: int, host) -> Series:
    """Trim `str.isspace` characters: mode 0 both sides, 1 left, 2 right."""
    d = _dict_map(s, lambda v: _strip(v, mode, host))
    if d is not None:
        return d
    if _device_strings(s):
        off, data = native_required().str_strip(s.offsets, s.data, mode)
        return Series(s.name, s.dtype, data=data, offsets=off,
                      validity=s.validity)
    return _map_python(s, host)


def lstrip(s: Series) -> Series:
    return _strip(s, 1, str.lstrip)


def rstrip(s: Series) -> Series:
    return _strip(s, 2, str.rstrip)


def strip(s: Series) -> Series:
    return _strip(s, 0, str.strip)


def reverse(s: Series) -> Series:
    """Reverse by code point (`v[::-1]`)."""
    d = _dict_map(s, lambda v: reverse(v))
    if d is not None:
        return d
    if _device_strings(s):
        off, data = native_required().str_reverse(s.offsets, s.data)
        return Series(s.name, s.dtype, data=data, offsets=off,
                      validity=s.validity)
    return _map_python(s, lambda v: v[::-1])


def capitalize(s: Series) -> Series:
    """`str.capitalize`.  An all-ASCII device column lower-cases with the
    byte-parallel kernel and upper-cases each row's first byte; a non-ASCII
    first character can title-case to another length (`ß` -> `Ss`): host."""
    d = _dict_map(s, lambda v: capitalize(v))
    if d is not None:
        return d
    if _device_strings(s) and _all_ascii(s):
        out = native_required().str_case(s.offsets, s.data, 0)
        first = s.offsets[:-1][s.offsets[1:] > s.offsets[:-1]]
        c = out[first]
        out[first] = torch.where((c >= 0x61) & (c <= 0x7A), c - 32, c)
        return Series(s.name, s.dtype, data=out, offsets=s.offsets,
                      validity=s.validity)
    return _map_python(s, str.capitalize)


# --- normalize --------------------------------------------------------------

def _normalize_value(v: str, remove_punct: bool, lowercase: bool,
                     nfd_unicode: bool, white_space: bool) -> str:
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


def _host_normalize(s: Series, remove_punct: bool, lowercase: bool,
                    nfd_unicode: bool, white_space: bool) -> Series:
    """Host path of normalize: one Python call per row."""
    return _host_rows(
        s, lambda v: _normalize_value(v, remove_punct, lowercase,
                                      nfd_unicode, white_space),
        DataType.string())


def normalize(s: Series, remove_punct: bool = False, lowercase: bool = True,
              nfd_unicode: bool = True, white_space: bool = True) -> Series:
    """Text normalization: strip combining marks after NFD, lower-case, drop
    what is neither `\\w` nor `\\s`, collapse whitespace runs, each if asked.

    On a device column the ASCII rows, for which NFD is the identity, run in
    one HIP kernel; it flags the rows that hold a byte >= 0x80, and only
    those go to the host and are merged back."""
    flags = (bool(remove_punct), bool(lowercase), bool(nfd_unicode),
             bool(white_space))
    d = _dict_map(s, lambda v: normalize(v, *flags))
    if d is not None:
        return d
    if not _device_strings(s):
        return _host_normalize(s, *flags)
    n = len(s)
    off, data, flagged = native_required().str_normalize_ascii(
        s.offsets, s.data, s.validity, flags[0], flags[1], flags[3])
    dev = Series(s.name, s.dtype, data=data, offsets=off, validity=s.validity)
    if not bool(flagged.any().item()):
        return dev
    rows = flagged.nonzero().reshape(-1)
    fixed = _host_normalize(s.take(rows), *flags)
    # spread the fixed rows over n rows: their bytes are already in order
    lens = torch.zeros(n, dtype=torch.int64, device=s.device)
    lens[rows] = fixed.offsets[1:] - fixed.offsets[:-1]
    spread_off = torch.zeros(n + 1, dtype=torch.int64, device=s.device)
    torch.cumsum(lens, 0, out=spread_off[1:])
    spread = Series(s.name, s.dtype, data=fixed.data, offsets=spread_off)
    from . import if_else
    cond = Series(s.name, DataType.bool(), data=flagged)
    return if_else(cond, spread, dev)


def concat_str(parts: List[Series]) -> Series:
    """Row-wise string concatenation."""
    parts = [p.dict_decode() for p in parts]
    # length-1 parts broadcast to the length of the others (which may be 0)
    lens = {len(p) for p in parts if len(p) != 1}
    assert len(lens) <= 1, f"concat_str: lengths differ: {sorted(lens)}"
    n = lens.pop() if lens else 1
    parts = [p.broadcast(n) if len(p) != n else p for p in parts]
    if _is_gpu(parts[0]):
        offs = [p.offsets for p in parts]
        datas = [p.data for p in parts]
        new_off, new_bytes = native_required().str_concat(offs, datas)
        validity = None
        for p in parts:
            if p.validity is not None:
                validity = p.validity if validity is None else (validity & p.validity)
        return Series(parts[0].name, DataType.string(), data=new_bytes,
                      offsets=new_off, validity=validity)
    cols = [p.to_pylist() for p in parts]
    out = []
    for vals in zip(*cols):
        if any(v is None for v in vals):
            out.append(None)
        else:
            out.append("".join(vals))
    return Series.from_pylist(parts[0].name, out, DataType.string())


def split(s: Series, sep: str) -> Series:
    """`str.split(sep)` as list<string>.  For a non-empty literal separator
    that is `re.split(re.escape(sep))`, which device columns run on the span
    kernels."""
    if _is_gpu(s) and isinstance(sep, str) and sep:
        return regexp_split(s, re.escape(sep))
    vals = _pylist_str(s.cpu())
    out = [None if v is None else v.split(sep) for v in vals]
    res = Series.from_pylist(s.name, out, DataType.list(DataType.string()))
    return res.to(s.device) if s.is_gpu() else res


def left(s: Series, n: int) -> Series:
    return substr(s, 0, n)


def _is_count(n) -> bool:
    return type(n) is int and n >= 0


def right(s: Series, n: int) -> Series:
    """The last `n` characters.  A negative `n` is a Python slice from the
    left (`v[-n:]`): host."""
    if _is_count(n):
        d = _dict_map(s, lambda v: right(v, n))
        if d is not None:
            return d
        if _device_strings(s):
            off, data = native_required().str_right(s.offsets, s.data, n)
            return Series(s.name, s.dtype, data=data, offsets=off,
                          validity=s.validity)
    return _map_python(s, lambda v: v[-n:] if n else "")


def find(s: Series, pat: str) -> Series:
    """Byte offset of the first match in the UTF-8 encoding, -1 if none
    (what the reference's `str::find` and the HIP kernel return; not the
    code-point index of Python's `str.find`)."""
    s = s.dict_decode()
    if _is_gpu(s):
        p = _bytes_tensor(pat.encode(), s.device)
        out = native_required().str_find(s.offsets, s.data, p, 0)
        return Series(s.name, DataType.int64(), data=out,
                      validity=s.validity)
    vals = _pylist_str(s)
    pb = pat.encode()
    out = torch.tensor([-1 if v is None else v.encode().find(pb)
                        for v in vals], dtype=torch.int64)
    return Series(s.name, DataType.int64(), data=out, validity=s.validity)


def _row_segments(s: Series, src, seg_start, seg_len, per_row: int) -> Series:
    """Rows made of `per_row` consecutive byte segments of `src` each."""
    off, data = _copy_strings(src, seg_start, seg_len)
    return Series(s.name, s.dtype, data=data,
                  offsets=off[::per_row].contiguous(), validity=s.validity)


def repeat(s: Series, n: int) -> Series:
    """`v * n`.  A device column copies each row as `n` segments."""
    if _is_count(n):
        d = _dict_map(s, lambda v: repeat(v, n))
        if d is not None:
            return d
        if _device_strings(s):
            k = max(n, 1)
            lens = (s.offsets[1:] - s.offsets[:-1]) if n else \
                torch.zeros(len(s), dtype=torch.int64, device=s.device)
            return _row_segments(s, s.data,
                                 s.offsets[:-1].repeat_interleave(k),
                                 lens.repeat_interleave(k), k)
    return _map_python(s, lambda v: v * n)


def _pad(s: Series, width: int, fillchar: str, left_side: bool) -> Series:
    """Device lpad / rpad: the first `width` characters of the row, and
    `width - length` copies of the fill before or after them.  The fill,
    repeated `width` times, sits behind the column's bytes in the copy
    source."""
    nat = native_required()
    n = len(s)
    head_off, _ = nat.str_substr(s.offsets, s.data, 0, width, True)
    head_len = head_off[1:] - head_off[:-1]
    chars = torch.clamp(nat.str_char_length(s.offsets, s.data), max=width)
    fill = fillchar.encode()
    src = torch.cat([s.data, _bytes_tensor(fill * width, s.device)])
    pad_start = torch.full((n,), s.data.numel(), dtype=torch.int64,
                           device=s.device)
    pad_len = (width - chars) * len(fill)
    parts = [(pad_start, pad_len), (s.offsets[:-1], head_len)]
    if not left_side:
        parts.reverse()
    return _row_segments(
        s, src, torch.stack([p[0] for p in parts], 1).reshape(-1),
        torch.stack([p[1] for p in parts], 1).reshape(-1), 2)


def _pad_args(width, fillchar) -> bool:
    # a negative width cuts characters off the end on the host
    # (`v.rjust(w)[:w]`), and a fill that is not one character raises there
    return _is_count(width) and isinstance(fillchar, str) and \
        len(fillchar) == 1


def lpad(s: Series, width: int, fillchar: str = " ") -> Series:
    if _pad_args(width, fillchar):
        d = _dict_map(s, lambda v: lpad(v, width, fillchar))
        if d is not None:
            return d
        if _device_strings(s):
            return _pad(s, width, fillchar, True)
    return _map_python(s, lambda v: v.rjust(width, fillchar)[:width])


def rpad(s: Series, width: int, fillchar: str = " ") -> Series:
    if _pad_args(width, fillchar):
        d = _dict_map(s, lambda v: rpad(v, width, fillchar))
        if d is not None:
            return d
        if _device_strings(s):
            return _pad(s, width, fillchar, False)
    return _map_python(s, lambda v: v.ljust(width, fillchar)[:width])

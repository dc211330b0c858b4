"""Parquet decode on the device: the bytes of the selected column chunks go
to HBM as the file holds them, and csrc/parquet.hip decompresses (Snappy) and
decodes their pages there.

The host does what is serial and small.  pyarrow's footer metadata says where
each column chunk lies and what it holds; a Thrift compact-protocol reader
(`_Thrift`) walks the chunk's page headers, which pyarrow does not expose.
`host_stage` turns a row group into an `RgPlan`: one pinned buffer with the
bytes of the device-decodable chunks, one page table (the int64 rows laid out
at the top of parquet.hip) and, per column, what to launch.  `decode` uploads
both once and runs, per row group, one Snappy launch over all pages and then
per column: the dictionary page (a typed gather table, or the vocabulary of a
string column), the definition levels, and the PLAIN and the RLE /
dictionary-index pages, each page by its own encoding.  A string or binary
column comes out as a dictionary Series (vocab, int32 codes).

Nulls.  A page stores only its non-null values.  The levels kernel writes
`validity` and, per page, the row of each stored value, so the value kernels
write every value straight to its row of a zeroed column; a V1 page does not
say how many nulls it has, and nothing on the host needs to know.  `validity`
is dropped when the chunk turns out to have no null.

Left on the host, column chunk by column chunk (`f.read_row_group` of those
columns, merged with the device columns in the requested order), and counted
in STATS["host_chunks"] with one of these reasons:

  codec      anything but UNCOMPRESSED and SNAPPY
  nested     a column with repetition, or more than one definition level
  type       INT96, decimals beyond precision 18, float16, time, duration,
             fixed-size binary, and whatever else is not int8..int64,
             uint8..uint64, float32/64, bool, date, timestamp, decimal <= 18
             (INT32, INT64 or FIXED_LEN_BYTE_ARRAY of <= 8 bytes), string,
             binary
  encoding   PLAIN BYTE_ARRAY data pages (also behind a dictionary that
             overflowed), DELTA_*, BYTE_STREAM_SPLIT, bit-packed levels
  corrupt    a page header that cannot be walked, or a page the kernels
             flagged: a Snappy element or RLE run past its page, a dictionary
             index out of range, a size that disagrees with the header

Syncs per row group: one, the transfer of every page's status and stored-value
count after the last launch, which decides on `corrupt` and on dropping
`validity`.  The uploads are from pinned memory and do not wait.
"""
from __future__ import annotations

import json
from typing import Iterator, List, Optional

import torch

from ..recordbatch import RecordBatch
from ..schema import DataType, TypeKind
from ..series import Series
from .. import arrow_interop

STATS = {"device_chunks": 0, "host_chunks": 0, "reasons": []}
REASONS = ("codec", "nested", "type", "encoding", "corrupt")

DESC = 12
ENC_PLAIN, ENC_DICT, ENC_RLE_BOOL = 0, 1, 2
_PAGE_DATA, _PAGE_DICT, _PAGE_DATA_V2 = 0, 2, 3
# parquet.thrift Encoding
_PLAIN, _PLAIN_DICTIONARY, _RLE, _RLE_DICTIONARY = 0, 2, 3, 8
_OTHER_ENCODINGS = {"DELTA_BINARY_PACKED", "DELTA_LENGTH_BYTE_ARRAY",
                    "DELTA_BYTE_ARRAY", "BYTE_STREAM_SPLIT", "BIT_PACKED"}
_INTS = {TypeKind.INT8: 1, TypeKind.INT16: 2, TypeKind.INT32: 4,
         TypeKind.INT64: 8, TypeKind.UINT8: 1, TypeKind.UINT16: 2,
         TypeKind.UINT32: 4, TypeKind.UINT64: 8}
_UNITS = {"milliseconds": "ms", "microseconds": "us", "nanoseconds": "ns"}


class _Fallback(Exception):
    def __init__(self, reason: str):
        super().__init__(reason)
        self.reason = reason


def _native():
    from . import native_required
    return native_required()


# ---------------------------------------------------------------------------
# Thrift compact protocol, as far as a PageHeader needs it
# ---------------------------------------------------------------------------

class _Thrift:
    """Reads structs as {field id: value}; nested structs as dicts, and
    every type it is not asked about is skipped."""

    def __init__(self, buf, pos: int, end: int):
        self.buf, self.pos, self.end = buf, pos, end

    def byte(self) -> int:
        if self.pos >= self.end:
            raise _Fallback("corrupt")
        b = self.buf[self.pos]
        self.pos += 1
        return b

    def varint(self) -> int:
        out = shift = 0
        while True:
            b = self.byte()
            out |= (b & 0x7F) << shift
            if not b & 0x80:
                return out
            shift += 7
            if shift > 63:
                raise _Fallback("corrupt")

    def zigzag(self) -> int:
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def skip_bytes(self, n: int):
        if n < 0 or self.pos + n > self.end:
            raise _Fallback("corrupt")
        self.pos += n

    def value(self, t: int, depth: int):
        if t in (1, 2):
            return t == 1
        if t == 3:
            return self.byte()
        if t in (4, 5, 6):
            return self.zigzag()
        if t == 7:
            return self.skip_bytes(8)
        if t == 8:
            return self.skip_bytes(self.varint())
        if t in (9, 10):
            head = self.byte()
            n = head >> 4
            if n == 15:
                n = self.varint()
            for _ in range(n):
                # a boolean element takes a byte of its own
                self.byte() if head & 15 in (1, 2) else \
                    self.value(head & 15, depth + 1)
            return None
        if t == 11:
            n = self.varint()
            kv = self.byte() if n else 0
            for _ in range(n):
                self.value(kv >> 4, depth + 1)
                self.value(kv & 15, depth + 1)
            return None
        if t == 12:
            return self.struct(depth + 1)
        raise _Fallback("corrupt")

    def struct(self, depth: int = 0) -> dict:
        if depth > 8:
            raise _Fallback("corrupt")
        out, fid = {}, 0
        while True:
            head = self.byte()
            if head == 0:
                return out
            fid = fid + (head >> 4) if head >> 4 else self.zigzag()
            out[fid] = self.value(head & 15, depth)


# ---------------------------------------------------------------------------
# what a column chunk needs
# ---------------------------------------------------------------------------

class _Col:
    """One device-decoded column of a row group: its rows of the page table
    and how its values are stored."""
    __slots__ = ("name", "dtype", "in_width", "big_endian", "out_width",
                 "optional", "dict_row", "dict_n", "dict_bytes", "rows",
                 "encs", "strings")


def _value_layout(pcol, atype):
    """(dtype, in_width, big_endian, out_width) of a flat column the kernels
    decode; raises _Fallback("type") otherwise."""
    import pyarrow as pa
    try:
        dt = arrow_interop.dtype_from_arrow(atype)
    except TypeError:
        raise _Fallback("type") from None
    k, phys = dt.kind, pcol.physical_type
    if k == TypeKind.BOOL and phys == "BOOLEAN":
        return dt, 0, False, 1
    if k in _INTS and phys in ("INT32", "INT64"):
        return dt, int(phys[3:]) // 8, False, _INTS[k]
    if k == TypeKind.FLOAT32 and phys == "FLOAT" and pa.types.is_float32(atype):
        return dt, 4, False, 4
    if k == TypeKind.FLOAT64 and phys == "DOUBLE":
        return dt, 8, False, 8
    if k == TypeKind.DATE and phys == "INT32" and pa.types.is_date32(atype):
        return dt, 4, False, 4
    if k == TypeKind.TIMESTAMP and phys == "INT64":
        lt = json.loads(pcol.logical_type.to_json() or "{}")
        if _UNITS.get(lt.get("timeUnit")) == atype.unit:
            return dt, 8, False, 8
    if k == TypeKind.DECIMAL128 and pa.types.is_decimal128(atype) and \
            atype.precision <= 18:
        if phys in ("INT32", "INT64"):
            return dt, int(phys[3:]) // 8, False, 8
        if phys == "FIXED_LEN_BYTE_ARRAY" and 1 <= pcol.length <= 8:
            return dt, pcol.length, True, 8
    if k in (TypeKind.STRING, TypeKind.BINARY) and phys == "BYTE_ARRAY" and \
            not pa.types.is_decimal(atype):
        return dt, 0, False, 4
    raise _Fallback("type")


def _walk_pages(raw, base: int, size: int, num_values: int):
    """Page headers of the chunk raw[base, base + size): a list of (header
    dict, payload position)."""
    pages, pos, seen = [], base, 0
    while seen < num_values and pos < base + size:
        rd = _Thrift(raw, pos, base + size)
        h = rd.struct()
        comp = h.get(3)
        if not isinstance(comp, int) or not isinstance(h.get(2), int) or \
                comp < 0 or h[2] < 0 or rd.pos + comp > base + size:
            raise _Fallback("corrupt")
        if h.get(1) in (_PAGE_DATA, _PAGE_DATA_V2):
            sub = h.get(5 if h[1] == _PAGE_DATA else 8)
            if not isinstance(sub, dict) or not isinstance(sub.get(1), int) \
                    or sub[1] < 0:
                raise _Fallback("corrupt")
            seen += sub[1]
        pages.append((h, rd.pos))
        pos = rd.pos + comp
    if seen != num_values:
        raise _Fallback("corrupt")
    return pages


def _plan_chunk(col: _Col, cmeta, raw, base: int, src0: int, arena: List[int],
                table: List[List[int]]) -> None:
    """Appends the chunk's rows to `table`.  raw[base:] holds the chunk and
    will lie at src0 of the device buffer; arena[0] is the next free byte of
    the decompression arena behind the uploaded bytes."""
    snappy = cmeta.compression == "SNAPPY"
    first_row = 0
    col.dict_row, col.dict_n, col.dict_bytes = None, 0, 0
    col.rows, col.encs = [], set()
    for h, pos in _walk_pages(raw, base, cmeta.total_compressed_size,
                              cmeta.num_values):
        kind, uncomp, comp = h.get(1), h[2], h[3]
        src = src0 + pos - base
        row = [0] * DESC
        if kind == _PAGE_DICT:
            sub = h.get(7)
            if not isinstance(sub, dict) or col.dict_row is not None or \
                    col.rows or not isinstance(sub.get(1), int) or sub[1] < 0:
                raise _Fallback("corrupt")
            if sub.get(2) not in (_PLAIN, _PLAIN_DICTIONARY):
                raise _Fallback("encoding")
            levels, nvals, enc, lvl_len = False, sub[1], ENC_PLAIN, 0
            col.dict_row, col.dict_n = len(table), nvals
            col.dict_bytes = uncomp - 4 * nvals
            compressed = snappy
        elif kind == _PAGE_DATA:
            sub = h[5]
            levels, nvals, lvl_len = col.optional, sub[1], -1
            if levels and sub.get(3) != _RLE:
                raise _Fallback("encoding")
            enc, compressed = sub.get(2), snappy
        elif kind == _PAGE_DATA_V2:
            sub = h[8]
            levels, nvals, lvl_len = col.optional, sub[1], sub.get(5, 0)
            if sub.get(6, 0) != 0 or lvl_len < 0 or lvl_len > comp or \
                    (not levels and lvl_len):
                raise _Fallback("corrupt")
            enc = sub.get(4)
            compressed = snappy and sub.get(7, True) and comp > lvl_len
        else:
            continue                      # an index page: nothing to decode
        if kind != _PAGE_DICT:
            if enc in (_PLAIN_DICTIONARY, _RLE_DICTIONARY):
                if col.dict_row is None:
                    raise _Fallback("corrupt")
                enc = ENC_DICT
            elif enc == _PLAIN and not col.strings:
                enc = ENC_PLAIN
            elif enc == _RLE and col.in_width == 0 and not col.strings:
                enc = ENC_RLE_BOOL
            else:
                raise _Fallback("encoding")
            col.rows.append(len(table))
            col.encs.add(enc)
        v2 = kind == _PAGE_DATA_V2
        head = lvl_len if v2 else 0       # bytes that are never compressed
        if compressed:
            dst = arena[0]
            arena[0] += (uncomp - head + 15) & ~15
            if uncomp < head:
                raise _Fallback("corrupt")
            row[0:4] = [src + head, comp - head, dst, uncomp - head]
            val_off, val_end = dst, dst + uncomp - head
        else:
            if comp != uncomp:
                raise _Fallback("corrupt")
            val_off, val_end = src + head, src + comp
        row[4] = src if v2 else val_off
        row[5] = lvl_len if v2 else -1 if levels else 0
        row[6], row[7] = val_off, val_end
        row[8], row[9], row[10] = nvals, 0 if kind == _PAGE_DICT else \
            first_row, enc
        if kind != _PAGE_DICT:
            first_row += nvals
        table.append(row)
    if col.strings and col.dict_row is None and col.rows:
        raise _Fallback("encoding")
    if col.strings and col.dict_bytes < 0:
        raise _Fallback("corrupt")


class RgPlan:
    """A row group after the host stage."""
    __slots__ = ("rg", "num_rows", "names", "cols", "host", "reasons",
                 "stage", "src_bytes", "buf_bytes", "table", "whole_host")


def host_stage(path: str, columns: Optional[List[str]], predicate=None,
               row_groups=None) -> Iterator[RgPlan]:
    """One RgPlan per row group that survives pruning: metadata, page-header
    walk, and the chunks' bytes read into pinned memory.  Nothing here
    touches the device."""
    import numpy as np
    import pyarrow.parquet as pq
    from ..io import readers
    f = pq.ParquetFile(path)
    md, aschema = f.metadata, f.schema_arrow
    names = list(aschema.names) if columns is None else list(columns)
    leaves = {}
    for i in range(md.num_columns):
        leaves.setdefault(f.schema.column(i).path.split(".")[0], []).append(i)
    bounds = readers._predicate_bounds(predicate)
    name_to_idx = {c: i for i, c in enumerate(aschema.names)} if bounds \
        else {}
    with open(path, "rb") as fh:
        for rg in (row_groups if row_groups is not None
                   else range(md.num_row_groups)):
            rmeta = md.row_group(rg)
            if bounds and not readers._rg_may_match(rmeta, name_to_idx,
                                                    bounds):
                continue
            plan = RgPlan()
            plan.rg, plan.num_rows, plan.names = rg, rmeta.num_rows, names
            plan.cols, plan.host, plan.reasons, plan.table = [], [], [], []
            plan.stage, plan.src_bytes, plan.buf_bytes = None, 0, 0
            plan.whole_host = rmeta.num_rows == 0 or \
                len(set(names)) != len(names) or \
                any(n not in leaves for n in names)
            if plan.whole_host:
                yield plan
                continue
            picked = []
            for name in names:
                try:
                    idx = leaves[name]
                    pcol = f.schema.column(idx[0])
                    if len(idx) != 1 or pcol.path != name or \
                            pcol.max_repetition_level or \
                            pcol.max_definition_level > 1:
                        raise _Fallback("nested")
                    cmeta = rmeta.column(idx[0])
                    if cmeta.compression not in ("UNCOMPRESSED", "SNAPPY"):
                        raise _Fallback("codec")
                    col = _Col()
                    col.name = name
                    col.dtype, col.in_width, col.big_endian, col.out_width = \
                        _value_layout(pcol, aschema.field(name).type)
                    col.strings = col.dtype.kind in (TypeKind.STRING,
                                                     TypeKind.BINARY)
                    col.optional = pcol.max_definition_level == 1
                    if _OTHER_ENCODINGS & set(cmeta.encodings):
                        raise _Fallback("encoding")
                    if cmeta.num_values != rmeta.num_rows:
                        raise _Fallback("corrupt")
                    start = cmeta.data_page_offset
                    if cmeta.has_dictionary_page and \
                            cmeta.dictionary_page_offset:
                        start = min(start, cmeta.dictionary_page_offset)
                    picked.append((col, cmeta, start))
                except _Fallback as e:
                    plan.host.append(name)
                    plan.reasons.append(e.reason)
            # every picked chunk 16-byte aligned in one pinned buffer
            total, at = 0, []
            for _, cmeta, _ in picked:
                at.append(total)
                total += (cmeta.total_compressed_size + 15) & ~15
            if not picked:
                yield plan
                continue
            stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            raw = memoryview(stage.numpy())
            arena = [total]
            for (col, cmeta, start), src0 in zip(picked, at):
                fh.seek(start)
                size = cmeta.total_compressed_size
                mark = len(plan.table)
                try:
                    if fh.readinto(raw[src0:src0 + size]) != size:
                        raise _Fallback("corrupt")
                    _plan_chunk(col, cmeta, raw, src0, src0, arena,
                                plan.table)
                    plan.cols.append(col)
                except _Fallback as e:
                    del plan.table[mark:]
                    plan.host.append(col.name)
                    plan.reasons.append(e.reason)
            plan.stage, plan.src_bytes, plan.buf_bytes = stage, total, \
                arena[0]
            yield plan


# ---------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------

def _host_columns(f, plan: RgPlan, names: List[str], device) -> dict:
    tbl = f.read_row_group(plan.rg, columns=names)
    rb = RecordBatch.from_arrow(tbl, device=device)
    return {c.name: c for c in rb.columns}


def decode(path: str, plan: RgPlan, device) -> RecordBatch:
    """The row group of `plan` as a batch on `device`."""
    import pyarrow.parquet as pq
    if plan.whole_host:
        tbl = pq.ParquetFile(path).read_row_group(plan.rg,
                                                  columns=plan.names)
        return RecordBatch.from_arrow(tbl, device=device)
    nat = _native()
    n = plan.num_rows
    done, host, reasons = {}, list(plan.host), list(plan.reasons)
    if plan.cols:
        with torch.cuda.device(device):
            buf = torch.empty(max(plan.buf_bytes, 16), dtype=torch.uint8,
                              device=device)
            buf[:plan.src_bytes].copy_(plan.stage[:plan.src_bytes],
                                       non_blocking=True)
            table = torch.tensor(plan.table, dtype=torch.int64).reshape(
                -1, DESC).pin_memory().to(device, non_blocking=True)
            npages = table.shape[0]
            status = torch.zeros(npages, dtype=torch.int32, device=device)
            stored_all = torch.zeros(npages, dtype=torch.int32, device=device)
            nat.pq_snappy(buf, table, status)
            built = []
            for col in plan.cols:
                built.append(_decode_column(nat, col, buf, table, status,
                                            stored_all, n, device))
            flags = torch.stack([status, stored_all]).tolist()   # the sync
        for col, s in zip(plan.cols, built):
            rows = col.rows + ([col.dict_row] if col.dict_row is not None
                               else [])
            if any(flags[0][r] for r in rows):
                host.append(col.name)
                reasons.append("corrupt")
                continue
            if col.optional and sum(flags[1][r] for r in col.rows) == n:
                s = Series(s.name, s.dtype, data=s.data, children=s.children,
                           length=n)
            done[col.name] = s
            STATS["device_chunks"] += 1
    if host:
        STATS["host_chunks"] += len(host)
        STATS["reasons"].extend(reasons)
        done.update(_host_columns(pq.ParquetFile(path), plan, host, device))
    return RecordBatch([done[name] for name in plan.names], num_rows=n)


def _decode_column(nat, col: _Col, buf, table, status, stored_all, n: int,
                   device) -> Series:
    lo, hi = col.rows[0], col.rows[-1] + 1
    pages, st = table[lo:hi], status[lo:hi]
    validity = row_map = stored = None
    if col.optional:
        validity, row_map, stored = nat.pq_levels(buf, pages, n, st)
        stored_all[lo:hi] = stored
    w = col.out_width
    # zeroed: the slot under a null stays 0
    out = torch.zeros(n * w, dtype=torch.uint8, device=device)
    dict_t, dict_n, vocab = None, 2, None
    if col.dict_row is not None:
        drow = table[col.dict_row:col.dict_row + 1]
        dst = status[col.dict_row:col.dict_row + 1]
        dict_n = col.dict_n
        if col.strings:
            offsets, data = nat.pq_dict_strings(buf, drow, dict_n,
                                                col.dict_bytes, dst)
            vocab = Series("vocab", col.dtype, data=data, offsets=offsets)
        else:
            dict_t = torch.zeros(dict_n * w, dtype=torch.uint8, device=device)
            nat.pq_plain(buf, drow, None, None, dict_t, col.in_width,
                         col.big_endian, w, dst)
    elif col.strings:
        # a chunk without pages: an empty vocabulary
        vocab = Series("vocab", col.dtype,
                       data=torch.zeros(0, dtype=torch.uint8, device=device),
                       offsets=torch.zeros(1, dtype=torch.int64,
                                           device=device))
        dict_n = 0
    if ENC_PLAIN in col.encs:
        nat.pq_plain(buf, pages, row_map, stored, out, col.in_width,
                     col.big_endian, w, st)
    if col.encs - {ENC_PLAIN}:
        nat.pq_rle_values(buf, pages, row_map, stored, dict_t, dict_n, out, w,
                          st)
    if col.strings:
        return Series.make_dict(col.name, vocab, out.view(torch.int32),
                                validity)
    return Series(col.name, col.dtype, data=out.view(col.dtype.to_torch()),
                  validity=validity)


# ---------------------------------------------------------------------------
# a file
# ---------------------------------------------------------------------------

def eligible(path, read_options: Optional[dict], device) -> bool:
    """The device path reads local files on a GPU, unless
    `device_decode=False`."""
    ro = read_options or {}
    if ro.get("device_decode") is False or \
            not str(device).startswith("cuda") or not isinstance(path, str):
        return False
    from ..io.object_store import is_remote
    return not is_remote(path)


def read_file_device(path: str, columns: Optional[List[str]],
                     limit: Optional[int], device, predicate=None,
                     row_groups=None,
                     staged: Optional[List[RgPlan]] = None
                     ) -> Iterator[RecordBatch]:
    """One batch per row group of a local parquet file, decoded on `device`;
    `staged` are the plans where a prefetching thread has made them."""
    remaining = limit
    plans = staged if staged is not None else \
        host_stage(path, columns, predicate, row_groups)
    for plan in plans:
        if remaining is not None and remaining <= 0:
            return
        rb = decode(path, plan, device)
        if remaining is not None:
            if len(rb) > remaining:
                rb = rb.slice(0, remaining)
            remaining -= len(rb)
        yield rb

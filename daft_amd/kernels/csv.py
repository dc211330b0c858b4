"""CSV decode on the device: raw file bytes go to HBM, csrc/csv.hip finds the
separators that are outside quotes and cuts out the selected columns, and the
parse kernels of csrc/strparse.hip turn them into values.

`decode_chunk` decodes one chunk that begins at a record start and raises
`CsvFallback(reason)` for what the kernels do not decide: an irregular quote
(`x"y`, `"x"y`), a ragged row, a blank line, invalid UTF-8, a quote still open
at the end of the file, no complete record in the chunk, or a `\r` outside
quotes that no `\n` follows (`bare_cr`: pyarrow ends a record there).
`read_file_device` cuts a file into chunks, carries each chunk's unconsumed
tail into the next, and sends a refused chunk through the pyarrow reader with
the scan schema's types, so those inputs give what the host path gives.
`STATS` counts both kinds of chunk.

A value that pyarrow refuses for the schema's type (`+5` as int64) has no
reason of its own: `device_decode=False` does not apply the schema's types
but infers them, so that chunk is read by pyarrow the same way, by inference,
and counted as a host chunk.

Syncs per chunk: two for the structure (the separator count; then flags and
column sizes in one transfer), one more per kernel-typed column (the status
maximum in `parse._merge`), and the small pageable upload of the selected
column indices.  A chunk that is grown by the next block is uploaded again.

Typed columns.  STRING columns are the extracted bytes and are never null.
Integers, float64, decimals of precision <= 18 and dates run the parse
kernels: status 1 (the empty field) is null, and the status-2 rows are
written out as a one-column, fully quoted CSV and read by pyarrow with the
column's type, so null spellings, whitespace and errors are pyarrow's by
construction.  Every other type goes through that host function whole.

Where pyarrow 25 disagrees with a status-0 answer of the kernels, a device
pre-check (csv_precheck) turns the row into status 2.  The grammar of
csrc/api.h, class by class:

  integers   `+5`, `+0`: an error in pyarrow, parsed by str_parse_int ->
             pre-check on a leading '+'.  `-0` in an unsigned column: an
             error in pyarrow, 0 in the kernel -> pre-check on a leading '-'.
             `007`, `-007`, `-0` (signed), the type's limits: both agree.
  decimals   pyarrow refuses a text whose digit count exceeds the precision,
             zeros included (`1.50000000000` for decimal(12, 2)), while the
             kernel accepts any zeros past the scale -> pre-check on more
             fractional digits than the scale, which also sends `1.500` to
             pyarrow (it answers 1.50).  `+1.5`, `.5`, `1.`, `007.5`, `-0`:
             both agree.  `1e2` is status 2 already.
  float64    `1.`, `.5`, `+.5`, `007`, `1e+5`, `1.e5`, `-0`, exponents with
             leading zeros: both agree.  `1e400`, `1e-400`, `4.9e-324`,
             `inf`, `nan` (null in pyarrow) and integers of 20 digits are
             status 2 already.  No pre-check.
  dates      only `YYYY-MM-DD` in years 0001-9999 is status 0, and pyarrow
             agrees on it.  No pre-check.
"""
from __future__ import annotations

import csv as _pycsv
import io
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from ..recordbatch import RecordBatch
from ..schema import DataType, TypeKind
from ..series import Series
from . import parse

STATS = {"device_chunks": 0, "host_chunks": 0, "reasons": []}
BLOCK_BYTES = 256 << 20          # file bytes per chunk; tests lower it
MAX_CHUNK = (1 << 31) - 64       # positions are int32

_ERR_IRREGULAR, _ERR_UTF8, _ERR_RAGGED, _ERR_BLANK, _ERR_BARE_CR = \
    1, 2, 4, 8, 16
_COMPRESSED = (".gz", ".zst", ".zstd", ".bz2", ".lz4")
_UNSIGNED = (TypeKind.UINT8, TypeKind.UINT16, TypeKind.UINT32,
             TypeKind.UINT64)


class CsvFallback(Exception):
    """The chunk is left to the host reader.  `consumed` is where its last
    complete record ends, when the kernels could tell.  `reason` is None
    where pyarrow refused a value for its column's type."""

    def __init__(self, reason: Optional[str],
                 consumed: Optional[int] = None):
        super().__init__(reason)
        self.reason = reason
        self.consumed = consumed


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------

def _host_convert(s: Series, dtype: DataType) -> Series:
    """The texts of `s` as `dtype`, converted by pyarrow's CSV reader."""
    import pyarrow as pa
    import pyarrow.csv as pacsv
    from .. import arrow_interop
    texts = s.cpu().to_pylist()
    if not texts:
        return Series.from_pylist(s.name, [], dtype, device=s.device)
    buf = "".join('"' + t.replace('"', '""') + '"\n' for t in texts)
    tbl = pacsv.read_csv(
        io.BytesIO(buf.encode("utf-8")),
        read_options=pacsv.ReadOptions(column_names=[s.name]),
        parse_options=pacsv.ParseOptions(newlines_in_values=True),
        convert_options=pacsv.ConvertOptions(
            column_types={s.name: arrow_interop.dtype_to_arrow(dtype)}))
    assert tbl.num_rows == len(texts)
    col, valid = tbl.column(0).combine_chunks(), None
    if col.null_count and (pa.types.is_integer(col.type) or
                           pa.types.is_floating(col.type)):
        # numpy would hold the nulls as NaN in a float64 array, which keeps
        # neither 64-bit integers nor infinities: fill them instead
        valid = torch.from_numpy(col.is_valid().to_numpy(zero_copy_only=False))
        col = col.fill_null(0)
    out = Series.from_arrow(s.name, col)
    if valid is not None:
        out = Series(out.name, out.dtype, data=out.data, validity=valid)
    return out.to(s.device)


def _kernel_type(dtype: DataType) -> bool:
    k = dtype.kind
    if k == TypeKind.DECIMAL128:
        return dtype.precision <= 18
    return k in parse._INT_RANGE or k in (TypeKind.FLOAT64, TypeKind.DATE)


def _typed(s: Series, dtype: DataType) -> Series:
    """The extracted STRING column `s` as the scan schema's `dtype`."""
    if dtype.kind == TypeKind.STRING:
        return s
    if len(s) == 0 or not _kernel_type(dtype):
        return _host_convert(s, dtype)
    values, status = parse._run_kernel(s, dtype)
    k = dtype.kind
    if k in parse._INT_RANGE:
        parse._native().csv_precheck(s.offsets, s.data, status,
                                     1 if k in _UNSIGNED else 0, 0)
    elif k == TypeKind.DECIMAL128:
        parse._native().csv_precheck(s.offsets, s.data, status, 2,
                                     dtype.scale)
    return parse._merge(s, dtype, values, status,
                        lambda t: _host_convert(t, dtype))


# ---------------------------------------------------------------------------
# one chunk
# ---------------------------------------------------------------------------

def decode_chunk(bytes_dev: torch.Tensor, ncols_expected: int,
                 names: List[str], schema: Dict[str, DataType],
                 columns: Optional[List[str]], delim: str,
                 skip_first_record: bool,
                 final: bool) -> Tuple[RecordBatch, int]:
    """(batch of the selected columns, bytes consumed) of a chunk that begins
    at a record start.  A final chunk ends in a newline."""
    import pyarrow as pa
    nat = parse._native()
    ncols = ncols_expected
    columns = list(names) if columns is None else list(columns)
    sel = [names.index(c) for c in columns]
    sepmask, tile_base, info = nat.csv_structure(bytes_dev, ord(delim))
    err, cont, _, nsep, end_parity = info.tolist()[:5]
    if (err & _ERR_UTF8) or cont != 0:
        raise CsvFallback("invalid_utf8")
    if err & _ERR_IRREGULAR:
        raise CsvFallback("irregular_quote")
    if err & _ERR_BARE_CR:
        raise CsvFallback("bare_cr")
    if final and end_parity:
        raise CsvFallback("open_quote_at_end")
    sep_pos = nat.csv_emit(bytes_dev, sepmask, tile_base, info, nsep, ncols)
    row0 = 1 if skip_first_record else 0
    nrows = max(nsep // ncols - row0, 0)
    seg_start, lens, any_quoted = nat.csv_field_lens(
        bytes_dev, sep_pos, ncols, row0, nrows, sel)
    offs = torch.zeros((len(sel), nrows + 1), dtype=torch.int64,
                       device=bytes_dev.device)
    torch.cumsum(lens, 1, out=offs[:, 1:])
    host = torch.cat([info.to(torch.int64), offs[:, -1],
                      any_quoted.to(torch.int64)]).tolist()
    err, consumed = host[0], host[2]
    if err & _ERR_BLANK:
        raise CsvFallback("blank_line", consumed)
    if err & _ERR_RAGGED:
        raise CsvFallback("ragged", consumed)
    if consumed == 0:
        raise CsvFallback("no_record_end")
    totals, quoted = host[8:8 + len(sel)], host[8 + len(sel):]
    cols = []
    for j, name in enumerate(columns):
        data = nat.csv_extract(bytes_dev, sep_pos, ncols, row0, sel[j],
                               seg_start[j], offs[j], totals[j],
                               bool(quoted[j]))
        s = Series(name, DataType.string(), data=data, offsets=offs[j])
        try:
            cols.append(_typed(s, schema[name]))
        except pa.ArrowInvalid:
            raise CsvFallback(None, consumed) from None
    return RecordBatch(cols, num_rows=nrows), consumed


# ---------------------------------------------------------------------------
# a file
# ---------------------------------------------------------------------------

def eligible(path, read_options: Optional[dict], device) -> bool:
    """The device path reads local, uncompressed files on a GPU, unless
    `device_decode=False`."""
    ro = read_options or {}
    if ro.get("device_decode") is False or "schema" not in ro or \
            not str(device).startswith("cuda") or not isinstance(path, str):
        return False
    from ..io.object_store import is_remote
    return not is_remote(path) and not path.endswith(_COMPRESSED)


_pinned: dict = {}


def _upload(buf: bytes, device) -> torch.Tensor:
    """`buf` in device memory, staged through a reused pinned buffer (every
    decode_chunk ends in a sync, so the buffer is free again)."""
    import numpy as np
    n = len(buf)
    stage = _pinned.get("buf")
    if stage is None or stage.numel() < n:
        stage = torch.empty(max(n, 1 << 16), dtype=torch.uint8,
                            pin_memory=True)
        _pinned["buf"] = stage
    stage.numpy()[:n] = np.frombuffer(buf, dtype=np.uint8)
    out = torch.empty(n, dtype=torch.uint8, device=device)
    out.copy_(stage[:n], non_blocking=True)
    return out


def _first_record(f, delim: str) -> Optional[List[str]]:
    """Fields of the file's first record, read by the csv module from a
    growing prefix; None for an empty file.  Leaves `f` at the start."""
    size = 1 << 20
    while True:
        f.seek(0)
        head = f.read(size)
        rows = _pycsv.reader(
            io.StringIO(head.decode("utf-8", "replace"), newline=""),
            delimiter=delim)
        row = next(rows, None)
        # a second record shows that the first one is complete
        if len(head) < size or next(rows, None) is not None:
            f.seek(0)
            return row
        size *= 4


def _host_records(raw: bytes, header: bytes, names, schema, columns,
                  read_options, device, typed: bool) -> Iterator[RecordBatch]:
    """Records `raw` through the pyarrow reader: with the scan schema's
    types, or, where those refused a value, inferring them as
    `device_decode=False` does."""
    import pyarrow as pa
    from .. import arrow_interop
    from ..io import readers
    types = {n: arrow_interop.dtype_to_arrow(schema[n]) for n in names
             if n in schema} if typed else None
    yield from readers._read_csv(pa.BufferReader(header + raw), columns,
                                 read_options, device, column_types=types)


def read_file_device(path: str, columns: Optional[List[str]],
                     read_options: dict, device,
                     raw: Optional[bytes] = None) -> Iterator[RecordBatch]:
    """Batches of a local CSV file decoded on `device`; `raw` is the file's
    content where a prefetching thread has read it already."""
    from ..io import readers
    ro = read_options
    delim = ro.get("delimiter", ",")
    has_headers = ro.get("has_headers", True)
    schema = ro["schema"]
    with (io.BytesIO(raw) if raw is not None else open(path, "rb")) as f:
        first = _first_record(f, delim)
        names = first if has_headers else \
            [f"f{i}" for i in range(len(first or []))]
        want = names if columns is None else columns
        if not names or len(set(names)) != len(names) or \
                any(c not in names or c not in schema for c in want):
            # nothing to decode by: the host reader answers, or raises
            yield from readers._read_csv(
                path if raw is None else io.BytesIO(raw), columns, ro,
                device)
            return
        header = b""
        if has_headers:
            header = delim.join('"' + n.replace('"', '""') + '"'
                                for n in names).encode("utf-8") + b"\n"
        block_bytes = BLOCK_BYTES
        tail, at_start, eof = b"", True, False
        while not eof:
            block = f.read(block_bytes)
            eof = len(block) < block_bytes
            buf = tail + block
            if eof and buf and not buf.endswith(b"\n"):
                buf += b"\n"
            if not buf:
                break
            skip = at_start and has_headers
            try:
                if len(buf) > MAX_CHUNK:
                    raise CsvFallback("no_record_end")
                with torch.cuda.device(device):
                    rb, consumed = decode_chunk(
                        _upload(buf, device), len(names), names, schema,
                        columns, delim, skip, eof)
            except CsvFallback as e:
                if e.reason == "no_record_end" and not eof and \
                        len(buf) <= MAX_CHUNK:
                    tail = buf          # grow the chunk by the next block
                    continue
                STATS["host_chunks"] += 1
                typed = e.reason is not None
                if typed:
                    STATS["reasons"].append(e.reason)
                # the first chunk still holds the file's own header record
                head = b"" if skip else header
                if e.consumed:
                    yield from _host_records(buf[:e.consumed], head, names,
                                             schema, columns, ro, device,
                                             typed)
                    tail, at_start = buf[e.consumed:], False
                    continue
                yield from _host_records(buf + f.read(), head, names, schema,
                                         columns, ro, device, typed)
                return
            STATS["device_chunks"] += 1
            tail, at_start = buf[consumed:], False
            if len(rb):
                yield rb

"""JSON-lines decode on the device: raw file bytes go to HBM, csrc/json.hip
finds the strings (escape-aware), the nesting depth and the fields of every
record by key, cuts out the values of the scan schema's columns, and the parse
kernels of csrc/strparse.hip turn number and timestamp texts into values.

`decode_chunk` decodes one chunk that begins at a record start and raises
`JsonFallback(reason)` for what the kernels do not decide.  Structure:
`invalid_utf8`, `long_escape_run` (64 or more backslashes in a row),
`control_char` (a raw byte below 0x20 in a string), `irregular` (any byte or
token order outside the grammar, `+1`, `01`, a trailing comma), `depth`,
`open_string_at_end`, `no_record_end`.  Keys: `escaped_key`, `unknown_key`,
`duplicate_key`; under the schema pyarrow raises or widens there, and the
host path decides which.  Values: `bad_escape` (also a lone surrogate),
`type_mismatch` (a value of another kind than its column's type),
`long_record` (pyarrow refuses a record of 1 MiB or more), and None where
pyarrow refused a value's text for its column's type.
`names` sends a whole file to the host: more than 256 schema names, or more
than 2048 bytes of them, do not fit the LDS table of json_fields.
`read_file_device` cuts a file into chunks, carries each chunk's unconsumed
tail into the next, and sends a refused chunk through `pyarrow.json` with the
scan schema as `explicit_schema`, so those inputs give what the host gives,
or its error.  `STATS` counts both kinds of chunk.

Syncs per chunk: three for the structure (token count and `consumed`; row
count and key flags; value flags, kinds seen and column sizes in one
transfer), one more per int64, float64 or timestamp column (the status
maximum in `parse._merge`).

Typed columns.  Strings are the unescaped bytes, bools come from the values
kernel, both with its null mask.  int64 and float64 texts run str_parse_int /
str_parse_float, timestamp[s] strings run str_parse_datetime with separator
`T`; status-2 rows (exponent forms in an int64 column, `1e400`, the space
separator, a `Z` suffix, date-only) are read back through `pyarrow.json` with
a one-field explicit schema, so they are pyarrow's answer by construction.
Every other type, struct, list and null included, goes through that host
function whole, selected or not, which also checks the nested text.

Every value of every schema column is classified and its grammar checked,
whether selected or not, as pyarrow parses all of a record.  What is not
checked for a column that is not selected is its numbers' range: pyarrow
refuses `99999999999999999999` under an int64 schema even there.
"""
from __future__ import annotations

import io
import json as _pyjson
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from ..recordbatch import RecordBatch
from ..schema import DataType, TypeKind
from ..series import Series
from . import parse
from .csv import MAX_CHUNK, _COMPRESSED, _upload

STATS = {"device_chunks": 0, "host_chunks": 0, "reasons": []}
BLOCK_BYTES = 256 << 20          # file bytes per chunk; tests lower it
MAX_KEYS, MAX_KEY_BYTES = 256, 2048   # what json_fields stages in LDS
MAX_RECORD = 1 << 20             # pyarrow's block: a record must fit in it

# info[0] bits of csrc/json.hip, in the order they are reported
_STRUCTURE = ((2, "invalid_utf8"), (4, "long_escape_run"),
              (256, "control_char"), (1, "irregular"), (8, "depth"))
_KEYS = ((1, "irregular"), (16, "escaped_key"), (32, "unknown_key"),
         (64, "duplicate_key"))
_VALUES = ((128, "bad_escape"), (1, "irregular"))
_NULL, _FALSE, _TRUE, _NUMBER, _STRING, _NESTED = 1, 2, 4, 8, 16, 32
_ESCAPES = 256


class JsonFallback(Exception):
    """The chunk is left to the host reader.  `consumed` is where its last
    complete line ends, when the kernels could tell.  `reason` is None where
    pyarrow refused a value for its column's type."""

    def __init__(self, reason: Optional[str],
                 consumed: Optional[int] = None):
        super().__init__(reason)
        self.reason = reason
        self.consumed = consumed


def _refuse(err: int, table, consumed: Optional[int] = None) -> None:
    for bit, reason in table:
        if err & bit:
            raise JsonFallback(reason, consumed)


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------

def _allowed(dtype: DataType) -> Optional[int]:
    """Kinds of value the kernels turn into `dtype`; None: the host function
    converts the whole column."""
    k = dtype.kind
    if k == TypeKind.STRING:
        return _NULL | _STRING
    if k == TypeKind.BOOL:
        return _NULL | _FALSE | _TRUE
    if k in (TypeKind.INT64, TypeKind.FLOAT64):
        return _NULL | _NUMBER
    if k == TypeKind.TIMESTAMP and dtype.timeunit == "s" and \
            not dtype.timezone:
        return _NULL | _STRING
    return None


def _arrow_type(dtype: DataType):
    """`dtype` as pyarrow.json builds it: its converters know the types with
    32-bit offsets only."""
    import pyarrow as pa
    from .. import arrow_interop

    def narrow(t):
        if pa.types.is_large_string(t):
            return pa.string()
        if pa.types.is_large_binary(t):
            return pa.binary()
        if pa.types.is_large_list(t) or pa.types.is_list(t):
            return pa.list_(narrow(t.value_type))
        if pa.types.is_struct(t):
            return pa.struct([(f.name, narrow(f.type)) for f in t])
        return t
    return narrow(arrow_interop.dtype_to_arrow(dtype))


def _host_convert(s: Series, dtype: DataType, quote: bool) -> Series:
    """The value texts of `s` (null where it is null) as `dtype`, read by
    pyarrow.json with a one-field explicit schema.  `quote`: the texts are
    string contents, else JSON values."""
    import pyarrow as pa
    import pyarrow.json as pajson
    c = s.cpu()
    if len(c) == 0:
        return Series.from_pylist(s.name, [], dtype, device=s.device)
    off = c.offsets.numpy()
    buf = c.data.numpy().tobytes() if len(c.data) else b""
    valid = None if c.validity is None else c.validity.numpy()
    lines = []
    for i in range(len(c)):
        t = buf[off[i]:off[i + 1]]
        if valid is not None and not valid[i]:
            t = b"null"
        elif quote:
            t = _pyjson.dumps(t.decode("utf-8")).encode()
        lines.append(b'{"v":' + t + b"}\n")
    text = b"".join(lines)
    tbl = pajson.read_json(
        pa.BufferReader(text),
        read_options=pajson.ReadOptions(
            use_threads=False, block_size=max(MAX_RECORD, len(text) + 1)),
        parse_options=pajson.ParseOptions(
            explicit_schema=pa.schema([("v", _arrow_type(dtype))]),
            unexpected_field_behavior="error"))
    assert tbl.num_rows == len(c)
    if _allowed(dtype) is None:
        rb = RecordBatch.from_arrow(tbl.rename_columns([s.name]),
                                    device=s.device)
        if rb.columns[0].dtype != dtype:
            raise pa.ArrowInvalid(f"{s.name}: {rb.columns[0].dtype}")
        return rb.columns[0]
    col = tbl.column(0).combine_chunks()
    ok = torch.from_numpy(col.is_valid().to_numpy(zero_copy_only=False))
    if pa.types.is_timestamp(col.type):
        col = col.cast(pa.int64())
    # numpy would hold the nulls as NaN in a float64 array: fill them
    data = torch.from_numpy(
        col.fill_null(0).to_numpy(zero_copy_only=False).copy())
    return Series(s.name, dtype, data=data.to(s.device),
                  validity=ok.to(s.device))


def _typed(s: Series, dtype: DataType) -> Series:
    """The texts `s` (numbers, or string contents) as `dtype`."""
    k = dtype.kind
    if k == TypeKind.STRING:
        return s
    if _allowed(dtype) is None or len(s) == 0:
        return _host_convert(s, dtype, False)
    if k == TypeKind.TIMESTAMP:
        values, status = parse._run_kernel(s, dtype, ord("T"))
        values = torch.div(values, 10 ** 6, rounding_mode="floor")
    else:
        values, status = parse._run_kernel(s, dtype)
    return parse._merge(s, dtype, values, status,
                        lambda t: _host_convert(t, dtype,
                                                k == TypeKind.TIMESTAMP))


# ---------------------------------------------------------------------------
# one chunk
# ---------------------------------------------------------------------------

def key_table(names: List[str], device) -> torch.Tensor:
    """The names as json_fields reads them from LDS."""
    return parse._native().json_keys(
        [n.encode("utf-8") for n in names]).to(device)


def keys_fit(names: List[str]) -> bool:
    return 0 < len(names) <= MAX_KEYS and \
        sum(len(n.encode("utf-8")) for n in names) <= MAX_KEY_BYTES


def decode_chunk(bytes_dev: torch.Tensor, names: List[str],
                 schema: Dict[str, DataType], columns: Optional[List[str]],
                 final: bool, keys: Optional[torch.Tensor] = None
                 ) -> Tuple[RecordBatch, int]:
    """(batch of the selected columns, bytes consumed) of a chunk that begins
    at a record start.  `names` are the scan schema's, in its order.  A final
    chunk ends in a newline."""
    import pyarrow as pa
    nat = parse._native()
    dev = bytes_dev.device
    columns = list(names) if columns is None else list(columns)
    if keys is None:
        keys = key_table(names, dev)
    mask, depth_in, tok_base, close_base, info = nat.json_structure(bytes_dev)
    err, cont, consumed, ntok, end_parity, _, _, closes = info.tolist()
    if cont != 0:
        err |= 2
    _refuse(err, _STRUCTURE)
    if final and end_parity:
        raise JsonFallback("open_string_at_end")
    if consumed == 0:
        raise JsonFallback("no_record_end")
    if ntok == 0 and bool((bytes_dev[:consumed] > 32).any()):
        raise JsonFallback("irregular")     # text, but no record
    tokens = nat.json_tokens(bytes_dev, mask, depth_in, tok_base, close_base,
                             ntok)
    field_tok, row_end = nat.json_fields(bytes_dev, tokens, consumed, closes,
                                         keys, len(names), info)
    host = info.tolist()
    _refuse(host[0], _KEYS, consumed)
    nrows = host[6]
    kinds, raw_start, raw_len, ulen, seen = nat.json_values(
        bytes_dev, tokens, field_tok, row_end, nrows, info)

    # the columns to build: the selected ones, and every column that only
    # the host function can check
    work = [names.index(c) for c in columns]
    work += [j for j, n in enumerate(names)
             if _allowed(schema[n]) is None and j not in work]
    lens = torch.empty((len(work), nrows), dtype=torch.int64, device=dev)
    for w, j in enumerate(work):
        ok = _allowed(schema[names[j]])
        if ok is None:
            lens[w] = raw_len[j]
        elif ok & _STRING:
            lens[w] = ulen[j]
        else:
            lens[w] = raw_len[j] * (kinds[j] == 3)
    offs = torch.zeros((len(work), nrows + 1), dtype=torch.int64, device=dev)
    torch.cumsum(lens, 1, out=offs[:, 1:])
    host = torch.cat([info.to(torch.int64), seen.to(torch.int64),
                      offs[:, -1]]).tolist()
    _refuse(host[0], _VALUES, consumed)
    if host[5] >= MAX_RECORD:
        raise JsonFallback("long_record", consumed)
    seen_host, totals = host[8:8 + len(names)], host[8 + len(names):]
    for j, n in enumerate(names):
        ok = _allowed(schema[n])
        if ok is not None and seen_host[j] & 63 & ~ok:
            raise JsonFallback("type_mismatch", consumed)

    cols = []
    for w, j in enumerate(work):
        name, dtype = names[j], schema[names[j]]
        ok, bits = _allowed(dtype), seen_host[j]
        valid = kinds[j] != 0 if bits & _NULL else None
        if ok is not None and not ok & (_STRING | _NUMBER):
            s = Series(name, dtype, data=kinds[j] == 2, validity=valid)
        else:
            string = ok is not None and bool(ok & _STRING)
            unescape = string and bool(bits & _ESCAPES)
            # a string's copy starts behind its opening quote
            start = raw_start[j] + 1 if string and not unescape \
                else raw_start[j]
            data = nat.json_extract(bytes_dev, kinds[j], start.contiguous(),
                                    raw_len[j], offs[w], totals[w], unescape)
            try:
                s = _typed(Series(name, DataType.string(), data=data,
                                  offsets=offs[w], validity=valid), dtype)
            except pa.ArrowInvalid:
                raise JsonFallback(None, consumed) from None
        if w < len(columns):
            cols.append(s)
    return RecordBatch(cols, num_rows=nrows), consumed


# ---------------------------------------------------------------------------
# a file
# ---------------------------------------------------------------------------

def eligible(path, read_options: Optional[dict], device) -> bool:
    """The device path reads local, uncompressed files on a GPU when
    `device_decode=True` asks for it.  None stays on the host: measured end
    to end (benchmarks/bench_json.py) the device path is not faster, the
    file read and the upload cost what the kernels save."""
    ro = read_options or {}
    if ro.get("device_decode") is not True or "schema" not in ro or \
            not str(device).startswith("cuda") or not isinstance(path, str):
        return False
    from ..io.object_store import is_remote
    return not is_remote(path) and not path.endswith(_COMPRESSED)


def _host_records(raw: bytes, names, schema, columns,
                  device) -> Iterator[RecordBatch]:
    """Records `raw` through pyarrow.json under the scan schema."""
    import pyarrow as pa
    import pyarrow.json as pajson
    a_schema = pa.schema([(n, _arrow_type(schema[n])) for n in names])
    tbl = pajson.read_json(
        pa.BufferReader(raw),
        parse_options=pajson.ParseOptions(explicit_schema=a_schema))
    if columns:
        tbl = tbl.select(columns)
    yield RecordBatch.from_arrow(tbl, device=device)


def read_file_device(path: str, columns: Optional[List[str]],
                     read_options: dict, device,
                     raw: Optional[bytes] = None) -> Iterator[RecordBatch]:
    """Batches of a local JSON-lines file decoded on `device`; `raw` is the
    file's content where a prefetching thread has read it already."""
    from ..io import readers
    schema = read_options["schema"]
    names = list(schema)
    if not keys_fit(names) or \
            any(c not in schema for c in columns or []):
        STATS["host_chunks"] += 1
        STATS["reasons"].append("names")
        yield from readers._read_json(
            path if raw is None else io.BytesIO(raw), columns, device)
        return
    keys = None
    with (io.BytesIO(raw) if raw is not None else open(path, "rb")) as f:
        block_bytes = BLOCK_BYTES
        tail, eof = b"", False
        while not eof:
            block = f.read(block_bytes)
            eof = len(block) < block_bytes
            buf = tail + block
            if eof and buf and not buf.endswith(b"\n"):
                buf += b"\n"
            if not buf:
                break
            try:
                if len(buf) > MAX_CHUNK:
                    raise JsonFallback("no_record_end")
                with torch.cuda.device(device):
                    if keys is None:
                        keys = key_table(names, device)
                    rb, consumed = decode_chunk(_upload(buf, device), names,
                                                schema, columns, eof, keys)
            except JsonFallback as e:
                if e.reason == "no_record_end" and not eof and \
                        len(buf) <= MAX_CHUNK:
                    tail = buf          # grow the chunk by the next block
                    continue
                STATS["host_chunks"] += 1
                if e.reason is not None:
                    STATS["reasons"].append(e.reason)
                if e.consumed:
                    yield from _host_records(buf[:e.consumed], names, schema,
                                             columns, device)
                    tail = buf[e.consumed:]
                    continue
                yield from _host_records(buf + f.read(), names, schema,
                                         columns, device)
                return
            STATS["device_chunks"] += 1
            tail = buf[consumed:]
            if len(rb):
                yield rb

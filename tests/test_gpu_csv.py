"""Device CSV decode (csrc/csv.hip, daft_amd/kernels/csv.py) against
`pyarrow.csv.read_csv` on the same bytes with the same column types; every
comparison is exact, floats by their 8 bytes."""
import gzip
import io
import random
import struct

import pyarrow as pa
import pyarrow.csv as pacsv
import pytest
import torch

import daft_amd as daft
from daft_amd import DataType
from daft_amd.kernels import csv as dcsv

pytestmark = pytest.mark.gpu

LONG = '"' + 'z,""\n' * 1700 + '"'          # 8502 bytes: spans three tiles
# name -> (second field, offset from its start of the byte that is slid over
# the border)
SPOTS = {
    "open_quote": ('"q,1"', 0),
    "close_quote": ('"q,1"', 4),
    "quote_pair": ('"x""y"', 3),
    "crlf": ("w", 4),                        # the '\n' of "w,t\r\n"
    "delim_last": ("w", -1),                 # the delimiter before the field
    "three_tiles": (LONG, 0),
    "utf8_split": ("€\U0001F600", 1),
}


def build_text(nrows: int, spot: str, at: int, ncols: int = 3) -> bytes:
    """A header and `nrows` records of `ncols` fields; in the first record
    the spot's byte sits at offset `at`."""
    rng = random.Random(nrows * 7919 + at)
    pool = ["", "7", "-12", 'q"q', "a,b", "l1\nl2", "é中", "x" * 300,
            "r\r\nn", '""']
    names = [f"c{i}" for i in range(ncols)]
    out = [(",".join(names) + "\n").encode()]
    for r in range(nrows):
        vals = [rng.choice(pool) for _ in range(ncols)]
        cells = ['"' + v.replace('"', '""') + '"'
                 if any(ch in v for ch in '",\r\n') or rng.random() < 0.2
                 or (ncols == 1 and not v) else v for v in vals]
        end = "\n"
        if r == 0 and ncols >= 3:
            field, key = SPOTS[spot]
            cells[1], cells[2:] = field, ["t"] * (ncols - 2)
            end = "\r\n" if spot == "crlf" else "\n"
            cells[0] = "f" * (at - len(out[0]) - 1 - key)
        out.append((",".join(cells) + end).encode())
    return b"".join(out)


def oracle(text: bytes, types: dict, columns=None) -> dict:
    tbl = pacsv.read_csv(
        io.BytesIO(text),
        parse_options=pacsv.ParseOptions(newlines_in_values=True),
        convert_options=pacsv.ConvertOptions(column_types=types,
                                             include_columns=columns))
    return tbl.to_pydict()


def decode(text: bytes, columns=None) -> dict:
    names = text.split(b"\n", 1)[0].decode().split(",")
    dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    rb, consumed = dcsv.decode_chunk(
        dev, len(names), names, {n: DataType.string() for n in names},
        columns, ",", True, True)
    assert consumed == len(text)
    return {c.name: c.to_pylist() for c in rb.columns}


def bits(values):
    return [struct.pack("<d", v) if isinstance(v, float) else v
            for v in values]


@pytest.fixture(autouse=True)
def stats():
    dcsv.STATS.update(device_chunks=0, host_chunks=0, reasons=[])
    return dcsv.STATS


# without records there is no spot to slide: one header-only case
@pytest.mark.parametrize("spot,at,nrows", [("open_quote", 4096, 0)] + [
    (spot, at, nrows) for spot in SPOTS for at in (4095, 4096, 4097, 4112)
    for nrows in (1, 255, 257)])
def test_structure(spot, at, nrows):
    text = build_text(nrows, spot, at)
    if nrows:
        field, key = SPOTS[spot]
        want = b"\n" if spot == "crlf" else b"," if key < 0 \
            else field.encode()[key:key + 1]
        assert text[at:at + 1] == want
    types = {n: pa.large_string() for n in ("c0", "c1", "c2")}
    assert decode(text) == oracle(text, types)


@pytest.mark.parametrize("columns", [None, ["c0"], ["c4"], ["c2"],
                                     ["c4", "c0"]])
@pytest.mark.parametrize("ncols", [1, 5])
def test_projection(ncols, columns, tmp_path, stats):
    if columns and ncols == 1:
        columns = ["c0"]
    text = build_text(257, "quote_pair", 4096, ncols)
    types = {f"c{i}": pa.large_string() for i in range(ncols)}
    want = oracle(text, types, columns)
    assert decode(text, columns) == want
    # the same through the reader, the file's last newline missing
    path = tmp_path / "t.csv"
    path.write_bytes(text[:-1])
    df = daft.read_csv(str(path))
    got = (df.select(*columns) if columns else df).to_pydict()
    assert got == want
    assert stats["host_chunks"] == 0 and stats["device_chunks"] >= 1


TYPED = {"i": DataType.int64(), "f": DataType.float64(),
         "d": DataType.date(), "m": DataType.decimal128(12, 2),
         "s": DataType.string(), "j": DataType.int32(),
         "b": DataType.bool(), "t": DataType.timestamp("us", None)}
TYPED_ARROW = {"i": pa.int64(), "f": pa.float64(), "d": pa.date32(),
               "m": pa.decimal128(12, 2), "s": pa.large_string(),
               "j": pa.int32(), "b": pa.bool_(), "t": pa.timestamp("us")}


def typed_text() -> bytes:
    rng = random.Random(5)
    special = [
        ["", "", "", "", "", "", "", ""],
        ['" 5"', "1e400", "2024-02-29", "1.500", '"a,""b""\nc"', "-7",
         "true", "2024-02-29 01:02:03"],
        ["NULL", "nan", "NULL", "NULL", "NULL", "NULL", "NULL", "NULL"],
        ["007", "12345678901234567890", "0001-01-01", "+1.5", '""', "007",
         "0", "1969-12-31T23:59:59"],
        ["-9223372036854775808", "-1e-400", "9999-12-31", "-.5", "é",
         "2147483647", "False", "2000-01-01 00:00:00"],
        ["9223372036854775807", "+.5", "1970-01-01 ", "9999999999.99", " x ",
         "-2147483648", "1", "2262-04-11 23:47:16"],
    ]
    rows = [",".join(TYPED)] + [",".join(r) for r in special]
    for _ in range(600):
        rows.append(",".join([
            str(rng.randrange(-10**12, 10**12)), repr(rng.uniform(-1e6, 1e6)),
            "%04d-%02d-%02d" % (rng.randint(1900, 2100), rng.randint(1, 12),
                                rng.randint(1, 28)),
            "%d.%02d" % (rng.randrange(10**6), rng.randrange(100)),
            '"c,%d\nd"' % rng.randrange(100), str(rng.randrange(-999, 999)),
            rng.choice(["true", "false"]),
            "2020-01-%02d 10:00:00" % rng.randint(1, 28)]))
    return ("\n".join(rows) + "\n").encode()


def test_types(tmp_path, stats, monkeypatch):
    text = typed_text()
    path = tmp_path / "typed.csv"
    path.write_bytes(text)
    want = {k: bits(v) for k, v in oracle(text, TYPED_ARROW).items()}
    got = daft.read_csv(str(path), schema=TYPED).to_pydict()
    assert {k: bits(v) for k, v in got.items()} == want
    assert stats["host_chunks"] == 0 and stats["device_chunks"] == 1
    # tails carry over many times: 4099-byte blocks give the same table
    monkeypatch.setattr(dcsv, "BLOCK_BYTES", 4099)
    again = daft.read_csv(str(path), schema=TYPED).to_pydict()
    assert {k: bits(v) for k, v in again.items()} == want
    assert stats["host_chunks"] == 0 and stats["device_chunks"] > 8


def outcome(path, **kw):
    try:
        return daft.read_csv(str(path), **kw).to_pydict()
    except Exception as e:          # compared by type
        return type(e)


EXPLICIT = {"a": DataType.int64(), "b": DataType.string()}
UNSIGNED = {"a": DataType.uint8(), "b": DataType.string()}


# schema=EXPLICIT where inference would refuse the file before any decode
@pytest.mark.parametrize("reason,body,schema", [
    ("irregular_quote", b'a,b\n1,x"y\n2,z\n', None),
    ("irregular_quote", b'a,b\n1,"x"y\n2,z\n', None),
    ("blank_line", b"a,b\n1,x\n\n2,z\n", None),
    ("ragged", b"a,b\n1,x\n2,z,9\n3,w\n", EXPLICIT),
    ("invalid_utf8", b"a,b\n1,x\xffy\n2,z\n", None),
    ("bare_cr", b"a\r1\r2\n", None),
    ("bare_cr", b"a,b\n1\r2,3\n", EXPLICIT),
])
def test_fallbacks(reason, body, schema, tmp_path, stats):
    path = tmp_path / "f.csv"
    path.write_bytes(body)
    host = outcome(path, schema=schema, device_decode=False)
    assert stats == {"device_chunks": 0, "host_chunks": 0, "reasons": []}
    assert repr(outcome(path, schema=schema)) == repr(host)
    assert stats == {"device_chunks": 0, "host_chunks": 1,
                     "reasons": [reason]}


@pytest.mark.parametrize("body,schema,want", [
    # pyarrow refuses "+5" as int64 and "-0" as uint8, which the parse kernels
    # would accept.  The host path does not apply the schema's types but
    # infers float64 and int64, and the device path has to give the same: the
    # pre-check hands the row to pyarrow, pyarrow refuses it, and the chunk is
    # read by inference, as a host chunk without a reason.
    (b"a,b\n1,x\n+5,z\n", EXPLICIT, {"a": [1.0, 5.0], "b": ["x", "z"]}),
    (b"a,b\n1,x\n-0,z\n", UNSIGNED, {"a": [1, 0], "b": ["x", "z"]}),
])
def test_values_pyarrow_refuses(body, schema, want, tmp_path, stats):
    path = tmp_path / "f.csv"
    path.write_bytes(body)
    host = daft.read_csv(str(path), schema=schema,
                         device_decode=False).to_pydict()
    assert repr(host) == repr(want)
    got = daft.read_csv(str(path), schema=schema).to_pydict()
    assert repr(got) == repr(want)
    assert stats == {"device_chunks": 0, "host_chunks": 1, "reasons": []}


def test_unchanged_paths(tmp_path, stats):
    body = b"a,b\n1,x\n2,y\n"
    (tmp_path / "p.csv").write_bytes(body)
    (tmp_path / "p.csv.gz").write_bytes(gzip.compress(body))
    want = {"a": [1, 2], "b": ["x", "y"]}
    assert daft.read_csv(str(tmp_path / "p.csv"),
                         device_decode=False).to_pydict() == want
    assert daft.read_csv(str(tmp_path / "p.csv.gz")).to_pydict() == want
    assert stats == {"device_chunks": 0, "host_chunks": 0, "reasons": []}

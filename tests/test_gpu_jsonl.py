"""Device JSON-lines decode (csrc/json.hip, daft_amd/kernels/jsonl.py) against
`pyarrow.json.read_json` on the same bytes under the same explicit schema;
every comparison is exact, floats by their 8 bytes."""
import io
import random
import struct

import pyarrow as pa
import pyarrow.json as pajson
import pytest
import torch

import daft_amd as daft
from daft_amd import DataType
from daft_amd.arrow_interop import dtype_to_arrow
from daft_amd.io import read_jsonl
from daft_amd.kernels import jsonl

pytestmark = pytest.mark.gpu

S = DataType.string()
BS = "\\"
# 8502 bytes of value text: spans three tiles
LONG = ('"' + (BS + "n" + BS + '"}{,:[z') * 850 + '"').encode()
TAIL = b',"t":"x"}'
# name -> (value of "s" in the first record, offset from its start of the
# byte that is slid over the border)
SPOTS = {
    "open_quote": (b'"q,1"', 0),
    "close_quote": (b'"q,1"', 4),
    "escaped_quote": (b'"x\\"y"', 3),
    "backslash_before_close": (b'"x\\\\"', 4),
    "backslash_run": (b'"a\\\\\\\\\\"b"', 7),
    "surrogate_pair": (b'"\\ud83d\\ude00"', 7),
    "multi_byte": ('"€\U0001F600"'.encode(), 2),
    "colon": (b'"w"', -1),
    "comma": (b'"w"', 3),
    "brace": (b'"w"', 3 + len(TAIL) - 1),
    "crlf": (b'"w"', 3 + len(TAIL) + 1),
    "three_tiles": (LONG, 0),
}
POOL = ['""', '"7"', '"q\\"q"', '"a,b"', '"l1\\nl2\\t\\/"', '"é中"',
        '"' + "x" * 300 + '"', '"\\u00e9\\ud83d\\ude00\\u4e2d"', '"}{[:"',
        '"\\\\"', "null"]


def build_text(nrows: int, spot: str, at: int) -> bytes:
    """`nrows` records of the string keys k, s, t; in the first one the
    spot's byte sits at offset `at`."""
    rng = random.Random(nrows * 7919 + at)
    value, key = SPOTS[spot]
    head = b'{"k":"'
    pad = at - key - len(head) - len(b'","s":')
    out = [head + b"f" * pad + b'","s":' + value + TAIL +
           (b"\r\n" if spot == "crlf" else b"\n")]
    for _ in range(nrows - 1):
        out.append(("{" + ",".join(f'"{n}":{rng.choice(POOL)}'
                                   for n in "kst") + "}\n").encode())
    return b"".join(out)


def oracle(text: bytes, types: dict, columns=None) -> dict:
    schema = pa.schema([(n, dtype_to_arrow(t)) for n, t in types.items()])
    tbl = pajson.read_json(
        io.BytesIO(text),
        parse_options=pajson.ParseOptions(explicit_schema=schema))
    return (tbl.select(columns) if columns else tbl).to_pydict()


def decode(text: bytes, types: dict, columns=None) -> dict:
    dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    rb, consumed = jsonl.decode_chunk(dev, list(types), types, columns, True)
    assert consumed == len(text)
    return {c.name: c.to_pylist() for c in rb.columns}


def bits(table: dict) -> dict:
    return {k: [struct.pack("<d", v) if isinstance(v, float) else v
                for v in vs] for k, vs in table.items()}


@pytest.fixture(autouse=True)
def stats():
    jsonl.STATS.update(device_chunks=0, host_chunks=0, reasons=[])
    return jsonl.STATS


@pytest.mark.parametrize("nrows", [1, 255, 257])
@pytest.mark.parametrize("at", [4095, 4096, 4097, 4112])
@pytest.mark.parametrize("spot", list(SPOTS))
def test_structure(spot, at, nrows):
    text = build_text(nrows, spot, at)
    value, key = SPOTS[spot]
    want = (b'","s":' + value + TAIL + b"\r\n")[6 + key:][:1]
    assert text[at:at + 1] == want
    types = {"k": S, "s": S, "t": S}
    assert decode(text, types) == oracle(text, types)


def keyed_text(nrows: int) -> bytes:
    """Records with shuffled, absent and null keys, `{}`, blank lines,
    whitespace around every token and two objects on one line."""
    rng = random.Random(nrows)
    lines = ['{"c0":"a","c1":1,"c2":"b","c3":"c","c4":"d"}']
    for r in range(nrows):
        names = rng.sample(["c0", "c1", "c2", "c3", "c4"], rng.randint(0, 5))
        sp = rng.choice(["", " ", " \t "])
        fields = [f'{sp}"{n}"{sp}:{sp}' +
                  ("null" if rng.random() < 0.2 else str(r) if n == "c1"
                   else rng.choice(POOL)) + sp for n in names]
        rec = "{" + ",".join(fields) + (sp if fields else "") + "}"
        if r % 7 == 3:
            rec += " " + '{"c4":"two","c0":"on a line"}'
        lines.append(sp + rec + sp + ("\n" if r % 5 == 0 else ""))
    return ("\n".join(lines) + "\n").encode()


@pytest.mark.parametrize("columns", [None, ["c0"], ["c4"], ["c3", "c1"]])
def test_keys_and_projection(columns, tmp_path, stats):
    text = keyed_text(300)
    types = {"c0": S, "c1": DataType.int64(), "c2": S, "c3": S, "c4": S}
    want = oracle(text, types, columns)
    assert decode(text, types, columns) == want
    # the same through the reader, the file's last newline missing
    path = tmp_path / "t.jsonl"
    path.write_bytes(text[:-1])
    df = daft.read_json(str(path), device_decode=True)
    got = (df.select(*columns) if columns else df).to_pydict()
    assert got == want
    assert stats["host_chunks"] == 0 and stats["device_chunks"] >= 1


INTS = ["9223372036854775807", "-9223372036854775808", "0", "-0", "12345"]
FLOATS = ["-0.0", "1E+5", "4.9e-324", "0.1234567890123456",
          "12345678.901234567", "-1.7976931348623157e308", "3", "2.5e-3"]
STRINGS = ['"\\" \\\\ \\/ \\b \\f \\n \\r \\t \\u0041 \\u00e9 \\u4e2d '
           '\\ud83d\\ude00"', '""', '"plain"', '"é中\U0001F600"']
STAMPS = ['"2024-01-02T03:04:05"', '"2024-01-02 03:04:05"',
          '"1969-12-31T23:59:59Z"', '"2024-02-29"']


@pytest.mark.parametrize("nrows", [257, 4099])
def test_types(nrows, tmp_path, stats):
    rng = random.Random(nrows)
    lines = []
    for r in range(nrows):
        rec = {"i": INTS[r % len(INTS)], "f": FLOATS[r % len(FLOATS)],
               "b": ["true", "false"][r % 2], "s": STRINGS[r % len(STRINGS)],
               "ts": STAMPS[r % len(STAMPS)],
               "st": '{"a":%d,"b":"x}"}' % r, "l": "[%d,2]" % r, "z": "null"}
        # "i" is never absent: the host reader takes an int64 column with
        # nulls through float64, which does not hold the limits
        keep = [k for k in rec if r < 8 or k == "i" or rng.random() < 0.9]
        lines.append("{" + ",".join(f'"{k}":{rec[k]}' for k in keep) + "}")
    path = tmp_path / "t.jsonl"
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    host = daft.read_json(str(path), device_decode=False)
    dev = read_jsonl(str(path), device_decode=True)
    got, want = dev.collect(), host.collect()
    # the dtypes of the batches themselves, not of the plan
    assert [[(c.name, c.dtype) for c in p.columns]
            for p in got.iter_partitions()] == \
        [[(c.name, c.dtype) for c in p.columns]
         for p in want.iter_partitions()]
    assert bits(got.to_pydict()) == bits(want.to_pydict())
    assert stats["host_chunks"] == 0 and stats["device_chunks"] >= 1


def test_chunk_seams(tmp_path, monkeypatch, stats):
    # cuts fall inside strings, escapes, keys and numbers
    text = keyed_text(300) + build_text(257, "surrogate_pair", 4097)
    types = {"c0": S, "c1": DataType.int64(), "c2": S, "c3": S, "c4": S,
             "k": S, "s": S, "t": S}
    path = tmp_path / "t.jsonl"
    path.write_bytes(text)
    monkeypatch.setattr(jsonl, "BLOCK_BYTES", 4231)
    assert daft.read_json(str(path), device_decode=True).to_pydict() == \
        oracle(text, types)
    assert stats["host_chunks"] == 0 and stats["device_chunks"] > 1


GOOD = b'{"a":1,"s":"x","f":1.5}\n' * 3
# name -> (a line added to GOOD, or a second file's content; the reason)
FALLBACKS = {
    "escaped_key": (b'{"\\u0061":2,"s":"y"}\n', "escaped_key"),
    "unknown_key": (b'{"a":2,"zz":1}\n', "unknown_key"),
    "duplicate_key": (b'{"a":2,"a":3}\n', "duplicate_key"),
    "plus": (b'{"a":+1}\n', "irregular"),
    "leading_zero": (b'{"a":01}\n', "irregular"),
    "lone_surrogate": (b'{"s":"\\ud83d"}\n', "bad_escape"),
    "raw_tab": (b'{"s":"a\tb"}\n', "control_char"),
    "invalid_utf8": (b'{"s":"\xff"}\n', "invalid_utf8"),
    "string_in_int64": (b'{"a":"x"}\n', "type_mismatch"),
    "1e400": (b'{"f":1e400}\n', None),
    "trailing_comma": (b'{"a":1,}\n', "irregular"),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallback(case, tmp_path, stats):
    line, reason = FALLBACKS[case]
    if case == "unknown_key":
        (tmp_path / "a.jsonl").write_bytes(GOOD)
        (tmp_path / "b.jsonl").write_bytes(line + GOOD)
    else:
        (tmp_path / "a.jsonl").write_bytes(GOOD + line + GOOD)

    def run(device_decode):
        try:
            return bits(daft.read_json(str(tmp_path / "*.jsonl"),
                                       device_decode=device_decode)
                        .to_pydict())
        except Exception as e:          # the type is what is compared
            return type(e)
    want, got = run(False), run(True)
    assert got == want
    if isinstance(got, dict) and reason:
        assert reason in stats["reasons"]

"""Device Parquet decode (csrc/parquet.hip, daft_amd/kernels/parquet.py)
against `pyarrow.parquet.read_table` on the same file; every comparison is
exact, floats by their bytes."""
import datetime
import decimal
import random
import struct

import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import daft_amd as daft
from daft_amd import col
from daft_amd.io import readers
from daft_amd.kernels import native_required, parquet as dpq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def stats():
    dpq.STATS.update(device_chunks=0, host_chunks=0, reasons=[])
    return dpq.STATS


def bits(values):
    return [struct.pack("<d", v) if isinstance(v, float) else v
            for v in values]


def read(path, **read_options):
    return list(readers.read_file(str(path), "parquet", None, None, None, {},
                                  read_options, DEV))


def check_file(path, stats, host_chunks=0):
    """The device path's rows against pyarrow's, its dtypes against the host
    path's."""
    want = pq.read_table(path).to_pydict()
    parts = read(path)
    assert stats["host_chunks"] == host_chunks
    assert [c.name for c in parts[0].columns] == list(want)
    for name in want:
        got = [v for rb in parts for v in rb.column(name).to_pylist()]
        assert bits(got) == bits(want[name]), name
    seen = dict(stats, reasons=list(stats["reasons"]))
    host = read(path, device_decode=False)
    assert [[(c.name, c.dtype) for c in rb.columns] for rb in parts] == \
        [[(c.name, c.dtype) for c in rb.columns] for rb in host]
    assert dpq.STATS == seen        # device_decode=False counts nothing


# ---------------------------------------------------------------------------
# 1. the Snappy kernel alone
# ---------------------------------------------------------------------------

def mix(rng):
    words = [b"the ", b"quick ", b"fox ", b"0123456789", b"ab"]
    out = []
    while sum(map(len, out)) < 300_000:
        r = rng.random()
        out.append(rng.choice(words) if r < 0.6 else
                   rng.randbytes(7) if r < 0.8 else
                   bytes(rng.randint(1, 89)))
    return b"".join(out)


RNG = random.Random(5)
PLAIN_TEXTS = [b"", b"a" * 100, b"abc" * 1000, RNG.randbytes(61),
               RNG.randbytes(300), RNG.randbytes(70000), b"xy" * 40000,
               mix(RNG)]
HANDWRITTEN = [
    b"\x10\x1cabcdefgh\x1f\x08\x00\x00\x00",          # 4-byte-offset copy
    b"\x46\xf8\x45\x00\x00" + bytes(range(70)),       # 3 length bytes
]
MALFORMED = [                       # (stream, size the page header promises)
    (b"\x10\x1cabcdefgh\x1e\x09\x00", 16),            # offset 9 after 8 bytes
    (b"\x10\x1cabcdefgh\x1e\x00\x00", 16),            # offset 0
    (b"\x0c\x1cabcdefgh\x1e\x08\x00", 12),            # copy past the length
    (b"\x10\x3cabcdefgh", 16),                        # cut inside a literal
]


def test_snappy_kernel():
    nat = native_required()
    good = [pa.compress(t, codec="snappy", asbytes=True)
            for t in PLAIN_TEXTS] + HANDWRITTEN
    want = PLAIN_TEXTS + [pa.decompress(s, 16 if i == 0 else 70,
                                        codec="snappy", asbytes=True)
                          for i, s in enumerate(HANDWRITTEN)]
    assert want[-2] == b"abcdefghabcdefgh"
    # malformed pages between the good ones, all in one launch
    pages = [(s, len(w), w) for s, w in zip(good, want)]
    for i, (s, n) in enumerate(MALFORMED):
        pages.insert(2 * i + 1, (s, n, None))
    src = b"".join(p[0] for p in pages)
    table, at, out_at = [], 0, len(src)
    for s, n, _ in pages:
        table.append([at, len(s), out_at, n] + [0] * 8)
        at, out_at = at + len(s), out_at + n
    buf = torch.zeros(out_at, dtype=torch.uint8)      # sized exactly
    buf[:len(src)] = torch.frombuffer(bytearray(src), dtype=torch.uint8)
    buf = buf.to(DEV)
    status = torch.zeros(len(pages), dtype=torch.int32, device=DEV)
    nat.pq_snappy(buf, torch.tensor(table, device=DEV), status)
    host, status = buf.cpu().numpy().tobytes(), status.tolist()
    for (s, n, w), row, st in zip(pages, table, status):
        if w is None:
            assert st != 0
        else:
            assert st == 0 and host[row[2]:row[2] + n] == w


# ---------------------------------------------------------------------------
# 2. the RLE / bit-packed hybrid, through files
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 504, 505, 4097])
@pytest.mark.parametrize("card", [1, 2, 3, 5, 129, 513, 70001])
def test_hybrid(card, rows, nulls, tmp_path, stats):
    if card > rows:
        pytest.skip("more distinct values than rows")
    rng = random.Random(card * 8191 + rows)
    vals = []
    while len(vals) < rows - card:
        v = rng.randrange(card)
        vals.extend([v] * rng.randint(8, 40) if rng.random() < 0.3 else [v])
    # every value of the dictionary at least once
    vals = [v * 10**12 + v for v in vals[:rows - card] + list(range(card))]
    if nulls:
        vals = [None if rng.random() < 0.1 else v for v in vals]
    path = tmp_path / "h.parquet"
    pq.write_table(pa.table({"x": pa.array(vals, pa.int64())}), path,
                   compression="NONE", data_page_size=1024,
                   use_dictionary=True)
    check_file(path, stats)
    assert stats["device_chunks"] == 1


# ---------------------------------------------------------------------------
# 3. types x page version x codec x nulls
# ---------------------------------------------------------------------------

def type_table(n, null_pattern):
    rng = random.Random(n)
    dec = decimal.Decimal

    def column(make, typ, all_null=False):
        vals = [None if all_null or (null_pattern and rng.random() < 0.1)
                else make() for _ in range(n)]
        return pa.array(vals, typ)
    day0 = datetime.date(1970, 1, 1)
    return pa.table({
        "i8": column(lambda: rng.randint(-128, 127), pa.int8()),
        "i32": column(lambda: rng.randint(-2**31, 2**31 - 1), pa.int32()),
        "i64": column(lambda: rng.randint(-2**63, 2**63 - 1), pa.int64()),
        "u32": column(lambda: rng.randint(0, 2**32 - 1), pa.uint32()),
        "f32": column(lambda: struct.unpack("<f", rng.randbytes(3) + b"\x42")[0],
                      pa.float32()),
        "f64": column(lambda: rng.uniform(-1e300, 1e300), pa.float64()),
        "b": column(lambda: rng.random() < 0.5, pa.bool_()),
        "d": column(lambda: day0 + datetime.timedelta(rng.randint(-9999, 29999)),
                    pa.date32()),
        "ts": column(lambda: rng.randint(-2**50, 2**50), pa.timestamp("us")),
        "dec12": column(lambda: dec(rng.randint(-10**12 + 1, 10**12 - 1))
                        .scaleb(-2), pa.decimal128(12, 2)),
        "dec5": column(lambda: dec(rng.randint(-99999, 99999)).scaleb(-1),
                       pa.decimal128(5, 1)),
        "s": column(lambda: rng.choice(["a", "bb", "ccc", ""]),
                    pa.large_string()),
        "bin": column(lambda: rng.choice([b"\x00\xff", b"", b"z" * 70]),
                      pa.binary()),
        "nul": column(lambda: rng.randint(0, 9), pa.int64(),
                      all_null=null_pattern == "column"),
    })


@pytest.mark.parametrize("null_pattern", [None, "tenth", "column"])
@pytest.mark.parametrize("compression", ["NONE", "SNAPPY"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_types(version, compression, null_pattern, tmp_path, stats):
    path = tmp_path / "t.parquet"
    pq.write_table(type_table(70_000, null_pattern), path,
                   compression=compression, data_page_version=version,
                   data_page_size=4096, row_group_size=50_000)
    check_file(path, stats)
    assert stats["reasons"] == [] and stats["device_chunks"] == 2 * 14


# ---------------------------------------------------------------------------
# 4. what stays on the host
# ---------------------------------------------------------------------------

UNIQUE = [f"{i:09d}-{i * 7919 % 1000003}" for i in range(30000)]
FALLBACKS = {
    "codec": (pa.array(range(30000), pa.int32()),
              dict(compression={"x": "ZSTD", "k": "SNAPPY"})),
    "nested": (pa.array([[i, i + 1] for i in range(30000)],
                        pa.list_(pa.int32())), {}),
    "type": (pa.array([decimal.Decimal(i) for i in range(30000)],
                      pa.decimal128(30, 2)), {}),
    "encoding": (pa.array(UNIQUE), dict(use_dictionary=False)),
    "encoding-overflow": (pa.array(UNIQUE),
                          dict(dictionary_pagesize_limit=8192)),
    "encoding-delta": (pa.array(range(30000), pa.int64()),
                       dict(use_dictionary=False,
                            column_encoding={"x": "DELTA_BINARY_PACKED",
                                             "k": "PLAIN"})),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallback(case, tmp_path, stats):
    x, options = FALLBACKS[case]
    path = tmp_path / "f.parquet"
    pq.write_table(pa.table({"x": x, "k": pa.array(range(30000), pa.int64())}),
                   path, row_group_size=10000, **options)
    check_file(path, stats, host_chunks=3)
    assert stats["reasons"] == [case.split("-")[0]] * 3
    assert stats["device_chunks"] == 3


# ---------------------------------------------------------------------------
# 5. the reader around it
# ---------------------------------------------------------------------------

@pytest.fixture
def three_groups(tmp_path):
    path = str(tmp_path / "r.parquet")
    pq.write_table(pa.table({"a": pa.array(range(300), pa.int64()),
                             "b": pa.array([i % 7 for i in range(300)],
                                           pa.int32()),
                             "c": pa.array([str(i % 5) for i in range(300)])}),
                   path, row_group_size=100)
    return path


QUERIES = {
    "projection": (lambda df: df.select("a", "c"), 2 * 3),
    "reordered": (lambda df: df.select("c", "a"), 2 * 3),
    "limit": (lambda df: df.limit(150), 3 * 2),
    "pruned": (lambda df: df.where(col("a") >= 250), 3 * 1),
}


@pytest.mark.parametrize("query", list(QUERIES))
def test_reader(query, three_groups, stats):
    run, chunks = QUERIES[query]
    want = run(daft.read_parquet(three_groups, device_decode=False)).to_pydict()
    assert stats["device_chunks"] == 0
    assert run(daft.read_parquet(three_groups)).to_pydict() == want
    assert stats["device_chunks"] == chunks and stats["host_chunks"] == 0


def test_row_group_subset(three_groups, stats):
    got = list(readers.read_file(three_groups, "parquet", ["b"], None, None,
                                 {}, {}, DEV, row_groups=[2, 0]))
    want = pq.ParquetFile(three_groups)
    assert [rb.to_pydict() for rb in got] == \
        [want.read_row_group(rg, columns=["b"]).to_pydict() for rg in (2, 0)]
    assert stats["device_chunks"] == 2


def test_empty_file(tmp_path, stats):
    path = str(tmp_path / "e.parquet")
    table = pa.table({"a": pa.array([], pa.int64()),
                      "s": pa.array([], pa.string())})
    pq.write_table(table, path)
    df = daft.read_parquet(path)
    assert df.to_pydict() == {"a": [], "s": []}
    host = daft.read_parquet(path, device_decode=False)
    assert [(f.name, f.dtype) for f in df.schema] == \
        [(f.name, f.dtype) for f in host.schema]

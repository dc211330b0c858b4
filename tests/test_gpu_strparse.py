"""The parse and format kernels (csrc/strparse.hip) and the casts, `to_date`,
`to_datetime` and `try_cast` built on them (daft_amd/kernels/parse.py),
against Python itself: `int`, `float`, `Decimal` quantized half-even,
`date.fromisoformat`, `strptime` and `str`.  Row counts sit around the
256-row block; columns are plain, null over bytes, sliced at a byte offset
that is no multiple of 16, or hold one 20 KB row so that its block leaves the
LDS tile.  All comparisons are exact, floats by their 8 bytes."""
import datetime as dtm
import decimal
import random
import re
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import DataType, Series, col
from daft_amd import functions as F
from daft_amd.kernels import native_required, parse

DEV = "cuda:0"
SIZES = [0, 1, 255, 256, 257, 4099]
VARIANTS = ["plain", "nulls", "sliced", "junk"]
INTS = {"int8": (-2**7, 2**7 - 1), "int16": (-2**15, 2**15 - 1),
        "int32": (-2**31, 2**31 - 1), "int64": (-2**63, 2**63 - 1),
        "uint8": (0, 2**8 - 1), "uint16": (0, 2**16 - 1),
        "uint32": (0, 2**32 - 1), "uint64": (0, 2**64 - 1)}
FMT = {"date": "%Y-%m-%d", "to_date": "%Y-%m-%d",
       "datetime": "%Y-%m-%d %H:%M:%S", "datetime_t": "%Y-%m-%dT%H:%M:%S"}
DEC_RE = r"[+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)"
# exact ties between two doubles with w > 2^53 (2^53 + 1, and 5^23 which has
# 54 bits): the truncated product cannot break a tie, so the host rounds them
TIES = {"9007199254740993", "1e23"}


def _dtype(t):
    if t in INTS or t in ("float32", "float64"):
        return getattr(DataType, t)()
    if t.startswith("dec"):
        return DataType.decimal128(18 if t == "dec18" else 12, int(t[-1]) if
                                   t != "dec18" else 2)
    return DataType.date() if t in ("date", "to_date") else \
        DataType.timestamp("us")


def _call(t, s):
    """The public call of target `t` on the column `s`."""
    if t == "to_date":
        e = col("s").str.to_date(FMT[t])
    elif t.startswith("datetime"):
        e = F.to_datetime(col("s"), FMT[t])
    else:
        return s.cast(_dtype(t))
    return e._node.fn(s, *e._node.literal_args, **e._node.kwargs)


def _oracle(t, v):
    """Python's value of the row `v`; raises what Python raises."""
    if v is None or (v == "" and t not in FMT):
        return None
    if t in INTS:
        if not INTS[t][0] <= int(v) <= INTS[t][1]:
            raise RuntimeError("out of range: what the storage type does")
        return int(v)
    if t.startswith("float"):
        x = torch.tensor(float(v), dtype=torch.float64)
        return x.item() if t == "float64" else x.to(torch.float32).item()
    if t.startswith("dec"):
        return decimal.Decimal(v).quantize(
            decimal.Decimal(1).scaleb(-_dtype(t).scale),
            rounding=decimal.ROUND_HALF_EVEN)
    if t == "date":
        return dtm.date.fromisoformat(v)
    d = dtm.datetime.strptime(v, FMT[t])
    return d.date() if t == "to_date" else d


def _native_row(t, v):
    """The row is one the kernel's grammar takes (else the host decides)."""
    if t in INTS:
        return bool(re.fullmatch(r"[+-]?[0-9]+", v, re.A)) and \
            INTS[t][0] <= int(v) <= min(INTS[t][1], 2**63 - 1)
    if t.startswith("float"):
        sig = re.sub(r"[eE].*|[+.-]", "", v).lstrip("0")
        x = float(v) if re.fullmatch(DEC_RE + "([eE][+-]?[0-9]+)?", v) \
            else float("nan")
        return len(sig) <= 19 and v not in TIES and \
            (not sig or 2.0**-1022 <= abs(x) < float("inf"))
    if t.startswith("dec"):
        if not re.fullmatch(DEC_RE, v):
            return False
        x = decimal.Decimal(v).scaleb(_dtype(t).scale)
        return x == int(x) and abs(x) < 10 ** _dtype(t).precision
    shape = r"\d{4}-\d\d-\d\d" + ("" if t in ("date", "to_date") else
                                  FMT[t][8] + r"\d\d:\d\d:\d\d")
    try:
        return bool(re.fullmatch(shape, v, re.A)) and bool(_oracle(t, v))
    except ValueError:
        return False


def _edges(t):
    """Edge rows of target `t`, good and bad together."""
    if t in INTS:
        lo, hi = INTS[t]
        return ["0", "-0", "+7", "007", str(lo), str(hi), str(lo - 1),
                str(hi + 1), "9223372036854775807", "9223372036854775808",
                "-9223372036854775808", "-9223372036854775809", "", " 1",
                "1_0", "١٢", "1.0", "-", "+"]
    if t.startswith("dec"):
        return ["1.50", "1.05", ".5", "5.", "-.5", "1e2", "", ".", "-0.0",
                "9999999999999999.99", "10000000000000000.00", "1.2.3"]
    if t.startswith("float"):
        return ["0", "-0.0", ".5", "5.", "1e22", "1e23", "9007199254740992",
                "9007199254740993", "9007199254740995", "0.30000000000000004",
                "1.7976931348623157e308", "1e309", "2.2250738585072014e-308",
                "5e-324", "12345678901234567890", "1234567890" * 4, "1e",
                "e5", ".", "inf", "nan", "1_0.5", "1e99999", ""]
    days = ["0001-01-01", "9999-12-31", "1970-01-01", "1969-12-31",
            "2000-02-29", "1900-02-29", "2024-02-30", "2024-13-01",
            "0000-01-01", "2024-1-5", "20240105", ""]
    times = [" 23:59:59", " 24:00:00", " 23:59:60", "T23:59:59", " 00:00:00"]
    return days + ["2024-01-05" + x for x in times] + \
        ["0001-01-01 00:00:00", "9999-12-31T23:59:59"]


def _good(t):
    out = []
    for v in _edges(t):
        try:
            _oracle(t, v)
            out.append(v)
        except (ValueError, RuntimeError, decimal.InvalidOperation):
            pass
    return out


def _canonical(t, rng):
    """A row the kernel must parse without the host."""
    if t in INTS:
        return str(rng.randint(max(INTS[t][0], -10**18 + 1),
                               min(INTS[t][1], 10**18 - 1)))
    if t.startswith("float"):
        return "%se%d" % (rng.randrange(10**15), rng.randint(-22, 22))
    if t.startswith("dec"):
        return "%d.%0*d" % (rng.randint(-10**9, 10**9), _dtype(t).scale,
                            rng.randrange(10 ** _dtype(t).scale))
    d = dtm.datetime(1, 1, 1) + dtm.timedelta(
        seconds=rng.randrange(3652059 * 86400))
    return d.strftime(FMT[t]).rjust(19 if "time" in t else 10, "0")


def _column(vals, variant, t="int64"):
    """(device column, the values its rows hold) for one variant."""
    vals = list(vals)
    valid = None
    if variant == "nulls":
        valid = [i % 3 != 1 for i in range(len(vals))]
    elif variant == "junk" and vals:
        mid = len(vals) // 2     # int, float and Decimal all strip blanks
        vals[mid] = " " * 20000 + (vals[mid] or "1")
        if t in FMT:
            valid = [i != mid for i in range(len(vals))]
    lead = ["xyz"] if variant == "sliced" else []
    s = Series.from_pylist("s", lead + vals, DataType.string(), device=DEV)
    s = Series("s", s.dtype, data=s.data, offsets=s.offsets[len(lead):],
               validity=None if valid is None else
               torch.tensor(valid, dtype=torch.bool, device=DEV))
    if valid is not None:
        vals = [v if ok else None for v, ok in zip(vals, valid)]
    return s, vals


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, float):
            assert g is not None and \
                struct.pack("<d", g) == struct.pack("<d", w), (i, g, w)
        else:
            assert g == w and type(g) is type(w), (i, g, w)


TARGETS = list(INTS) + ["float32", "float64", "dec1", "dec2", "dec18", "date",
                        "to_date", "datetime", "datetime_t"]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    native_required()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("t", ["int8", "int64", "uint32", "float64", "dec2",
                               "date", "datetime"])
def test_parse_matrix(t, n, variant):
    rng = random.Random(n)
    pool = _good(t) + [_canonical(t, rng) for _ in range(n)]
    s, vals = _column(pool[:n], variant, t)
    _same(_call(t, s).to_pylist(), [_oracle(t, v) for v in vals])


@pytest.mark.parametrize("t", TARGETS)
def test_edges_and_host_rows(t, monkeypatch):
    """Good edge rows equal Python; the host is called once, with exactly the
    rows outside the kernel's grammar."""
    rng = random.Random(1)
    vals = _good(t) + [_canonical(t, rng) for _ in range(40)]
    seen = []
    real = parse._host_parse
    monkeypatch.setattr(parse, "_host_parse", lambda s, *a:
                        seen.append(s.to_pylist()) or real(s, *a))
    _same(_call(t, _column(vals, "plain")[0]).to_pylist(),
          [_oracle(t, v) for v in vals])
    host = [v for v in vals if v and not _native_row(t, v)]
    assert seen == ([host] if host else [])


def _outcome(fn, s):
    try:
        return fn(s).to_pylist()
    except Exception as e:
        return type(e)


@pytest.mark.parametrize("t", TARGETS)
def test_bad_rows_match_cpu(t):
    """Rows Python rejects raise as on a CPU column and are null through
    try_cast; rows outside the type's range do what the storage type does."""
    ok = _good(t)[0]
    bad = [v for v in _edges(t) if v not in _good(t)]
    alone = []
    for v in bad:
        cpu = Series.from_pylist("s", [ok, v], DataType.string())
        alone.append(_outcome(lambda s: _call(t, s), cpu))
        assert _outcome(lambda s: _call(t, s),
                        _column([ok, v], "plain")[0]) == alone[-1]
    assert any(isinstance(a, type) for a in alone)
    if t not in FMT or t == "date":
        run = F.try_cast(col("s"), _dtype(t))._node.fn
        got = run(_column(bad + [ok], "plain")[0]).to_pylist()
        _same(got, run(Series.from_pylist("s", bad + [ok],
                                          DataType.string())).to_pylist())
        assert got[-1] == _oracle(t, ok) and all(
            g is None for g, a in zip(got, alone) if isinstance(a, type))


def _raise(*a, **k):
    raise AssertionError("host path taken")


@pytest.mark.parametrize("t", TARGETS)
def test_canonical_rows_stay_on_device(t, monkeypatch):
    monkeypatch.setattr(parse, "_host_parse", _raise)
    monkeypatch.setattr(parse, "_host_to_string", _raise)
    rng = random.Random(2)
    s, vals = _column([_canonical(t, rng) for _ in range(257)], "nulls")
    out = _call(t, s)
    _same(out.to_pylist(), [_oracle(t, v) for v in vals])
    if t in INTS and t != "uint64" or t in ("date", "to_date"):
        _same(out.cast(DataType.string()).to_pylist(),
              [None if v is None else str(_oracle(t, v)) for v in vals])


@pytest.mark.parametrize("kind", ["repr", "w_e_q"])
def test_float_corpus(kind, monkeypatch):
    """`repr` rows have at most 17 digits and reach the host only through an
    ambiguity exit of the Eisel-Lemire step: under 1 % of them."""
    rng = random.Random(3)
    vals = []
    while len(vals) < 4099:
        if kind == "repr":
            b = rng.getrandbits(64)
            if 0 < (b >> 52) & 0x7FF < 0x7FF:
                vals.append(repr(struct.unpack("<d", struct.pack("<Q", b))[0]))
        else:
            d = rng.randint(1, 19)
            vals.append("%de%d" % (rng.randrange(10**(d - 1), 10**d),
                                   rng.randint(-330, 310)))
    sent = []
    real = parse._host_parse
    monkeypatch.setattr(parse, "_host_parse",
                        lambda s, *a: sent.append(len(s)) or real(s, *a))
    out = _column(vals, "plain")[0].cast(DataType.float64())
    _same(out.to_pylist(), [float(v) for v in vals])
    if kind == "repr":
        assert sum(sent) < 0.01 * len(vals), sent


@pytest.mark.parametrize("t", [t for t in INTS if t != "uint64"] + ["date"])
def test_format(t, monkeypatch):
    monkeypatch.setattr(parse, "_host_to_string", _raise)
    if t == "date":
        vals = [dtm.date(1, 1, 1), None, dtm.date(9999, 12, 31), dtm.date(1970, 1, 1),
                dtm.date(1969, 12, 31), dtm.date(2000, 2, 29)]
    else:
        vals = [0, None, 7, -7 if INTS[t][0] else 9, *INTS[t], 10, 99, 100]
    s = Series.from_pylist("v", vals * 43, _dtype(t), device=DEV)
    _same(s.cast(DataType.string()).to_pylist(),
          [None if v is None else str(v) for v in vals * 43])
    assert s.slice(0, 0).cast(DataType.string()).to_pylist() == []


def test_format_date_out_of_range_takes_host(monkeypatch):
    seen = []
    real = parse._host_to_string
    monkeypatch.setattr(parse, "_host_to_string",
                        lambda s: seen.append(len(s)) or real(s))
    days = torch.tensor([0, parse._DAY_MAX + 1], dtype=torch.int32)
    with pytest.raises(OverflowError):
        Series("d", DataType.date(), data=days).cast(DataType.string())
    with pytest.raises(OverflowError):
        Series("d", DataType.date(), data=days.to(DEV)).cast(DataType.string())
    assert seen == [2, 2]


@pytest.mark.parametrize("n", [0, 1, 257])
def test_raw_outputs_and_refusals(n):
    nat = native_required()
    s, _ = _column((["7", "x", "", "1.25", "2024-01-05", "100"] * 50)[:n],
                   "nulls")
    c = (s.offsets, s.data, s.validity)
    p5 = parse.pow5_table(DEV)
    calls = {"str_parse_int": (lambda *c: nat.str_parse_int(*c, -9, 99),
                               torch.int64),
             "str_parse_decimal": (lambda *c: nat.str_parse_decimal(*c, 2, 99),
                                   torch.int64),
             "str_parse_float": (lambda *c: nat.str_parse_float(*c, p5),
                                 torch.float64),
             "str_parse_datetime": (lambda *c: nat.str_parse_datetime(*c, 0),
                                    torch.int32)}
    for name, (fn, dt) in calls.items():
        values, status = fn(*c)
        assert values.dtype == dt and status.dtype == torch.uint8
        assert values.shape == status.shape == (n,)
        assert values.device == status.device == s.data.device
        assert not values[status != 0].any()
        for args in [(c[0].cpu(), c[1], c[2]), (c[0][:0], c[1], c[2]),
                     (c[0].to(torch.int32), c[1], c[2]),
                     (c[0], c[1].to(torch.int8), c[2]),
                     (c[0], c[1], torch.ones(n + 1, dtype=torch.bool,
                                             device=DEV)),
                     (c[0], c[1], torch.ones(n, dtype=torch.uint8,
                                             device=DEV))]:
            with pytest.raises(RuntimeError, match=name):
                fn(*args)
        again = fn(*c)
        assert torch.equal(again[0], values) and torch.equal(again[1], status)
    i32 = torch.zeros(3, dtype=torch.int32)
    for name, call in [
            ("str_parse_int", lambda: nat.str_parse_int(*c, 1, 0)),
            ("str_parse_decimal", lambda: nat.str_parse_decimal(*c, 19, 9)),
            ("str_parse_decimal", lambda: nat.str_parse_decimal(*c, 2, 10**18)),
            ("str_parse_float", lambda: nat.str_parse_float(*c, p5[:650])),
            ("str_parse_datetime", lambda: nat.str_parse_datetime(*c, 47)),
            ("format_int", lambda: nat.format_int(i32.to(DEV), None)),
            ("format_date", lambda: nat.format_date(i32, None))]:
        with pytest.raises(RuntimeError, match=name):
            call()
    off, data = nat.format_int(torch.tensor([-10, 5], device=DEV), None)
    assert off.tolist() == [0, 3, 4] and bytes(data.tolist()) == b"-105"
    values, status = nat.str_parse_int(*c, -9, 99)
    want = [(7, 0), (0, 1), (0, 1), (0, 2), (0, 1), (0, 2)]   # rows 1, 4: null
    assert list(zip(values.tolist(), status.tolist())) == (want * 50)[:n]


def test_dataframe_and_sql_match_cpu():
    rng = random.Random(4)
    data = {k: [_canonical(t, rng) for _ in range(300)] + tail
            for k, t, tail in [("i", "int64", [None, ""]),
                               ("f", "float64", ["1e23", None]),
                               ("m", "dec2", ["1.005", None]),
                               ("d", "date", [None, None])]}
    out = {}
    for dev in ("cpu", DEV):
        t = daft.from_pydict(data, device=dev)
        i, d = col("i").cast(DataType.int64()), col("d").cast(DataType.date())
        q = t.select(i, col("f").cast(DataType.float64()),
                     col("m").cast(DataType.decimal128(12, 2)), d,
                     i.cast(DataType.string()).alias("i_s"),
                     d.cast(DataType.string()).alias("d_s"))
        out[dev] = (q.to_pydict(), daft.sql(
            "select cast(i as bigint) as i, cast(f as double) as f from t")
            .to_pydict())
    for got, want in zip(out[DEV], out["cpu"]):
        assert got.keys() == want.keys()
        for k in want:
            _same(got[k], want[k])
    _same(out[DEV][1]["i"], out[DEV][0]["i"])
    _same(out[DEV][0]["i_s"][:300], [str(int(v)) for v in data["i"][:300]])

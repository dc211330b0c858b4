"""Native as-of probe (csrc/asof.hip) against the brute-force oracle in
asof_cases.py, and the device path of asof_match / join_asof against the CPU
path.  Every comparison is exact index or value equality.

The probe launches min(2048, ceil(nl / 256)) blocks of 256 threads and
grid-strides, so 2048 * 256 + 1 left rows are the first size at which a
thread takes a second row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import Series
from daft_amd.kernels import native_required
from daft_amd.physical.asof import asof_match

import asof_cases as ac

DEV = "cuda:0"
CODE = {"backward": 0, "forward": 1, "nearest": 2}
BIG = 2048 * 256 + 1


@pytest.fixture(scope="module")
def native():
    return native_required()


def _dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _probe(native, inputs, strategy, allow_exact, float_keys):
    out = native.asof_probe(*inputs, CODE[strategy], allow_exact, float_keys)
    assert out.dtype == torch.int64 and out.device == inputs[0].device
    assert out.shape == inputs[0].shape
    return out


@pytest.mark.parametrize("case", ac.grid(), ids=ac.case_ids())
def test_probe_equals_oracle(native, case):
    inputs = _dev(*ac.probe_inputs(case))
    for strategy, allow_exact in ac.VARIANTS:
        got = _probe(native, inputs, strategy, allow_exact, case.is_float)
        assert tuple(got.tolist()) == ac.expected(case, strategy,
                                                  allow_exact), \
            (strategy, allow_exact)


@pytest.mark.parametrize("i", range(len(ac.HAND)))
def test_match_hand_cases(i):
    lk, lg, rk, rg, strategy, allow_exact, want = ac.HAND[i]
    dt = "float64" if isinstance(lk[0], float) else "int64"
    got = asof_match(
        ac.key_series("t", dt, lk, [True] * len(lk), DEV),
        ac.key_series("t", dt, rk, [True] * len(rk), DEV),
        [ac.gid_series("g", lg, DEV)], [ac.gid_series("g", rg, DEV)],
        strategy, allow_exact)
    assert got.is_cuda and got.tolist() == want


def test_probe_grid_stride(native):
    # the 257-row left side tiled to one row more than a full grid covers in
    # one pass: the expected output is the small case's answer tiled
    case = ac.big_case()
    lk, lg, rk, rows, seg = ac.probe_inputs(case)
    reps = -(-BIG // len(lk))
    inputs = _dev(np.tile(lk, reps)[:BIG], np.tile(lg, reps)[:BIG], rk, rows,
                  seg)
    for strategy, allow_exact in ac.VARIANTS:
        small = np.array(ac.expected(case, strategy, allow_exact))
        want = torch.from_numpy(np.tile(small, reps)[:BIG]).to(DEV)
        got = _probe(native, inputs, strategy, allow_exact, False)
        assert torch.equal(got, want), (strategy, allow_exact)


@pytest.mark.parametrize("case", ac.grid(), ids=ac.case_ids())
def test_match_device_equals_cpu(case):
    host = ac.case_series(case)
    dev = ac.case_series(case, DEV)
    for strategy, allow_exact in ac.VARIANTS:
        want = asof_match(*host, strategy, allow_exact)
        got = asof_match(*dev, strategy, allow_exact)
        assert got.is_cuda and got.dtype == torch.int64
        assert torch.equal(got.cpu(), want), (strategy, allow_exact)


def test_match_string_by_device_equals_cpu():
    case = ac._make("string-by", 77, 65, 64, 7, "heavy_dups")
    sym = lambda gs: Series.from_pylist(
        "a", [None if g is None else f"sym-{g:03d}" for g in gs])
    lk, rk, lb, rb = ac.case_series(case)
    host = (lk, rk, [sym(case.left_gid)] + lb, [sym(case.right_gid)] + rb)
    dev = tuple([s.to(DEV) for s in x] if isinstance(x, list) else x.to(DEV)
                for x in host)
    for strategy, allow_exact in ac.VARIANTS:
        want = ac.expected(case, strategy, allow_exact)
        assert tuple(asof_match(*host, strategy, allow_exact).tolist()) == want
        assert tuple(asof_match(*dev, strategy, allow_exact).tolist()) == want


def test_strided_keys(native):
    case = ac._make("strided", 31, 257, 65, 2, nulls=False)
    lk, rk, lb, rb = ac.case_series(case, DEV)
    wide = torch.stack([lk.data, lk.data + 1], dim=1)       # [nl, 2]
    strided = Series("t", lk.dtype, data=wide[:, 0])
    assert not strided.data.is_contiguous()
    for strategy, allow_exact in ac.VARIANTS:
        want = asof_match(lk, rk, lb, rb, strategy, allow_exact)
        got = asof_match(strided, rk, lb, rb, strategy, allow_exact)
        assert torch.equal(got, want)
    # the raw entry point refuses what the wrapper repairs
    inputs = _dev(*ac.probe_inputs(case))
    wide = torch.stack([inputs[0], inputs[0]], dim=1)
    with pytest.raises(RuntimeError, match="left_keys"):
        native.asof_probe(wide[:, 0], *inputs[1:], 0, True, False)


def test_argument_errors(native):
    case = ac._make("errors", 32, 65, 64, 2, nulls=False)
    lk, lg, rk, rows, seg = _dev(*ac.probe_inputs(case))
    ok = dict(lk=lk, lg=lg, rk=rk, rows=rows, seg=seg, strategy=0,
              allow_exact=True)

    def call(**kw):
        a = dict(ok, **kw)
        return native.asof_probe(a["lk"], a["lg"], a["rk"], a["rows"],
                                 a["seg"], a["strategy"], a["allow_exact"],
                                 False)
    assert call().shape == lk.shape
    bad = [
        dict(lk=lk.to(torch.int32)),
        dict(rk=rk.to(torch.float64)),
        dict(seg=seg.to(torch.int32)),
        dict(lk=lk.cpu()),
        dict(lg=lg.cpu()),
        dict(rows=rows.cpu()),
        dict(lg=lg[:-1]),
        dict(rows=rows[:-1]),
        dict(lk=lk.reshape(1, -1), lg=lg.reshape(1, -1)),
        dict(strategy=3),
        dict(strategy=-1),
        dict(strategy=2, allow_exact=False),
        dict(seg=seg[:0]),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError, match="asof_probe"):
            call(**kw)
    # nothing to do: an empty int64 tensor on the device
    out = native.asof_probe(lk[:0], lg[:0], rk, rows, seg, 0, True, False)
    assert out.shape == (0,) and out.dtype == torch.int64 and out.is_cuda


def _doc_frames(device):
    left = daft.from_pydict({"entity": ["A", "A", "B"],
                             "timestamp": [10, 11, 10]}, device=device)
    right = daft.from_pydict({"entity": ["A", "A", "A", "B", "B"],
                              "timestamp": [9, 10, 11, 9, 11],
                              "value": [1.0, 2.0, 3.0, 5.0, 6.0]},
                             device=device)
    return left, right


@pytest.mark.parametrize("strategy", ac.STRATEGIES)
def test_join_asof_docstring_example(strategy):
    outs = []
    for device in ("cpu", DEV):
        left, right = _doc_frames(device)
        outs.append(left.join_asof(right, on="timestamp", by="entity",
                                   strategy=strategy)
                    .sort(["entity", "timestamp"]).to_pydict())
    assert outs[0] == outs[1]
    if strategy == "backward":
        assert outs[1]["value"] == [2.0, 3.0, 5.0]


@pytest.mark.parametrize("strategy", ac.STRATEGIES)
def test_join_asof_seeded_1000(strategy):
    n = 1000
    syms = [f"s{i}" for i in range(20)]

    def frame(device, with_v):
        r = np.random.default_rng(12 + with_v)
        d = {"sym": [syms[i] for i in r.integers(0, 20, n)],
             "t": [int(v) for v in r.integers(0, 5000, n)]}
        if with_v:
            d["v"] = [float(v) for v in r.random(n)]
        return daft.from_pydict(d, device=device)
    outs = []
    for device in ("cpu", DEV):
        out = frame(device, 0).join_asof(frame(device, 1), on="t", by="sym",
                                         strategy=strategy).to_pydict()
        outs.append(out)
    assert outs[0] == outs[1]
    assert len(outs[1]["v"]) == n
    assert any(v is not None for v in outs[1]["v"])

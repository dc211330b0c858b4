"""Out-of-core (grace) hash join on the device: build sides over
`memory_limit_bytes` are partitioned with the native partitioner
(csrc/partition.hip) and must return the rows of the in-memory join as a
multiset.  The CPU tier of the same logic is tests/test_grace_join.py."""
import functools
import random

import pyarrow as pa
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import daft_amd as daft
from daft_amd import execution_config_ctx
from daft_amd.kernels import native_required, rowops
from daft_amd.physical import ops
from tests.conftest import assert_df_eq

DEV = "cuda:0"
HOWS = ("inner", "left", "right", "outer", "semi", "anti")
N_BUILD, N_PROBE, BATCH = 20_000, 50_000, 8192
LIMIT = 64 << 10


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    native_required()


@pytest.fixture
def spy(monkeypatch):
    """Records every rowops.hash_partition call as (is_cuda, P, remix) and
    every JoinOp that executes."""
    class Spy:
        calls = []
        joins = []
    orig = rowops.hash_partition

    def hash_partition(hashes, num_partitions, remix=False):
        Spy.calls.append((hashes.is_cuda, num_partitions, remix))
        return orig(hashes, num_partitions, remix)
    monkeypatch.setattr(rowops, "hash_partition", hash_partition)
    orig_exec = ops.JoinOp.execute

    def execute(self, ectx):
        Spy.joins.append(self)
        return orig_exec(self, ectx)
    monkeypatch.setattr(ops.JoinOp, "execute", execute)
    Spy.calls, Spy.joins = [], []
    return Spy


def _ints(rng, n, lo, hi, null_rate=0.0):
    return [None if rng.random() < null_rate else rng.randrange(lo, hi)
            for _ in range(n)]


def _strs(ints):
    return [None if v is None else f"key_{v}" for v in ints]


@functools.lru_cache(maxsize=None)
def _data(name):
    """(probe columns, build columns, dictionary columns per side); about
    2.5 build rows per key, so matches fan out."""
    rng = random.Random(name)
    nulls = 0.1 if name in ("int64", "string") else 0.0
    lo = -4000 if name == "int32_vs_int64" else 0
    lk = _ints(rng, N_PROBE, lo, lo + 12_000, nulls)
    rk = _ints(rng, N_BUILD, lo, lo + 8_000, nulls)
    if name in ("string", "dict_vs_plain"):
        lk, rk = _strs(lk), _strs(rk)
    left = {"k": lk, "pv": list(range(N_PROBE))}
    right = {"k": rk, "bv": list(range(N_BUILD))}
    return left, right, (("k",) if name == "dict_vs_plain" else ())


def _frame(data, device, dict_cols=(), int32=False):
    if dict_cols:
        t = pa.table({k: (pa.array(v).dictionary_encode() if k in dict_cols
                          else pa.array(v)) for k, v in data.items()})
        df = daft.from_arrow(t, device=device)
    else:
        df = daft.from_pydict(data, device=device)
    if int32:
        df = df.with_column("k", daft.col("k").cast(daft.DataType.int32()))
    return df.into_batches(BATCH)


def _frames(name, device=DEV):
    left, right, ldict = _data(name)
    return (_frame(left, device, ldict, int32=name == "int32_vs_int64"),
            _frame(right, device))


def _grace(L, R, how, spy, on_device=True):
    spy.calls.clear()
    spy.joins.clear()
    with execution_config_ctx(memory_limit_bytes=LIMIT,
                              enable_gpu=on_device):
        got = L.join(R, on="k", how=how).to_pydict()
    assert len(spy.joins) == 1
    stats = spy.joins[0].grace_stats
    assert stats is not None and stats["partitions"] >= 2
    nb = stats["partitions"]
    # on the device the native partitioner ran: device hashes, one radix
    # digit, remixed
    assert nb <= 256 and spy.calls
    assert all(c == (on_device, nb, True) for c in spy.calls), spy.calls[:3]
    return got


def _check(name, how, spy):
    L, R = _frames(name)
    want = L.join(R, on="k", how=how).to_pydict()
    assert spy.calls == [] and [j.grace_stats for j in spy.joins] == [None]
    got = _grace(L, R, how, spy)
    assert_df_eq(got, want, sort_by=list(want.keys()))
    return got


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", ("int64", "string"))
def test_grace_join_equals_in_memory_join(name, how, spy):
    _check(name, how, spy)


@pytest.mark.parametrize("name", ("int32_vs_int64", "dict_vs_plain"))
def test_grace_inner_join_mixed_key_types(name, spy):
    got = _check(name, "inner", spy)
    assert len(got["k"]) > N_PROBE


def test_grace_join_on_device_equals_cpu_tier(spy):
    got = _grace(*_frames("int64"), "outer", spy)
    want = _grace(*_frames("int64", device="cpu"), "outer", spy,
                  on_device=False)
    assert_df_eq(got, want, sort_by=list(want.keys()))

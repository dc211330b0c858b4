"""Aux subsystem tests: subscribers/events, checkpoint store, IO round trips,
UDFs, config (ref pattern: tests/test_subscribers.py, tests/io/)."""
import os

import pytest

import daft_amd as daft
from daft_amd import DataType, col
from daft_amd.context import Subscriber, get_context


class _Capture(Subscriber):
    def __init__(self):
        self.events = []

    def on_query_start(self, query_id, explain):
        self.events.append(("start", query_id))

    def on_query_end(self, query_id, seconds, error):
        self.events.append(("end", query_id, error))

    def on_operator_end(self, query_id, node_id, name, rows_in, rows_out,
                        seconds):
        self.events.append(("op", name, rows_out))


def test_subscriber_events():
    sub = _Capture()
    daft.attach_subscriber(sub)
    try:
        daft.from_pydict({"a": [1, 2, 3]}).where(col("a") > 1).collect()
    finally:
        daft.detach_subscriber(sub)
    kinds = [e[0] for e in sub.events]
    assert "start" in kinds and "end" in kinds and "op" in kinds
    op_events = {e[1]: e[2] for e in sub.events if e[0] == "op"}
    assert op_events.get("Filter") == 2


def test_event_log_subscriber(tmp_path):
    from daft_amd.subscribers import EventLogSubscriber
    sub = EventLogSubscriber(str(tmp_path))
    daft.attach_subscriber(sub)
    try:
        daft.from_pydict({"a": [1]}).collect()
    finally:
        daft.detach_subscriber(sub)
    import json
    lines = [json.loads(l) for l in open(sub.path)]
    assert any(l["event"] == "query_end" for l in lines)


def test_checkpoint_roundtrip(tmp_path):
    from daft_amd.checkpoint import CheckpointConfig, LocalCheckpointStore
    store = LocalCheckpointStore(str(tmp_path / "ck"))
    cfg = CheckpointConfig(store, on="id")
    df1 = daft.from_pydict({"id": [1, 2, 3], "v": [10, 20, 30]})
    out1 = cfg.filter_processed(df1)
    assert out1.count_rows() == 3
    cfg.commit(out1)
    df2 = daft.from_pydict({"id": [2, 3, 4, 5], "v": [0, 0, 40, 50]})
    out2 = cfg.filter_processed(df2)
    assert sorted(out2.to_pydict()["id"]) == [4, 5]


def test_parquet_roundtrip(tmp_path):
    df = daft.from_pydict({
        "a": [1, 2, 3], "b": ["x", None, "z"], "c": [1.5, 2.5, None],
    })
    df.write_parquet(str(tmp_path / "out"))
    back = daft.read_parquet(str(tmp_path / "out") + "/*.parquet") \
        .sort("a").to_pydict()
    assert back == {"a": [1, 2, 3], "b": ["x", None, "z"],
                    "c": [1.5, 2.5, None]}


def test_parquet_pushdown(tmp_path):
    daft.from_pydict({"a": list(range(100)), "b": list(range(100))}) \
        .write_parquet(str(tmp_path / "p"))
    df = daft.read_parquet(str(tmp_path / "p") + "/*.parquet")
    out = df.select("a").where(col("a") < 5).to_pydict()
    assert out == {"a": [0, 1, 2, 3, 4]}
    # limit pushdown
    assert daft.read_parquet(str(tmp_path / "p") + "/*.parquet") \
        .limit(3).count_rows() == 3


def test_csv_roundtrip(tmp_path):
    df = daft.from_pydict({"a": [1, 2], "s": ["x", "y"]})
    df.write_csv(str(tmp_path / "c"))
    back = daft.read_csv(str(tmp_path / "c") + "/*.csv").sort("a").to_pydict()
    assert back["a"] == [1, 2] and back["s"] == ["x", "y"]


def test_json_write(tmp_path):
    df = daft.from_pydict({"a": [1, 2]})
    paths = df.write_json(str(tmp_path / "j")).to_pydict()["path"]
    import json
    rows = [json.loads(l) for l in open(paths[0])]
    assert rows == [{"a": 1}, {"a": 2}]


def test_partitioned_write(tmp_path):
    df = daft.from_pydict({"g": ["a", "a", "b"], "v": [1, 2, 3]})
    paths = df.write_parquet(str(tmp_path / "pw"),
                             partition_cols=[col("g")]).to_pydict()["path"]
    assert any("g=a" in p for p in paths)
    assert any("g=b" in p for p in paths)


def test_udf_row_wise():
    @daft.func
    def add1(x: int) -> int:
        return x + 1

    df = daft.from_pydict({"a": [1, 2, 3]})
    assert df.select(add1(col("a"))).to_pydict()["add1"] == [2, 3, 4]


def test_udf_batched():
    @daft.func(return_dtype=DataType.float64(), batched=True)
    def double(s):
        import torch
        from daft_amd.series import Series
        return Series("d", DataType.float64(), data=s.data * 2.0,
                      validity=s.validity)

    df = daft.from_pydict({"a": [1.0, 2.0]})
    assert df.select(double(col("a"))).to_pydict()["double"] == [2.0, 4.0]


def test_udf_retry_and_null():
    calls = {"n": 0}

    @daft.func(return_dtype=DataType.int64(), max_retries=2)
    def flaky(x: int) -> int:
        calls["n"] += 1
        if calls["n"] < 3:
            raise RuntimeError("boom")
        return x

    df = daft.from_pydict({"a": [7]})
    assert df.select(flaky(col("a"))).to_pydict()["flaky"] == [7]

    @daft.func(return_dtype=DataType.int64(), on_error="null")
    def broken(x: int) -> int:
        raise RuntimeError("always")

    out = df.select(broken(col("a"))).to_pydict()["broken"]
    assert out == [None]


def test_stateful_cls_udf():
    @daft.cls
    class Scaler:
        def __init__(self, k):
            self.k = k

        @daft.method(return_dtype=DataType.int64())
        def scale(self, x):
            return x * self.k

    sc = Scaler(10)
    df = daft.from_pydict({"a": [1, 2]})
    assert df.select(sc.scale(col("a"))).to_pydict()["scale"] == [10, 20]


def test_execution_config_ctx():
    from daft_amd import execution_config_ctx
    ctx = get_context()
    before = ctx.execution_config.morsel_size_rows
    with execution_config_ctx(morsel_size_rows=123):
        assert ctx.execution_config.morsel_size_rows == 123
    assert ctx.execution_config.morsel_size_rows == before


def test_cli_schema(tmp_path, capsys):
    daft.from_pydict({"a": [1]}).write_parquet(str(tmp_path / "t"))
    from daft_amd.cli import main
    import glob
    path = glob.glob(str(tmp_path / "t") + "/*.parquet")[0]
    main(["schema", path])
    out = capsys.readouterr().out
    assert "a" in out


def test_window_functions():
    from daft_amd.functions import dense_rank, rank, row_number
    from daft_amd.window import Window
    df = daft.from_pydict({"g": ["a", "a", "a", "b"],
                           "v": [3.0, 1.0, 3.0, 5.0]})
    w = Window().partition_by("g").order_by("v")
    out = df.with_window_columns({
        "rn": row_number().over(w),
        "rk": rank().over(w),
        "dr": dense_rank().over(w),
        "sv": col("v").sum().over(w),
    }).sort(["g", "v", "rn"]).to_pydict()
    assert out["rn"] == [1, 2, 3, 1]
    assert out["rk"] == [1, 2, 2, 1]
    assert out["dr"] == [1, 2, 2, 1]
    # SQL RANGE-default: sum over (partition, order) is a RUNNING sum with
    # peer sharing
    assert out["sv"] == [1.0, 7.0, 7.0, 5.0]


def test_lag_lead():
    df = daft.from_pydict({"g": ["a", "a", "a"], "v": [1, 2, 3]})
    from daft_amd.window import Window
    w = Window().partition_by("g").order_by("v")
    out = df.with_window_columns({
        "prev": col("v").lag(1).over(w),
        "next": col("v").lead(1).over(w),
    }).sort("v").to_pydict()
    assert out["prev"] == [None, 1, 2]
    assert out["next"] == [2, 3, None]


def test_explain(capsys):
    df = daft.from_pydict({"a": [1]}).where(col("a") > 0).select(col("a"))
    df.explain(show_all=True)
    out = capsys.readouterr().out
    assert "Filter" in out and "Optimized" in out


def test_udf_use_process():
    @daft.func(return_dtype=DataType.int64(), use_process=True)
    def triple(x: int) -> int:
        import os
        return x * 3

    df = daft.from_pydict({"a": [1, 2, 3]})
    assert df.select(triple(col("a"))).to_pydict()["triple"] == [3, 6, 9]


def test_pivot_and_unpivot_roundtrip():
    df = daft.from_pydict({"id": [1, 2], "x": [10, 20], "y": [30, 40]})
    long = df.unpivot(["id"])
    wide = long.pivot("id", col("variable"), col("value"), "sum",
                      names=["x", "y"]).sort("id").to_pydict()
    assert wide == {"id": [1, 2], "x": [10, 20], "y": [30, 40]}


def test_from_arrow_dictionary_roundtrip():
    import pyarrow as pa
    arr = pa.array(["a", "b", "a", None]).dictionary_encode()
    t = pa.table({"d": arr})
    df = daft.from_arrow(t)
    assert df.to_pydict() == {"d": ["a", "b", "a", None]}
    back = df.collect()._result[0].column("d")
    assert back.is_dict()
    out = df.to_arrow()
    assert pa.types.is_dictionary(out.column("d").type)


def test_dashboard_api():
    from daft_amd import dashboard
    from fastapi.testclient import TestClient
    state = dashboard.DashboardState()
    sub = dashboard.DashboardSubscriber(state)
    daft.attach_subscriber(sub)
    try:
        daft.from_pydict({"a": [1, 2]}).where(col("a") > 1).collect()
    finally:
        daft.detach_subscriber(sub)
    client = TestClient(dashboard.make_app(state))
    qs = client.get("/api/queries").json()
    assert len(qs) == 1 and qs[0]["status"] == "done"
    detail = client.get(f"/api/queries/{qs[0]['id']}").json()
    assert any(op["name"] == "Filter" for op in detail["operators"])
    html = client.get("/").text
    assert "daft_amd" in html and "api/queries" in html


def test_partition_cache_spill_bookkeeping():
    from daft_amd import execution_config_ctx
    from daft_amd.context import PartitionCache
    ctx = get_context()
    # a cache of its own, filled by host execution: the context's cache
    # holds whatever earlier tests left, device-resident partitions included
    saved, ctx.cache = ctx.cache, PartitionCache()
    try:
        cache = ctx.cache
        with execution_config_ctx(enable_gpu=False):
            df1 = daft.from_pydict({"a": list(range(1000))}).collect()
            df2 = daft.from_pydict({"b": list(range(1000))}).collect()
        assert cache.total_bytes() > 0
        # nothing on a cuda device here: spill_lru reports nothing to free
        assert cache.spill_lru("cuda:0") == 0
        # host residents are the spill TARGET, never a spill source
        assert cache.spill_lru("cpu") == 0
    finally:
        ctx.cache = saved


def test_memory_limit_admission():
    from daft_amd.execution.memory import MemoryManager
    from daft_amd import execution_config_ctx
    ctx = get_context()
    with execution_config_ctx(memory_limit_bytes=1):
        mm = MemoryManager(ctx)
        # admission with an impossible limit spills what it can, then
        # proceeds (best-effort, no deadlock)
        mm.admit(10_000, "cpu")
    out = daft.from_pydict({"a": [1, 2]}).where(col("a") > 0).to_pydict()
    assert out == {"a": [1, 2]}


def test_running_window_aggs():
    df = daft.from_pydict({"g": ["a"] * 4 + ["b"] * 2,
                           "t": [1, 2, 3, 4, 1, 2],
                           "v": [10.0, 20.0, 30.0, 40.0, 5.0, 7.0]})
    from daft_amd.window import Window
    w = Window().partition_by("g").order_by("t")
    out = df.with_window_columns({
        "rs": col("v").sum().over(w),
        "rc": col("v").count().over(w),
        "rm": col("v").mean().over(w),
    }).sort(["g", "t"]).to_pydict()
    assert out["rs"] == [10.0, 30.0, 60.0, 100.0, 5.0, 12.0]
    assert out["rc"] == [1, 2, 3, 4, 1, 2]
    assert out["rm"] == [10.0, 15.0, 20.0, 25.0, 5.0, 6.0]


def test_running_window_ties_share_frame():
    df = daft.from_pydict({"t": [1, 1, 2], "v": [10.0, 20.0, 5.0]})
    from daft_amd.window import Window
    w = Window().order_by("t")
    out = df.with_window_columns({"rs": col("v").sum().over(w)}) \
        .sort(["t", "v"]).to_pydict()
    # t=1 rows are peers: both see the full 30.0
    assert out["rs"] == [30.0, 30.0, 35.0]


def test_whole_partition_agg_without_order():
    df = daft.from_pydict({"g": ["a", "a", "b"], "v": [1.0, 2.0, 5.0]})
    from daft_amd.window import Window
    w = Window().partition_by("g")
    out = df.with_window_columns({"s": col("v").sum().over(w)}) \
        .sort(["g", "v"]).to_pydict()
    assert out["s"] == [3.0, 3.0, 5.0]


def test_rows_between_frames():
    df = daft.from_pydict({"g": ["a"] * 5, "t": [1, 2, 3, 4, 5],
                           "v": [1.0, 2.0, 3.0, 4.0, 5.0]})
    from daft_amd.window import Window
    W = Window
    w = Window().partition_by("g").order_by("t").rows_between(-1, 1)
    out = df.with_window_columns({"s": col("v").sum().over(w)}) \
        .sort("t").to_pydict()
    assert out["s"] == [3.0, 6.0, 9.0, 12.0, 9.0]
    w2 = Window().partition_by("g").order_by("t") \
        .rows_between(W.unbounded_preceding, W.current_row)
    out2 = df.with_window_columns({"s": col("v").sum().over(w2)}) \
        .sort("t").to_pydict()
    assert out2["s"] == [1.0, 3.0, 6.0, 10.0, 15.0]
    w3 = Window().partition_by("g").order_by("t").rows_between(-1, -1)
    out3 = df.with_window_columns({"m": col("v").mean().over(w3)}) \
        .sort("t").to_pydict()
    assert out3["m"] == [None, 1.0, 2.0, 3.0, 4.0]


def test_ddsketch_accuracy_and_merge():
    """physical/sketch.py: relative error within alpha; merge = exact
    concatenation semantics (DDSketch property)."""
    import numpy as np
    import torch
    from daft_amd.physical import sketch
    from daft_amd.series import Series
    from daft_amd.schema import DataType

    rng = np.random.default_rng(3)
    vals = np.concatenate([
        rng.lognormal(3, 2, 20000),          # positives over decades
        -rng.lognormal(1, 1, 5000),          # negatives
        np.zeros(100),
    ])
    rng.shuffle(vals)
    s = Series("x", DataType.float64(), data=torch.from_numpy(vals))
    gids = torch.zeros(len(vals), dtype=torch.int64)
    sk = sketch.grouped_sketch(s, gids, 1, "sk")

    for q in (0.01, 0.25, 0.5, 0.9, 0.99):
        got = float(sketch.grouped_sketch_final(
            sk, torch.zeros(1, dtype=torch.int64), 1, q, "p").data[0])
        want = float(np.quantile(vals, q))
        denom = max(abs(want), 1e-9)
        assert abs(got - want) / denom < 3 * sketch.ALPHA, (q, got, want)

    # split in two, sketch each half, merge: same buckets as one pass
    half = len(vals) // 2
    s1 = Series("x", DataType.float64(), data=torch.from_numpy(vals[:half]))
    s2 = Series("x", DataType.float64(), data=torch.from_numpy(vals[half:]))
    sk1 = sketch.grouped_sketch(s1, torch.zeros(half, dtype=torch.int64),
                                1, "sk")
    sk2 = sketch.grouped_sketch(
        s2, torch.zeros(len(vals) - half, dtype=torch.int64), 1, "sk")
    merged = sk1.children[0].data + sk2.children[0].data
    assert torch.equal(merged, sk.children[0].data)


def test_shard_and_torch_iter_dataset(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import daft_amd as daft
    paths = []
    for i in range(5):
        p = str(tmp_path / f"f{i}.parquet")
        pq.write_table(pa.table({"a": [i * 10 + j for j in range(3)]}), p)
        paths.append(p)
    df = daft.read_parquet(paths)
    s0 = df._shard("file", 2, 0).to_pydict()["a"]
    s1 = df._shard("file", 2, 1).to_pydict()["a"]
    assert sorted(s0 + s1) == sorted(df.to_pydict()["a"])
    assert not set(s0) & set(s1)
    rows = list(df.to_torch_iter_dataset(shard_strategy="file",
                                         world_size=2, rank=0))
    assert [r["a"] for r in rows] == s0
    with pytest.raises(ValueError):
        df._shard("row", 2, 0)
    with pytest.raises(ValueError):
        daft.from_pydict({"a": [1]})._shard("file", 2, 0)


def test_read_warc(tmp_path):
    import gzip
    import json
    import daft_amd as daft
    from daft_amd import col

    def rec(rid, rtype, uri, date, payload, extra=None):
        h = [b"WARC/1.0",
             f"WARC-Record-ID: <urn:uuid:{rid}>".encode(),
             f"WARC-Type: {rtype}".encode()]
        if uri:
            h.append(f"WARC-Target-URI: {uri}".encode())
        h.append(f"WARC-Date: {date}".encode())
        h.append(f"Content-Length: {len(payload)}".encode())
        if extra:
            h.extend(f"{k}: {v}".encode() for k, v in extra.items())
        return b"\r\n".join(h) + b"\r\n\r\n" + payload + b"\r\n\r\n"

    blob = (rec("aaa-111", "response", "http://x.com/",
                "2024-01-02T03:04:05Z", b"<html>hi</html>",
                {"Content-Type": "application/http"}) +
            rec("bbb-222", "request", None, "2024-01-02T03:04:06Z",
                b"GET /"))
    p1 = str(tmp_path / "a.warc")
    open(p1, "wb").write(blob)
    p2 = str(tmp_path / "b.warc.gz")
    open(p2, "wb").write(gzip.compress(blob))

    out = daft.read_warc(p1).to_pydict()
    assert out["WARC-Record-ID"] == ["aaa-111", "bbb-222"]
    assert out["warc_content"] == [b"<html>hi</html>", b"GET /"]
    assert out["WARC-Target-URI"] == ["http://x.com/", None]
    assert json.loads(out["warc_headers"][0])["Content-Type"] == \
        "application/http"
    assert daft.read_warc(p2).to_pydict()["WARC-Record-ID"] == \
        out["WARC-Record-ID"]
    assert daft.read_warc([p1, p2]) \
        .where(col("WARC-Type") == "response").count_rows() == 2
    fp = daft.read_warc([p1, p2], file_path_column="src").to_pydict()["src"]
    assert fp == [p1, p1, p2, p2]


def test_datasets_common_crawl_local_mirror(tmp_path):
    import gzip as _gz
    import daft_amd as daft
    crawl = "CC-MAIN-2025-33"
    seg_dir = tmp_path / "crawl-data" / crawl / "segments" / "123" / "warc"
    seg_dir.mkdir(parents=True)
    rec = (b"WARC/1.0\r\nWARC-Record-ID: <urn:uuid:x-1>\r\n"
           b"WARC-Type: response\r\nWARC-Date: 2025-01-01T00:00:00Z\r\n"
           b"Content-Length: 2\r\n\r\nhi\r\n\r\n")
    rel = f"crawl-data/{crawl}/segments/123/warc/part-0.warc"
    (tmp_path / rel).write_bytes(rec)
    man = tmp_path / "crawl-data" / crawl / "warc.paths.gz"
    man.write_bytes(_gz.compress((rel + "\n").encode()))
    df = daft.datasets.common_crawl(crawl, data_root=str(tmp_path))
    out = df.to_pydict()
    assert out["warc_content"] == [b"hi"]
    with pytest.raises(FileNotFoundError):
        daft.datasets.common_crawl(crawl, segment="999",
                                   data_root=str(tmp_path))


def test_datasets_lerobot(tmp_path):
    import json
    import pyarrow as pa
    import pyarrow.parquet as pq
    import daft_amd as daft
    (tmp_path / "meta").mkdir()
    (tmp_path / "meta" / "info.json").write_text(json.dumps({
        "data_path": "data/chunk-{episode_chunk:03d}/"
                     "episode_{episode_index:06d}.parquet"}))
    d = tmp_path / "data" / "chunk-000"
    d.mkdir(parents=True)
    for e in range(3):
        pq.write_table(pa.table({"obs": [e * 1.0, e + 0.5],
                                 "episode_index": [e, e]}),
                       str(d / f"episode_{e:06d}.parquet"))
    df = daft.datasets.lerobot.load(str(tmp_path))
    assert df.count_rows() == 6
    df2 = daft.datasets.lerobot.load(str(tmp_path), episodes=[1])
    assert df2.to_pydict()["episode_index"] == [1, 1]


def test_udf_actor_pool_concurrency():
    @daft.func(return_dtype=DataType.int64(), use_process=True,
               max_concurrency=2)
    def whoami(x: int) -> int:
        import os
        return os.getpid()

    df = daft.from_pydict({"x": list(range(64))})
    pids = set(df.select(whoami(col("x")).alias("p")).to_pydict()["p"])
    assert len(pids) == 2, pids
    import os
    assert os.getpid() not in pids


def test_native_extension_plugin(tmp_path):
    """daft_amd/ext: build the example plugin with g++, load it, call its
    functions through expressions."""
    import subprocess
    import daft_amd as daft
    repo = os.path.dirname(os.path.dirname(os.path.abspath(daft.__file__)))
    src = os.path.join(repo, "examples", "ext_plugin", "example_plugin.cpp")
    so = str(tmp_path / "example_plugin.so")
    subprocess.run(
        ["g++", "-O2", "-shared", "-fPIC",
         "-I" + os.path.join(repo, "daft_amd", "ext"), src, "-o", so],
        check=True, capture_output=True)
    names = daft.load_extension(so)
    assert set(names) >= {"ext_add1", "ext_hypot"}
    # the example plugin's functions are host-only
    with daft.execution_config_ctx(enable_gpu=False):
        df = daft.from_pydict({"a": [1, 2, None], "x": [3.0, 5.0, 8.0],
                               "y": [4.0, 12.0, 15.0]})
        out = df.select(
            daft.ext_function("ext_add1", col("a")).alias("a1"),
            daft.ext_function("ext_hypot", col("x"), col("y")).alias("h"),
        ).to_pydict()
    assert out["a1"] == [2, 3, None]
    assert out["h"] == [5.0, 13.0, 17.0]


def test_udaf():
    from daft_amd import udaf
    from daft_amd.series import Series as S

    @udaf(return_dtype=DataType.float64())
    class GeoMean:
        def aggregate(self, values):
            import math
            vals = [v for v in values.to_pylist() if v is not None]
            return (sum(math.log(v) for v in vals), len(vals))

        def combine(self, states):
            s = c = 0
            for a, b in states:
                s += a
                c += b
            return (s, c)

        def finalize(self, state):
            import math
            s, c = state
            return math.exp(s / c) if c else None

    df = daft.from_pydict({"g": ["a", "a", "b", "b", "b"],
                           "v": [2.0, 8.0, 1.0, 1.0, 27.0]})
    out = df.groupby("g").agg(GeoMean()(col("v")).alias("gm")) \
        .sort("g").to_pydict()
    assert out["gm"][0] == pytest.approx(4.0)
    assert out["gm"][1] == pytest.approx(3.0)
    # ungrouped
    tot = df.agg(GeoMean()(col("v")).alias("gm")).to_pydict()["gm"][0]
    import math
    assert tot == pytest.approx(math.exp(sum(map(math.log,
                                                 [2, 8, 1, 1, 27])) / 5))


def test_great_circle_distance():
    from daft_amd.functions import great_circle_distance
    df = daft.from_pydict({"lat1": [48.8566, 91.0], "lon1": [2.3522, 0.0],
                           "lat2": [51.5074, 0.0], "lon2": [-0.1278, 0.0]})
    out = df.select(great_circle_distance(
        col("lat1"), col("lon1"), col("lat2"), col("lon2")).alias("d")) \
        .to_pydict()["d"]
    assert abs(out[0] - 343_556) < 2000
    assert out[1] is None  # invalid latitude


def test_file_type(tmp_path):
    from daft_amd import File
    from daft_amd.functions import file, file_size
    p = tmp_path / "x.png"
    p.write_bytes(b"\x89PNG\r\n\x1a\n" + b"0" * 100)
    f = File(str(p))
    assert f.size() == 108 and f.exists() and f.is_image()
    assert f.mime_type() == "image/png"
    with f.open() as h:
        assert h.read(4) == b"\x89PNG"
    m = File(b"abcdef")
    assert m.size() == 6 and m.read() == b"abcdef"
    with m.to_tempfile() as tf:
        assert open(tf.name, "rb").read() == b"abcdef"

    df = daft.from_pydict({"p": [str(p), None]})
    out = df.select(file_size(file(col("p"))).alias("sz")).to_pydict()["sz"]
    assert out == [108, None]


def test_parquet_rowgroup_stats_pruning(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import daft_amd as daft
    from daft_amd.io import readers
    p = str(tmp_path / "t.parquet")
    # 4 row groups of 100 rows, a increasing
    pq.write_table(pa.table({"a": list(range(400)),
                             "b": [i * 2.0 for i in range(400)]}),
                   p, row_group_size=100)
    df = daft.read_parquet(p).where(col("a") >= 350)
    out = df.to_pydict()
    assert out["a"] == list(range(350, 400))
    # verify groups actually skipped
    from daft_amd.expressions.expressions import BinaryOp, ColumnRef, Literal
    pred = BinaryOp("ge", ColumnRef("a"), Literal(350))
    batches = list(readers._read_parquet(p, None, None, "cpu", pred))
    assert sum(len(b) for b in batches) == 100  # only the last group read


def test_compressed_csv_json(tmp_path):
    import gzip
    import daft_amd as daft
    pc = str(tmp_path / "t.csv.gz")
    with gzip.open(pc, "wt") as f:
        f.write("a,b\n1,x\n2,y\n")
    out = daft.read_csv(pc).to_pydict()
    assert out == {"a": [1, 2], "b": ["x", "y"]}
    pj = str(tmp_path / "t.jsonl.gz")
    with gzip.open(pj, "wt") as f:
        f.write('{"a": 1}\n{"a": 5}\n')
    assert daft.read_json(pj).to_pydict() == {"a": [1, 5]}


def test_window_first_last_value():
    from daft_amd.functions import w_first_value, w_last_value
    from daft_amd.window import Window
    df = daft.from_pydict({"g": ["a", "a", "a", "b", "b"],
                           "v": [3, 1, 2, 9, 8]})
    w = Window().partition_by("g").order_by("v")
    out = df.with_window_columns(
        {"f": w_first_value(col("v")).over(w),
         "l": w_last_value(col("v")).over(w)}).sort(["g", "v"]).to_pydict()
    assert out["f"] == [1, 1, 1, 8, 8]
    assert out["l"] == [1, 2, 3, 8, 9]


def test_session_sql_ddl():
    from daft_amd.catalog import Session
    s = Session()
    s.create_temp_table("t", daft.from_pydict({"a": [1, 2, 3]}))
    s.sql("create temp table big as select a * 10 as b from t where a > 1")
    out = s.sql("select sum(b) as s from big").to_pydict()
    assert out["s"] == [50]
    tables = s.sql("show tables").to_pydict()["table"]
    assert "big" in tables and "t" in tables
    with pytest.raises(ValueError):
        s.sql("create table big as select * from t")
    s.sql("create or replace table big as select a from t")
    assert s.sql("select count(*) as c from big").to_pydict()["c"] == [3]
    s.sql("drop table big")
    assert "big" not in s.sql("show tables").to_pydict()["table"]
    with pytest.raises(KeyError):
        s.sql("drop table nope")
    s.sql("drop table if exists nope")


def test_read_sql_and_blob(tmp_path):
    import sqlite3
    import daft_amd as daft
    db = str(tmp_path / "t.db")
    c = sqlite3.connect(db)
    c.execute("create table t (a int, b text)")
    c.executemany("insert into t values (?, ?)", [(1, "x"), (2, "y")])
    c.commit()
    df = daft.read_sql("select * from t order by a",
                       lambda: sqlite3.connect(db))
    assert df.to_pydict() == {"a": [1, 2], "b": ["x", "y"]}
    (tmp_path / "f1.bin").write_bytes(b"abc")
    g = daft.from_glob_path(str(tmp_path / "*.bin")).to_pydict()
    assert g["size"] == [3]
    b = daft.read_blob(str(tmp_path / "*.bin")).to_pydict()
    assert b["data"] == [b"abc"]
    with pytest.raises(RuntimeError):
        daft.read_deltalake("x")


def test_session_api_top_level():
    """Top-level daft.* session/catalog/utility surface (129/129 export
    parity with the reference's daft/__init__.py)."""
    import daft_amd as d
    df = d.range(5)
    assert df.to_pydict()["id"] == [0, 1, 2, 3, 4]
    d.create_temp_table("t_api", df)
    assert d.has_table("t_api") and "t_api" in d.list_tables()
    d.write_table("t_api", d.range(3))
    assert d.read_table("t_api").count_rows() == 8
    d.drop_table("t_api")
    assert not d.has_table("t_api")
    assert d.concat([d.range(2), d.range(2)]).count_rows() == 4
    assert str(d.TimeUnit.ns()) == "ns"
    with d.planning_config_ctx(morsel_size_rows=7):
        from daft_amd.context import get_context
        assert get_context().execution_config.morsel_size_rows == 7
    with pytest.raises(RuntimeError):
        d.set_runner_ray()


def test_running_min_max_over_order():
    # MIN/MAX with ORDER BY must be RUNNING min/max,
    # not whole-partition
    df = daft.from_pydict({"g": ["a"] * 4 + ["b"] * 2,
                           "t": [1, 2, 3, 4, 1, 2],
                           "v": [30.0, 10.0, 20.0, 5.0, 7.0, 3.0]})
    from daft_amd.window import Window
    w = Window().partition_by("g").order_by("t")
    out = df.with_window_columns({
        "rmin": col("v").min().over(w),
        "rmax": col("v").max().over(w),
    }).sort(["g", "t"]).to_pydict()
    assert out["rmin"] == [30.0, 10.0, 10.0, 5.0, 7.0, 3.0]
    assert out["rmax"] == [30.0, 30.0, 30.0, 30.0, 7.0, 7.0]


def test_running_min_max_int_and_frames():
    df = daft.from_pydict({"t": [1, 2, 3, 4, 5],
                           "v": [5, 1, 4, 2, 3]})
    from daft_amd.window import Window
    w = Window().order_by("t").rows_between(-1, 1)
    out = df.with_window_columns({
        "fmin": col("v").min().over(w),
        "fmax": col("v").max().over(w),
    }).sort("t").to_pydict()
    assert out["fmin"] == [1, 1, 1, 2, 2]
    assert out["fmax"] == [5, 5, 4, 4, 3]


def test_running_stddev_variance():
    import statistics
    df = daft.from_pydict({"t": [1, 2, 3], "v": [1.0, 3.0, 5.0]})
    from daft_amd.window import Window
    w = Window().order_by("t")
    out = df.with_window_columns({
        "rv": col("v").var().over(w) if hasattr(col("v"), "var")
        else col("v").stddev().over(w),
    }).sort("t").to_pydict() if False else None
    out = df.with_window_columns({
        "rs": col("v").stddev().over(w),
    }).sort("t").to_pydict()
    # population stddev of prefixes: [1], [1,3], [1,3,5]
    assert abs(out["rs"][0] - 0.0) < 1e-9
    assert abs(out["rs"][1] - 1.0) < 1e-9
    assert abs(out["rs"][2] - statistics.pstdev([1.0, 3.0, 5.0])) < 1e-9


def test_rank_with_null_order_keys():
    # a null key after a non-null row is NOT a peer
    from daft_amd.functions import rank
    from daft_amd.window import Window
    df = daft.from_pydict({"t": [1, None, None, 2]})
    w = Window().order_by("t")  # nulls last by default
    out = df.with_window_columns({"rk": rank().over(w)}).to_pydict()
    by_t = {}
    rows = sorted(zip(out["t"], out["rk"]),
                  key=lambda r: (r[0] is None, r[0] if r[0] is not None else 0))
    # t=1 -> rank 1, t=2 -> rank 2, nulls are peers of each other -> rank 3
    vals = [r[1] for r in rows]
    assert vals == [1, 2, 3, 3]


def test_lag_default_keeps_genuine_nulls():
    # default fills only out-of-partition offsets
    df = daft.from_pydict({"t": [1, 2, 3], "v": [10, None, 30]})
    from daft_amd.window import Window
    w = Window().order_by("t")
    out = df.with_window_columns({
        "prev": col("v").lag(1, default=-1).over(w),
    }).sort("t").to_pydict()
    # row t=3's lag is the genuinely-NULL v at t=2: stays NULL
    assert out["prev"] == [-1, 10, None]


def test_intersect_precedence():
    # INTERSECT binds tighter than UNION
    import daft_amd as daft2
    a = daft.from_pydict({"x": [1, 2]})
    b = daft.from_pydict({"x": [2, 3]})
    c = daft.from_pydict({"x": [3, 4]})
    from daft_amd.session_api import Session
    s = Session()
    s.create_temp_table("a", a)
    s.create_temp_table("b", b)
    s.create_temp_table("c", c)
    out = s.sql("SELECT x FROM a UNION (SELECT x FROM b INTERSECT SELECT x FROM c)") \
        .to_pydict()
    expected = sorted([1, 2, 3])
    out2 = s.sql("SELECT x FROM a UNION SELECT x FROM b INTERSECT SELECT x FROM c") \
        .to_pydict()
    # A UNION (B ∩ C) = {1,2} ∪ {3} = {1,2,3}; the flat-left-assoc reading
    # (A ∪ B) ∩ C would give {3}
    assert sorted(out2["x"]) == expected


def test_literal_repr_includes_dtype():
    from daft_amd.expressions.expressions import Literal
    a = repr(Literal(30, DataType.int32()))
    b = repr(Literal(30, DataType.int64()))
    assert a != b


def test_external_sort_spills_and_orders():
    """Sort larger than the memory budget range-partitions to host
    buckets and emits ordered batches (out-of-core sort path)."""
    import random
    random.seed(5)
    n = 50_000
    vals = [random.randint(-10**6, 10**6) for _ in range(n)]
    tag = [random.choice("abc") for _ in range(n)]
    df = daft.from_pydict({"v": vals, "t": tag}).into_batches(4096)
    from daft_amd.context import get_context
    cfg = get_context().execution_config
    old = cfg.memory_limit_bytes
    cfg.memory_limit_bytes = 64 * 1024   # force the spill path
    try:
        out = df.sort("v").to_pydict()
    finally:
        cfg.memory_limit_bytes = old
    assert out["v"] == sorted(vals)
    # rows stay aligned with their payload (multiset compare: ties keep
    # stable input order, not tag order)
    assert sorted(zip(out["v"], out["t"])) == sorted(zip(vals, tag))


def test_external_sort_multikey_desc_nulls():
    import random
    random.seed(6)
    n = 20_000
    a = [random.randint(0, 50) if i % 17 else None for i in range(n)]
    b = [random.random() for _ in range(n)]
    df = daft.from_pydict({"a": a, "b": b}).into_batches(1024)
    from daft_amd.context import get_context
    cfg = get_context().execution_config
    old = cfg.memory_limit_bytes
    cfg.memory_limit_bytes = 32 * 1024
    try:
        out = df.sort(["a", "b"], desc=[True, False]).to_pydict()
    finally:
        cfg.memory_limit_bytes = old
    # oracle: the engine's own in-memory sort (spilled path must agree)
    want = daft.from_pydict({"a": a, "b": b}) \
        .sort(["a", "b"], desc=[True, False]).to_pydict()
    assert out["a"] == want["a"]
    assert out["b"] == want["b"]


def test_topn_bounded_fold():
    import random
    random.seed(7)
    vals = [random.random() for _ in range(100_000)]
    df = daft.from_pydict({"v": vals}).into_batches(2048)
    out = df.sort("v", desc=True).limit(25).to_pydict()
    assert out["v"] == sorted(vals, reverse=True)[:25]


def test_batched_udf_subprocess():
    """@daft.func(batched=True, use_process=True): whole Series cross the
    process boundary through torch.multiprocessing (shared memory on CPU,
    CUDA/dmabuf IPC on GPU — see test_gpu.py for the device variant)."""
    import os as _os
    parent_pid = _os.getpid()

    @daft.func(return_dtype=DataType.float64(), batched=True,
               use_process=True)
    def scaled(x):
        import os
        import torch as _t
        assert os.getpid() != 0
        return _t.as_tensor(x.data, dtype=_t.float64) * 2.5

    df = daft.from_pydict({"x": [1.0, 2.0, 3.0, 4.0]})
    out = df.select(scaled(col("x")).alias("y")).to_pydict()
    assert out["y"] == [2.5, 5.0, 7.5, 10.0]


def test_batched_udf_subprocess_isolation():
    """A crash-prone batched UDF in a subprocess doesn't take the engine
    down; on_error surfaces as an error."""
    @daft.func(return_dtype=DataType.int64(), batched=True,
               use_process=True)
    def boom(x):
        raise ValueError("kaboom")

    df = daft.from_pydict({"x": [1, 2]})
    import pytest as _pt
    with _pt.raises(Exception, match="kaboom"):
        df.select(boom(col("x"))).to_pydict()


def test_scan_task_split_and_merge(tmp_path):
    """daft-scan parity: a big parquet file splits into row-group tasks
    and small files merge into one task (96-384 MB defaults scaled down
    for the test)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    big = tmp_path / "big.parquet"
    tbl = pa.table({"x": list(range(100_000)),
                    "s": [f"val{i}" for i in range(100_000)]})
    pq.write_table(tbl, big, row_group_size=10_000)
    for i in range(3):
        small = tmp_path / f"small{i}.parquet"
        pq.write_table(pa.table({"x": [i], "s": ["a"]}), small)
    from daft_amd.io.readers import plan_scan_tasks
    paths = sorted(str(p) for p in tmp_path.glob("*.parquet"))
    tasks = plan_scan_tasks(paths, "parquet", None,
                            min_bytes=100_000, max_bytes=300_000)
    # the big file must be split into multiple row-group tasks
    split = [t for t in tasks if t[1] is not None]
    assert len(split) >= 2
    covered = sorted(i for _p, rgs in split for i in rgs)
    assert covered == list(range(10))         # all 10 row groups, once
    # the three small files must be merged into one whole-file task
    merged = [t for t in tasks if t[1] is None]
    assert any(len(t[0]) == 3 for t in merged)
    # reading through the engine still yields every row exactly once
    out = daft.read_parquet(paths).to_pydict()
    assert sorted(out["x"]) == sorted(list(range(100_000)) + [0, 1, 2])


def test_hive_partitioned_read(tmp_path):
    """read_parquet parses key=value directories into typed partition
    columns (ref: daft-scan src/hive.rs), round-tripping the engine's own
    hive-partitioned writer."""
    import os
    df = daft.from_pydict({"year": [2023, 2023, 2024, 2024],
                           "region": ["us", "eu", "us", "eu"],
                           "v": [1.0, 2.0, 3.0, 4.0]})
    root = str(tmp_path / "t")
    df.write_parquet(root, partition_cols=["year", "region"])
    back = daft.read_parquet(root + "/**/*.parquet") \
        .sort(["year", "region"]).to_pydict()
    assert back["year"] == [2023, 2023, 2024, 2024]
    assert back["region"] == ["eu", "us", "eu", "us"]
    assert sorted(back["v"]) == [1.0, 2.0, 3.0, 4.0]
    # filters on partition columns work
    from daft_amd import col as _c
    f = daft.read_parquet(root + "/**/*.parquet") \
        .where((_c("year") == 2024) & (_c("region") == "us")).to_pydict()
    assert f["v"] == [3.0]


def test_otlp_file_span_exporter(tmp_path):
    """Spans export as OTLP/JSON resourceSpans at query end (ref:
    common/tracing OTLP wiring, flushed at run.rs:404)."""
    import json
    from daft_amd.context import get_context
    from daft_amd.subscribers.otlp import OTLPFileSpanExporter
    path = str(tmp_path / "spans.jsonl")
    sub = OTLPFileSpanExporter(path)
    ctx = get_context()
    ctx.attach_subscriber(sub) if hasattr(ctx, "attach_subscriber") else \
        ctx.subscribers.append(sub)
    try:
        df = daft.from_pydict({"x": [1, 2, 3]})
        df.where(col("x") > 1).select((col("x") * 2).alias("y")).to_pydict()
    finally:
        ctx.subscribers.remove(sub)
    lines = open(path).read().strip().splitlines()
    assert lines
    doc = json.loads(lines[-1])
    spans = doc["resourceSpans"][0]["scopeSpans"][0]["spans"]
    names = [s["name"] for s in spans]
    assert "query" in names and "optimize" in names
    assert any("Filter" in n for n in names)
    root = next(s for s in spans if s["name"] == "query")
    assert all(s.get("parentSpanId") == root["spanId"]
               for s in spans if s is not root)
    assert root["status"]["code"] == 1


def test_ipc_write_read_roundtrip(tmp_path):
    """Arrow IPC writer/reader (ref: daft-writers src/ipc.rs)."""
    df = daft.from_pydict({"k": [1, 2, 3], "s": ["a", None, "c"],
                           "f": [1.5, 2.5, 3.5]})
    root = str(tmp_path / "ipc")
    df.write_ipc(root)
    import os
    assert any(f.endswith(".arrow") for f in os.listdir(root))
    back = daft.read_ipc(root + "/*.arrow").sort("k").to_pydict()
    assert back["k"] == [1, 2, 3]
    assert back["s"] == ["a", None, "c"]
    assert back["f"] == [1.5, 2.5, 3.5]


def test_dashboard_ui_and_api():
    from fastapi.testclient import TestClient
    from daft_amd.dashboard import DashboardState, DashboardSubscriber, \
        make_app
    st = DashboardState()
    sub = DashboardSubscriber(st)
    from daft_amd.context import get_context
    ctx = get_context()
    ctx.subscribers.append(sub)
    try:
        daft.from_pydict({"x": [1, 2, 3]}).where(col("x") > 1).to_pydict()
    finally:
        ctx.subscribers.remove(sub)
    app = make_app(st)
    c = TestClient(app)
    qs = c.get("/api/queries").json()
    assert qs and qs[0]["status"] == "done"
    qid = qs[0]["id"]
    rec = c.get(f"/api/queries/{qid}").json()
    assert rec["operators"], "per-operator stats missing"
    html = c.get("/").text
    assert "daft_amd" in html and "/api/queries" in html


def test_segmented_multi_agg_matches_scatter():
    """Sorted-gids segmented aggregation (q21/q18 clustered keys) equals
    the scatter reference for sum/min/max/count with nulls."""
    import torch
    from daft_amd.physical.agg import _segmented_multi_agg
    torch.manual_seed(3)
    n, G = 100_000, 20_000
    gids = torch.sort(torch.randint(0, G, (n,), dtype=torch.int64)).values
    # ensure every group appears (dense ids contract)
    gids[:G] = torch.arange(G)
    gids = torch.sort(gids).values
    d1 = torch.rand(n, dtype=torch.float64)
    v1 = torch.rand(n) > 0.2
    d2 = torch.rand(n, dtype=torch.float64) * 100
    datas = [d1, d2, d2, torch.empty(0, dtype=torch.float64)]
    valids = [v1, None, v1, None]
    ops = [0, 1, 2, 3]     # sum, min, max, count
    out, cnt = _segmented_multi_agg(gids, G, datas, valids, ops, n,
                                    torch.device("cpu"))
    out = out.view(4, G)
    cnt = cnt.view(4, G)
    ref_sum = torch.zeros(G, dtype=torch.float64).scatter_add_(
        0, gids, torch.where(v1, d1, torch.zeros_like(d1)))
    assert torch.allclose(out[0], ref_sum)
    ref_min = torch.full((G,), float("inf"), dtype=torch.float64) \
        .scatter_reduce_(0, gids, d2, reduce="amin")
    assert torch.allclose(out[1], ref_min)
    ref_max = torch.full((G,), float("-inf"), dtype=torch.float64) \
        .scatter_reduce_(0, gids, torch.where(
            v1, d2, torch.full_like(d2, float("-inf"))), reduce="amax")
    assert torch.allclose(out[2], ref_max)
    ref_cnt = torch.zeros(G, dtype=torch.int64).scatter_add_(
        0, gids, torch.ones(n, dtype=torch.int64))
    assert torch.equal(cnt[3], ref_cnt)
    # per-agg valid counts
    ref_cv = torch.zeros(G, dtype=torch.int64).scatter_add_(
        0, gids, v1.to(torch.int64))
    assert torch.equal(cnt[0], ref_cv)


def test_segmented_reduce_matches_numpy():
    """The shared segmented helper against a numpy scatter reference at
    far more groups than rows, and its valid-row count past 2^24 rows in
    one group (exact in float64, not in float32)."""
    import numpy as np
    import torch
    from daft_amd.kernels import AGG_COUNT, AGG_MAX, AGG_MIN, AGG_SUM
    from daft_amd.kernels.rowops import segment_bounds, segmented_reduce
    rng = np.random.default_rng(9)
    n, G = 5000, 70_000
    g = np.sort(rng.integers(0, G, n))
    d = rng.integers(-(1 << 20), 1 << 20, n) / 1024.0   # exact sums
    v = rng.random(n) > 0.2
    tg, td, tv = torch.from_numpy(g), torch.from_numpy(d), torch.from_numpy(v)
    for valid in (None, v):
        keep = np.ones(n, bool) if valid is None else valid
        want_cnt = np.zeros(G, np.int64)
        np.add.at(want_cnt, g[keep], 1)
        ref = {AGG_SUM: (np.add, 0.0), AGG_MIN: (np.minimum, np.inf),
               AGG_MAX: (np.maximum, -np.inf)}
        for op, (ufunc, ident) in ref.items():
            want = np.full(G, ident)
            ufunc.at(want, g[keep], d[keep])
            out, cnt = segmented_reduce(tg, G, td,
                                        None if valid is None else tv, op)
            assert np.array_equal(out.numpy(), want), op
            assert cnt.dtype == torch.int64
            assert np.array_equal(cnt.numpy(), want_cnt), op
        out, cnt = segmented_reduce(tg, G, None,
                                    None if valid is None else tv, AGG_COUNT)
        assert np.array_equal(cnt.numpy(), want_cnt) and not out.any()
    assert np.array_equal(segment_bounds(tg, G)[2].numpy(),
                          np.bincount(g, minlength=G))
    # one group of 2^24 + 3 valid rows, fed as a lengths tensor
    big = (1 << 24) + 3
    _, cnt = segmented_reduce(torch.zeros(big, dtype=torch.int64), 1, None,
                              torch.ones(big, dtype=torch.bool), AGG_COUNT,
                              lengths=torch.tensor([big]))
    assert cnt.tolist() == [big]


def test_round2_edge_cases():
    """Empty inputs through the round-2 surfaces: new optimizer rules,
    external sort, jq, Map, is_in table path, scan tasks, framed windows."""
    from daft_amd.schema import DataType as DT
    from daft_amd.series import Series as S
    e = daft.from_pydict({"k": [], "v": []})
    big = daft.from_pydict({"k2": [1, 2], "w": [1.0, 2.0]})
    out = e.join(big, left_on="k", right_on="k2", how="left") \
        .groupby("v").agg(col("w").sum().alias("s")).to_pydict()
    assert out["s"] == []
    from daft_amd.context import get_context
    cfg = get_context().execution_config
    old = cfg.memory_limit_bytes
    cfg.memory_limit_bytes = 1024
    try:
        assert e.sort("k").to_pydict()["k"] == []
    finally:
        cfg.memory_limit_bytes = old
    from daft_amd.functions import jq
    assert daft.from_pydict({"j": []}) \
        .select(jq(col("j"), ".a")).to_pydict() is not None
    dt = DT.map(DT.string(), DT.int64())
    assert S.from_pylist("m", [], dt).to_pylist() == []
    s2 = S.from_pylist("x", [1, 2, 3], DT.int64())
    assert s2.is_in(S.from_pylist("v", [], DT.int64())).to_pylist() == \
        [False] * 3
    from daft_amd.io.readers import plan_scan_tasks
    assert plan_scan_tasks([], "parquet", None) == []
    one = daft.from_pydict({"t": [1], "v": [2.0]})
    from daft_amd.window import Window
    w = Window().order_by("t")
    assert one.with_window_columns(
        {"m": col("v").min().over(w)}).to_pydict()["m"] == [2.0]


def test_custom_data_source_and_sink():
    """Python connector APIs: DataSource tasks -> DataFrame, DataSink
    start/write/finalize via write_sink (ref: daft/io/{source,sink}.py)."""
    import daft_amd as daft
    from daft_amd import col
    from daft_amd.io import (DataSink, DataSource, DataSourceTask,
                             Pushdowns, WriteResult, read_source)
    from daft_amd.recordbatch import RecordBatch
    from daft_amd.schema import DataType, Field, Schema
    from daft_amd.series import Series

    sch = Schema([Field("x", DataType.int64())])

    class RangeTask(DataSourceTask):
        def __init__(self, lo, hi):
            self.lo, self.hi = lo, hi

        @property
        def schema(self):
            return sch

        def read(self):
            yield RecordBatch(
                [Series.from_pylist("x", list(range(self.lo, self.hi)),
                                    DataType.int64())],
                num_rows=self.hi - self.lo)

    class RangeSource(DataSource):
        @property
        def name(self):
            return "range"

        @property
        def schema(self):
            return sch

        def get_tasks(self, pushdowns=None):
            assert pushdowns is None or isinstance(pushdowns, Pushdowns)
            yield RangeTask(0, 5)
            yield RangeTask(5, 8)

    df = read_source(RangeSource())
    assert df.to_pydict() == {"x": list(range(8))}
    assert df.where(col("x") >= 6).count_rows() == 2

    class CollectSink(DataSink):
        def __init__(self):
            self.rows = []
            self.started = False

        def start(self):
            self.started = True

        def write(self, batch):
            got = batch.to_pydict()["x"]
            self.rows.extend(got)
            return WriteResult(result=len(got), rows_written=len(got))

        def finalize(self, results):
            return {"writes": len(results),
                    "rows": sum(r.rows_written for r in results)}

    sink = CollectSink()
    out = df.write_sink(sink)
    assert sink.started and sorted(sink.rows) == list(range(8))

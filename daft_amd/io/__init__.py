"""IO layer: in-memory ingestion + file readers/writers (ref capability:
/root/reference/src/daft-io, daft-parquet, daft-csv, daft-json, daft-scan,
daft-writers and daft/io/*.py)."""
from __future__ import annotations

import glob as _glob
import os
from typing import Dict, List, Optional, Union

from ..context import get_context
from ..dataframe import DataFrame
from ..logical.builder import LogicalPlanBuilder
from ..recordbatch import RecordBatch
from ..schema import DataType, Field, Schema


def _default_device(device=None):
    if device is not None:
        return device
    return get_context().default_device_str()


def from_pydict(data: Dict[str, list], device=None) -> DataFrame:
    ctx = get_context()
    rb = RecordBatch.from_pydict(data, device=_default_device(device))
    key = ctx.cache.new_key()
    ctx.cache.put(key, [rb])
    return DataFrame(LogicalPlanBuilder.from_in_memory(
        rb.schema, key, len(rb), rb.size_bytes()))


def from_recordbatches(batches: List[RecordBatch],
                       partitioning=None) -> DataFrame:
    """`partitioning=(token, [key_cols])` declares rank-colocation of equal
    keys under a named distribution (skips distributed exchanges)."""
    ctx = get_context()
    key = ctx.cache.new_key()
    ctx.cache.put(key, batches)
    rows = sum(len(b) for b in batches)
    size = sum(b.size_bytes() for b in batches)
    return DataFrame(LogicalPlanBuilder.from_in_memory(
        batches[0].schema, key, rows, size, partitioning))


def from_arrow(table, device=None) -> DataFrame:
    import pyarrow as pa
    if isinstance(table, (pa.RecordBatch,)):
        table = pa.Table.from_batches([table])
    rb = RecordBatch.from_arrow(table, device=_default_device(device))
    return from_recordbatches([rb])


def from_pandas(df, device=None) -> DataFrame:
    import pyarrow as pa
    return from_arrow(pa.Table.from_pandas(df), device=device)


def _expand_paths(path: Union[str, List[str]],
                  io_config=None) -> List[str]:
    from .object_store import get_source, glob_paths, is_remote
    paths = [path] if isinstance(path, str) else list(path)
    out: List[str] = []
    for p in paths:
        if is_remote(p):
            if any(ch in p for ch in "*?["):
                out.extend(glob_paths(p, io_config))
            elif p.endswith("/"):
                out.extend(sorted(
                    f for f, _sz in
                    get_source(p, io_config).list_prefix(p)))
            else:
                out.append(p)
            continue
        if any(ch in p for ch in "*?["):
            matches = sorted(_glob.glob(p, recursive=True))
            out.extend(matches)
        elif os.path.isdir(p):
            for root, _dirs, files in os.walk(p):
                for f in sorted(files):
                    if not f.startswith((".", "_")):
                        out.append(os.path.join(root, f))
        else:
            out.append(p)
    if not out:
        raise FileNotFoundError(f"no files match {path}")
    return out


def _parse_hive_partitions(paths: List[str]):
    """key=value path segments common to every file (ref: daft-scan
    src/hive.rs).  Returns (per-path {col: str value}, ordered keys) or
    (None, None) when the layout is not hive-partitioned."""
    import urllib.parse
    per = []
    keysets = []
    for p in paths:
        comps = p.replace("\\", "/").split("/")[:-1]
        d = {}
        order = []
        for c in comps:
            if "=" in c and not c.startswith("="):
                k, _, v = c.partition("=")
                if k and k not in d:
                    d[k] = urllib.parse.unquote(v)
                    order.append(k)
        per.append(d)
        keysets.append(tuple(order))
    if not per or not keysets[0] or any(ks != keysets[0]
                                        for ks in keysets):
        return None, None
    return per, list(keysets[0])


def _hive_typed(values: List[str]):
    try:
        return [int(v) for v in values], DataType.int64()
    except ValueError:
        pass
    try:
        return [float(v) for v in values], DataType.float64()
    except ValueError:
        return values, DataType.string()


def read_parquet(path, columns: Optional[List[str]] = None,
                 io_config=None, hive_partitioning: bool = True,
                 device_decode: Optional[bool] = None,
                 **kwargs) -> DataFrame:
    """`device_decode`: None or True decode local files on the execution
    device when it is a GPU (kernels/parquet.py); False, a CPU device, and
    remote inputs are decoded by pyarrow on the host."""
    from . import readers
    paths = _expand_paths(path, io_config)
    schema = readers.infer_schema(paths[0], "parquet",
                                  storage_options=io_config)
    read_options = {"device_decode": device_decode}
    if hive_partitioning:
        per, keys = _parse_hive_partitions(paths)
        if keys:
            keys = [k for k in keys if k not in set(schema.names())]
        if keys:
            from ..schema import Field
            hive_fields = []
            hive_parts = {}
            for k in keys:
                vals, dt = _hive_typed([d[k] for d in per])
                hive_fields.append(Field(k, dt))
                for pth, v in zip(paths, vals):
                    hive_parts.setdefault(pth, {})[k] = v
            schema = Schema(schema.fields() + hive_fields)                 if hasattr(schema, "fields") else schema
            read_options.update(hive_parts=hive_parts,
                                hive_fields=[(f.name, f.dtype)
                                             for f in hive_fields])
    b = LogicalPlanBuilder.from_scan(schema, paths, "parquet",
                                     storage_options=io_config,
                                     read_options=read_options)
    df = DataFrame(b)
    if columns:
        df = df.select(*columns)
    return df


def read_warc(path, io_config=None, file_path_column: Optional[str] = None,
              **kwargs) -> DataFrame:
    """Read WARC / gzipped-WARC web-archive files (capability of the
    reference's daft.read_warc, /root/reference/daft/io/_warc.py:24:
    fixed schema of mandatory WARC headers, raw record content, and the
    remaining headers as a JSON string column)."""
    from . import readers
    paths = _expand_paths(path)
    b = LogicalPlanBuilder.from_scan(readers.warc_schema(), paths, "warc",
                                     storage_options=io_config)
    df = DataFrame(b)
    if file_path_column:
        # single-scan case: tag each row with its source path
        import daft_amd as _d
        parts = []
        for p in paths:
            sub = DataFrame(LogicalPlanBuilder.from_scan(
                readers.warc_schema(), [p], "warc",
                storage_options=io_config))
            parts.append(sub.with_column(file_path_column, _d.lit(p)))
        df = parts[0]
        for extra in parts[1:]:
            df = df.concat(extra)
    return df


def read_ipc(path, columns: Optional[List[str]] = None,
             io_config=None, **kwargs) -> DataFrame:
    """Read Arrow IPC (Feather v2 / .arrow) files (ref: daft-writers
    src/ipc.rs make_ipc_writer — the reference's shuffle/interchange
    format)."""
    from . import readers
    paths = _expand_paths(path, io_config)
    schema = readers.infer_schema(paths[0], "ipc",
                                  storage_options=io_config)
    b = LogicalPlanBuilder.from_scan(schema, paths, "ipc",
                                     storage_options=io_config)
    df = DataFrame(b)
    if columns:
        df = df.select(*columns)
    return df


def read_csv(path, has_headers: bool = True, delimiter: str = ",",
             schema: Optional[Dict[str, DataType]] = None,
             io_config=None, device_decode: Optional[bool] = None,
             **kwargs) -> DataFrame:
    """`device_decode`: None or True decode local, uncompressed files on the
    execution device when it is a GPU (kernels/csv.py); False, a CPU device,
    and compressed or remote inputs are decoded by pyarrow on the host."""
    from . import readers
    paths = _expand_paths(path)
    read_options = {"has_headers": has_headers, "delimiter": delimiter}
    if schema is not None:
        sch = Schema.from_dict(schema)
    else:
        sch = readers.infer_schema(paths[0], "csv", read_options,
                                   storage_options=io_config)
    read_options["device_decode"] = device_decode
    # the device decoder types its columns by the scan schema
    read_options["schema"] = {f.name: f.dtype for f in sch}
    return DataFrame(LogicalPlanBuilder.from_scan(
        sch, paths, "csv", storage_options=io_config,
        read_options=read_options))


def read_json(path, io_config=None, device_decode: Optional[bool] = None,
              **kwargs) -> DataFrame:
    """`device_decode=True` decodes local, uncompressed JSON-lines files on
    the execution device when it is a GPU (kernels/jsonl.py).  None (the
    default, as the device path measured no faster end to end), False, a CPU
    device, and compressed or remote inputs are decoded by pyarrow on the
    host."""
    from . import readers
    paths = _expand_paths(path)
    sch = readers.infer_schema(paths[0], "json",
                               storage_options=io_config)
    # the device decoder finds and types its columns by the scan schema
    read_options = {"device_decode": device_decode,
                    "schema": {f.name: f.dtype for f in sch}}
    return DataFrame(LogicalPlanBuilder.from_scan(
        sch, paths, "json", storage_options=io_config,
        read_options=read_options))


def read_text(path, line_column: str = "text") -> DataFrame:
    """Read text files line-by-line (ref capability: daft-text read.rs)."""
    paths = _expand_paths(path)
    lines: List[str] = []
    for p in paths:
        with open(p, "r", errors="replace") as f:
            lines.extend(l.rstrip("\n") for l in f)
    return from_pydict({line_column: lines})


def read_jsonl(path, device_decode: Optional[bool] = None) -> DataFrame:
    """Read newline-delimited JSON (alias of read_json for local files)."""
    return read_json(path, device_decode=device_decode)


def read_sql(sql: str, conn_factory, partition_col=None, **kwargs) -> DataFrame:
    """Read from any DB-API connection factory (capability of
    daft.read_sql; works offline against sqlite3)."""
    conn = conn_factory() if callable(conn_factory) else conn_factory
    cur = conn.cursor()
    cur.execute(sql)
    names = [d[0] for d in cur.description]
    rows = cur.fetchall()
    data = {n: [r[i] for r in rows] for i, n in enumerate(names)}
    from .. import from_pydict
    return from_pydict(data)


def from_glob_path(path: str, **kwargs) -> DataFrame:
    """One row per file matching the glob: path, size, num_rows=None
    (ref: daft.from_glob_path)."""
    import glob as _g
    import os as _os
    paths = sorted(_g.glob(path, recursive=True))
    return _from_file_rows([p for p in paths if _os.path.isfile(p)])


def from_files(paths, **kwargs) -> DataFrame:
    if isinstance(paths, str):
        return from_glob_path(paths)
    return _from_file_rows(list(paths))


def _from_file_rows(paths) -> DataFrame:
    import os as _os
    from .. import from_pydict
    return from_pydict({
        "path": paths,
        "size": [_os.path.getsize(p) if _os.path.exists(p) else None
                 for p in paths],
        "num_rows": [None] * len(paths),
    })


def read_blob(path, **kwargs) -> DataFrame:
    """Read whole files as binary rows: path + data (ref capability:
    daft read of raw blobs)."""
    import glob as _g
    import os as _os
    paths = sorted(_g.glob(path, recursive=True)) \
        if isinstance(path, str) else list(path)
    paths = [p for p in paths if _os.path.isfile(p)]
    from .. import from_pydict
    return from_pydict({
        "path": paths,
        "data": [open(p, "rb").read() for p in paths],
    })


def _gated_reader(name, needs):
    def make(*a, **k):
        raise RuntimeError(
            f"{name}() requires {needs}, which is not available in this "
            f"offline build")
    make.__name__ = name
    return make


read_deltalake = _gated_reader("read_deltalake", "deltalake")
read_iceberg = _gated_reader("read_iceberg", "pyiceberg")
read_lance = _gated_reader("read_lance", "lance")
read_hudi = _gated_reader("read_hudi", "hudi")
read_kafka = _gated_reader("read_kafka", "a kafka client")
read_mcap = _gated_reader("read_mcap", "mcap")
read_paimon = _gated_reader("read_paimon", "paimon")
read_huggingface = _gated_reader("read_huggingface",
                                 "network access to the HF hub")
read_video_frames = _gated_reader("read_video_frames", "ffmpeg")

from .object_store import (  # noqa: F401,E402  config/API parity exports
    AzureConfig, CosConfig, GCSConfig, GooseFSConfig, GravitinoConfig,
    HTTPConfig, HdfsConfig, HuggingFaceConfig, IOConfig, S3Config,
    S3Credentials, TosConfig, UnityConfig)
from .source import (  # noqa: F401,E402
    DataSource, DataSourceTask, Pushdowns, read_source)
from .sink import DataSink, WriteResult  # noqa: F401,E402
from .vendor import (  # noqa: E402,F401  gated vendor surfaces
    BigtableDataSink, ClickHouseDataSink, GravitinoCatalog,
    GravitinoClient, PaimonDataSink, TurbopufferDataSink, UnityCatalog,
    UnityCatalogClient, UnityCatalogTable, load_gravitino)

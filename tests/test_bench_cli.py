"""bench.py command line: the result line, --steps, --dump-outputs, --full.
One tiny run (SF 0.01, two queries) shared by the tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 0.01
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "0", "--sf", str(SF),
        "--queries", "1,6"]


def _bench(extra):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")]
                       + ARGS + extra, cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines          # exactly one JSON result line
    return json.loads(lines[0]), p.stderr


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    result, err = _bench(["--full", "--dump-outputs", str(out)])
    return result, err, out


def test_result_line_and_steps(dumped):
    result, err, _ = dumped
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in result
    assert result["unit"] == "s" and result["higher_is_better"] is False
    assert result["steps"] == 2
    # --steps really sets the number of timed passes
    assert sum("[bench] step " in l for l in err.splitlines()) == 2
    # value is rounded to 1 ms, ms_per_step to 0.1 ms
    assert result["ms_per_step"] == pytest.approx(result["value"] * 1000.0,
                                                  abs=0.56)


def test_dump_outputs_match_direct_run(dumped):
    """The dumped arrays are what the queries return on the same inputs."""
    import daft_amd  # noqa: F401
    from benchmarks.tpch import datagen, queries
    from bench import _column_to_f64
    _, _, out = dumped
    names = sorted(os.listdir(out))
    assert names and all(n.endswith(".npy") for n in names)
    assert sum(os.path.getsize(out / n) for n in names) <= 64 << 20
    assert {n[:3] for n in names} == {"q01", "q06"}
    device = "cuda:0" if __import__("torch").cuda.is_available() else "cpu"
    tables = datagen.dataframes(SF, device=device)
    for qi in (1, 6):
        want = queries.run_query(qi, tables, sf=SF).to_pydict()
        for col_name, values in want.items():
            got = np.load(out / ("q%02d__%s.npy" % (qi, col_name)))
            assert got.dtype == np.float64
            # fp64 sums over <= 6e4 rows in any order: 6e4 * 2.2e-16 ~ 1e-11
            np.testing.assert_allclose(got, _column_to_f64(values),
                                       rtol=1e-9, equal_nan=True)

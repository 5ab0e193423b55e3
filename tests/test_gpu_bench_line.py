"""bench.py's plain line (no --full) and its --dump-outputs files, on the small `smoke` workload: the line carries the
contract keys and none of the --full measurements, and the dumped arrays are the timed path's result, equal to the
CPU oracle's."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_line_and_dumped_outputs(tmp_path, oracle):
    out = tmp_path / "outputs"
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--workload", "smoke", "--steps", "4",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 4 and line["warmup"] == 1 and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(100 * 1e3 / line["ms_per_step"], rel=1e-2)      # 100 queries per step
    for key in ("value_host_io", "cpu_baseline", "cpu_baselines", "ids_equal_cpu_oracle_first32", "also"):
        assert key not in line, key

    from bench import make_data

    X, Q, k, metric = make_data("smoke", 0)
    D, I = np.load(out / "distances.npy"), np.load(out / "ids.npy")
    assert D.dtype == np.float32 and I.dtype == np.float64 and D.shape == I.shape == (Q.shape[0], k)
    Do, Io = oracle.knn(X, Q, k, metric)
    assert np.array_equal(I, Io.astype(np.float64)) and np.array_equal(D, Do)

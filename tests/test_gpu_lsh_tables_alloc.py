"""Every device allocation of a handle with LSH hash tables is given back: the $VDBHIP_ALLOC_LOG of one child process that
installs tables, adds, runs the candidate and search calls (fallback included), resets, re-fills, installs other tables and
destroys the handle must pair each "A" line with a later "F" line of the same address and size (test_gpu_alloc_balance.check_log).

The library opens the log once per process, hence the child: this file run as a script (`--child`).  The parent only reads the
log; nothing here provokes a fault."""
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
CHILD_TIMEOUT_S = 120


def child() -> None:
    sys.path[:0] = [str(ROOT), str(ROOT / "vectordb-retrieval_amd")]
    import vdbhip
    from vdbhip.lsh_tables import make_tables

    rng = np.random.default_rng(1)
    X = rng.standard_normal((40000, 32)).astype(np.float32)       # above the sample: both scans run
    Q = rng.standard_normal((64, 32)).astype(np.float32)
    report = {}
    idx = vdbhip.FlatIndex(32, "l2", 0)
    p, b = make_tables(32, 6, 3, "l2", 2.0, 1)
    idx.lsht_set_tables(p, b, 2.0)
    report["tables_only"] = idx.stats()["bytes_resident"]
    idx.add(X[:30000])
    idx.add(X[30000:])
    report["rows"] = idx.stats()["bytes_resident"]
    votes, ids = idx.lsht_candidates(Q, 64)
    for fallback in (False, True):
        idx.lsht_search(Q, 10, 64, fallback)
    idx.set_option("lsh_force_fallback", 1)
    votes2, ids2 = idx.lsht_candidates(Q, 64)
    assert np.array_equal(ids, ids2) and np.array_equal(votes, votes2)
    idx.set_option("lsh_force_fallback", 0)
    report["searched"] = idx.stats()["bytes_resident"]
    report["workspace"] = idx.stats()["bytes_workspace"]
    idx.reset()
    report["reset"] = idx.stats()["bytes_resident"]
    idx.add(X)
    p2, _ = make_tables(32, 24, 40, "cosine", 4.0, 2)             # other tables, wider keys: the rows are keyed again
    idx.lsht_set_tables(p2)
    idx.lsht_search(Q, 10, 2560, True)
    report["rekeyed"] = idx.stats()["bytes_resident"]
    idx.close()
    print("LSHT_ALLOC_REPORT " + json.dumps(report), flush=True)


def test_every_allocation_of_a_handle_with_tables_is_freed_once(tmp_path):
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gpu_alloc_balance import check_log

    log = tmp_path / "alloc.log"
    env = dict(os.environ, VDBHIP_ALLOC_LOG=str(log))
    run = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, cwd=str(ROOT), timeout=CHILD_TIMEOUT_S,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    tail = [ln for ln in run.stdout.splitlines() if ln.startswith("LSHT_ALLOC_REPORT ")]
    assert tail, run.stdout[-4000:]
    report = json.loads(tail[-1].split(" ", 1)[1])
    print(json.dumps(report))
    tables = 6 * 3 * 32 * 4 + 6 * 3 * 4
    assert report["tables_only"] == tables                      # transposed projections + offsets, exactly sized
    key_bytes = 40000 * 6 * 3 * 4
    assert report["rows"] >= report["tables_only"] + 40000 * 32 * 4 + key_bytes
    assert 0 < report["searched"] - report["rows"] <= report["workspace"]
    assert report["reset"] < report["tables_only"] + report["workspace"] + 4096      # rows and keys gone; tables, workspace and the statistics block stay
    assert report["rekeyed"] > report["searched"]               # 24 tables x 2 words
    problems, seen = check_log(log.read_text().splitlines())
    print(f"{seen} allocations, {len(problems)} problems")
    assert seen > 20
    assert not problems, "\n".join(problems[:40])


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()

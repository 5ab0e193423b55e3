"""The inputs of tests/test_gpu_guard.py must make the exactness guard decisive -- checked here, on the CPU.

A condition, not a measurement: for every case of the GPU file the NumPy emulation of the scan (tests/guard_cases.py) returns
a wrong top-k set for at least FLOOR of the queries whose exact k-th and (k + 1)-th keys differ.  A case whose inputs fall
below the floor would pass on the GPU with the guard removed; it fails here instead."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import pq_restatement as pq_ref  # noqa: E402

from tests import guard_cases as gc  # noqa: E402
from tests.helpers import np_decode, np_encode, np_ranges  # noqa: E402


def host_corpus(c):
    """(rows the search ranks, Q, restrict) of a case, everything the GPU would do to the rows restated on the host."""
    X, Q, cb = gc.case_inputs(c)
    restrict = None
    if c.index == "pq":
        X = pq_ref.reconstruct(X, cb)
    elif c.index in ("ivf", "sq8"):
        C = gc.ivf_centroids(c.d, c.kind)
        lor = gc.host_assign(C, X, c.metric)
        gc.check_list_layout(lor, c)
        if c.index == "sq8":
            vmin, vdiff = np_ranges(X, C, lor)
            X = np_decode(np_encode(X, C, lor, vmin, vdiff), C, lor, vmin, vdiff)
        restrict = gc.probed_mask(C, lor, Q, c.metric, c.nprobe)
    return X, Q, restrict


_BY_KEY = {}
for _c in gc.CASES:
    _BY_KEY.setdefault(_c.data_key, _c)


@pytest.mark.parametrize("case", list(_BY_KEY.values()), ids=lambda c: c.id)
def test_inputs_make_the_guard_decisive(case):
    X, Q, restrict = host_corpus(case)
    crit = gc.critical_mask(X, Q, case.metric, case.k, restrict)
    share = float(crit.mean())
    print(f"{case.id}: critical share {share:.3f} of {len(Q)} queries")
    assert share >= gc.FLOOR, share
    # (cases that search fewer queries than they generate take the critical ones first: there must be that many)
    fewest = min(c.nq for c in gc.CASES if c.data_key == case.data_key)
    assert crit.sum() >= min(fewest, 64), (int(crit.sum()), fewest)


def test_case_table_is_well_formed():
    ids = [c.id for c in gc.CASES]
    assert len(set(ids)) == len(ids)
    for c in gc.CASES:
        assert c.nb % 8 == 0 and (c.index == "coarse" or c.nb % 1024 == 0), c.id
        assert c.metric in ("l2", "ip") and c.layout in ("blocked", "strided", "strided32")
        assert c.layout != "strided32" or c.nb % 32 == 0
    assert {c.family for c in gc.CASES} == {"flat128", "flat_kloop", "dense", "shards", "ivf128", "ivf_kloop", "coarse",
                                            "ivf_sq8", "pq"}


def test_layouts_place_the_replicas_where_they_say():
    nb, k = 2048, 4
    for layout in ("blocked", "strided", "strided32"):
        X, _ = gc.make_clusters(nb, k, 16, 8, 3, layout, "gauss")
        rows = gc.cluster_rows(nb, k, layout)
        assert sorted(rows.ravel().tolist()) == list(range(nb * (k + 1)))
        rel = np.abs(X[rows[:, 1:]] / X[rows[:, :1]] - 1.0).max()          # every replica is a near-copy of replica 0
        assert 0 < rel < 20 * gc.REL
        if layout == "blocked":
            assert (np.diff(rows, axis=1) == nb).all()
        elif layout == "strided":
            assert (np.diff(rows, axis=1) == 8).all() and (rows // 256 == rows[:, :1] // 256).mean() > 0.8
        else:
            assert (np.diff(rows, axis=1) == 32).all()


def test_kinds_that_no_gpu_case_uses():
    """"offset" (cancellation in ||x||^2 - 2 q.x) makes most queries critical, but its eps exceeds the spacing of the rows, so on
    the GPU every query would take the exhaustive fallback, which hides the guard: host only.  "bytes" (a corpus that is exact
    in fp16, fractional queries) stays below the floor under either metric: only the query rounds.  (A variant tuned to clear
    the floor -- steps up only, query shift 0.5 -- did so through emulated ties alone, and no case of it failed on the GPU with
    the 2 eps term removed: the family is left out.)"""
    X, Q = gc.make_clusters(4096, 1, 64, 128, 2, "blocked", "offset")
    assert gc.critical_share(X, Q, "l2", 1) >= gc.FLOOR
    for k in (1, 4):
        X, Q = gc.make_clusters(4096, k, 64, 128, 2, "blocked", "bytes")
        assert gc.critical_share(X, Q, "l2", k) < gc.FLOOR and gc.critical_share(X, Q, "ip", k) < gc.FLOOR

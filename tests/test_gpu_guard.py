"""Near-tie corpora on every scan path: searches that are exact only because of the exactness guard.

Every case of tests/guard_cases.py builds its index, searches, and compares ids and distances bit for bit with the CPU oracle
(over the reconstructed rows for SQ8 and PQ).  The k + 1 nearest rows of every query are near-copies of one row whose fp16
scores the scan cannot order, so a select that forgets the 2 eps term, a panel producer that rounds differently from the bound's
assumptions or an eps in the wrong units returns a wrong id.  Each case also asserts that the intended path served the batch and
that NO query fell back to the exhaustive pass, which would hide the guard.  tests/test_guard_host.py holds the same inputs to
a floor on the share of queries the guard decides."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import pq_restatement as pq_ref  # noqa: E402

from tests import guard_cases as gc  # noqa: E402
from tests.helpers import np_decode  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}         # the inputs of the last data key: cases that differ in options only share rows, queries and oracle result


def _inputs(c):
    if _cache.get("key") != c.data_key:
        _cache.clear()
        X, Q, cb = gc.case_inputs(c)
        _cache.update(key=c.data_key, X=X, Q=Q, cb=cb, want={})
    return _cache["X"], _cache["Q"], _cache["cb"]


def _queries(c, rows, Q, restrict=None):
    """the queries of the case: all NQ, or the first c.nq with the ones the host emulation calls critical in front"""
    if c.nq >= len(Q):
        return Q
    tag = ("crit", c.k)
    if tag not in _cache:
        _cache[tag] = gc.critical_mask(rows, Q, c.metric, c.k, restrict)
    return np.ascontiguousarray(Q[gc.pick_queries(c, Q, _cache[tag])])


def _want(c, make):
    """the oracle's answer, computed once per (data, nq)"""
    if c.nq not in _cache["want"]:
        _cache["want"][c.nq] = make()
    return _cache["want"][c.nq]


def _options(idx, opts):
    for name, value in opts:
        idx.set_option(name, value)


def _check(c, got, want, st, path, dtype=0):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])
    assert st["last_path_name"] == path and st["scan_dtype"] == dtype, st
    assert st["last_fallback_queries"] == 0, st
    if c.layout == "blocked":        # replicas in different bins: each is a bin minimum, i.e. a candidate
        assert st["last_candidates"] > 0, st
    else:                            # replicas inside one bin: its second minimum passes the threshold and the bin is re-scanned
        assert st["last_candidates"] + st["last_rescan_bins"] > 0, st
    if c.shape >= 0:
        assert st["scan_shape"] == c.shape, st


def _run_flat(c, vdb, oracle):
    X, Q, _ = _inputs(c)
    q = _queries(c, X, Q)
    idx = vdb.FlatIndex(c.d, c.metric, [0, 0, 0] if c.index == "multi" else 0)
    try:
        _options(idx, c.pre)
        if c.index == "multi":
            idx.set_option("multi_stage_all", 1)
        idx.add(X)
        _options(idx, c.post)
        if len(X) < 32768 and c.family != "dense":
            idx.set_option("force_path", 2)
        got = idx.search(q, c.k)
        st = idx.stats()
        _check(c, got, _want(c, lambda: oracle.knn(X, q, c.k, c.metric)), st, "mfma_scan")
    finally:
        idx.close()


def _run_partial(c, vdb, oracle):
    """two shards of two replica blocks each: partial lists (float64 keys, global ids) per shard, merged on the device"""
    import torch

    X, Q, _ = _inputs(c)
    half = len(X) // 2
    q_t = torch.from_numpy(Q.copy()).cuda()
    keys = torch.empty((2, len(Q), c.k), dtype=torch.float64, device="cuda")
    ids = torch.empty((2, len(Q), c.k), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for p in range(2):
        s = vdb.FlatIndex(c.d, c.metric, 0)
        try:
            s.add(X[p * half:(p + 1) * half], id_base=p * half)
            s.search_partial_device(q_t.data_ptr(), len(Q), c.k, keys[p].data_ptr(), ids[p].data_ptr(), stream)
            torch.cuda.synchronize()
            st = s.stats()
            assert st["last_path_name"] == "mfma_scan" and st["last_candidates"] > 0 and st["last_fallback_queries"] == 0, st
        finally:
            s.close()
    D = torch.empty((len(Q), c.k), dtype=torch.float32, device="cuda")
    I = torch.empty((len(Q), c.k), dtype=torch.int64, device="cuda")
    vdb.merge_partials_device(c.metric, 0, keys.data_ptr(), ids.data_ptr(), 2, len(Q), c.k, D.data_ptr(), I.data_ptr(), stream)
    torch.cuda.synchronize()
    Do, Io = oracle.knn(X, Q, c.k, c.metric)
    np.testing.assert_array_equal(I.cpu().numpy(), Io)
    np.testing.assert_array_equal(D.cpu().numpy(), Do)


def _run_ivf(c, vdb, oracle):
    X, Q, _ = _inputs(c)
    C = gc.ivf_centroids(c.d, c.kind)
    idx = (vdb.IVFSQ8Index if c.index == "sq8" else vdb.IVFFlatIndex)(c.d, 4, c.metric, 0)
    try:
        idx.set_centroids(C)
        _options(idx, c.pre)
        if c.index == "sq8":
            idx.train_ranges(X)
        idx.add(X)
        _options(idx, c.post)
        lor = idx.assignment()
        gc.check_list_layout(lor, c)        # (blocked: replicas in different bins; strided32: in other quads of one bin)
        rows = X
        if c.index == "sq8":
            vmin, vdiff = idx.ranges()
            rows = np_decode(idx.codes(), C, lor, vmin, vdiff)
        idx.set_nprobe(c.nprobe)
        got = idx.search(Q, c.k)
        st = idx.stats()
        _check(c, got, _want(c, lambda: oracle.ivf_search(rows, C, lor, Q, c.k, c.nprobe, c.metric)), st, "ivf",
               2 if c.index == "sq8" else 0)
    finally:
        idx.close()


def _run_coarse(c, vdb, oracle):
    """The centroids are the near-copies: the rows must be filed under the truly nearer centroid of a pair, and a search must
    probe it (the coarse quantizer's register select in set-only mode).  The coarse index exposes no statistics, so its path is
    NOT asserted: 128 centroids and batches of >= 64 rows are what search_batch sends to the dense register select."""
    C, X, _ = _inputs(c)
    idx = vdb.IVFFlatIndex(c.d, len(C), c.metric, 0)
    try:
        idx.set_centroids(C)
        idx.add(X)
        lor = idx.assignment()
        want = _want(c, lambda: oracle.ivf_assign(C, X, c.metric))
        np.testing.assert_array_equal(lor, want)
        assert len(np.unique(lor)) > len(C) // 2            # (both centroids of most pairs own rows)
        idx.set_nprobe(1)
        Q = X[:gc.NQ] + np.float32(0.01)
        got = idx.search(Q, 1)
        Do, Io = oracle.ivf_search(X, C, lor, Q, 1, 1, c.metric)
        np.testing.assert_array_equal(got[1], Io)
        np.testing.assert_array_equal(got[0], Do)
        assert idx.stats()["last_fallback_queries"] == 0
    finally:
        idx.close()


def _run_pq(c, vdb, oracle):
    codes, Q, cb = _inputs(c)
    rows = pq_ref.reconstruct(codes, cb)
    idx = vdb.PQIndex(c.d, 16, c.metric, 0)
    try:
        idx.set_codebooks(cb)
        idx.add_codes(codes)
        _options(idx, c.post)
        got = idx.search(Q, c.k)
        _check(c, got, _want(c, lambda: oracle.knn(rows, Q, c.k, c.metric)), idx.stats(), "mfma_scan", 2)
    finally:
        idx.close()


_RUN = {"flat": _run_flat, "multi": _run_flat, "partial": _run_partial, "ivf": _run_ivf, "sq8": _run_ivf, "coarse": _run_coarse,
        "pq": _run_pq}


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_near_ties_are_resolved_exactly(case, vdb, oracle):
    _RUN[case.index](case, vdb, oracle)

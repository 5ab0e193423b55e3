"""Range search (vdb_range_search / vdb_range_results and their device variants) against the contract of include/vdbhip.h.

Expected results come from the CPU: oracle.c_oracle.pair_keys gives the canonical float64 keys of every (query, row) pair and
range_cases.expected applies the rule -- np.float32(key) < r (L2) / np.float32(-key) > r (IP), ascending id, D the same float32
values.  Every comparison is bit for bit on lims, I and D (the payload of a NaN is never compared: NaN rows are never returned).

Three routes: the prefilter scan on layout "x16" (D <= 128, above 15 360 rows), the one on p16 panels (D > 128, above
2048 rows), and the all-ones path of every other handle.  The shapes are the smallest at which each route is still the one taken."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT / "vectordb-retrieval_amd"), str(ROOT), str(ROOT / "tests")):      # (also when this file runs as the child script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import admission_cases as ac  # noqa: E402
import hostile_cases as hc  # noqa: E402

from tests import range_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
_KEYS = {}          # the oracle's keys, computed once per (corpus, queries, metric) and shared


def _keys(oracle, tag, X, Q, metric):
    key = (tag, X.shape, Q.shape, metric)
    if key not in _KEYS:
        _KEYS[key] = oracle.pair_keys(X, Q, np.tile(np.arange(len(X), dtype=np.int64), (len(Q), 1)), metric)
        _KEYS[key].flags.writeable = False
    return _KEYS[key]


def _same(got, want, what):
    for name, g, w in zip(("lims", "D", "I"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(g != w)[:5])


def _gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F32)


def _index(vdb, X, metric, opts=(), id_base=0):
    idx = vdb.FlatIndex(X.shape[1], metric, 0)
    try:
        for name, value in opts:
            idx.set_option(name, value)
        idx.add(X, id_base=id_base)
    except Exception:
        idx.close()
        raise
    return idx


def _radius_at(keys_of_query, metric, rank):
    """the float32 distance of the query's rank-th nearest row (0-based): `<` / `>` then keeps the rows strictly nearer"""
    d = np.sort((keys_of_query if metric == "l2" else -keys_of_query).astype(F32))
    return float(d[rank] if metric == "l2" else d[::-1][rank])


# ---- parity on the three routes --------------------------------------------------------------------------------------------------
ROUTES = [("x16", 16421, 64, ()), ("x16", 16421, 100, ()), ("p16", 2203, 200, ()), ("p16", 2100, 384, ()),
          ("ones", 300, 16, ()), ("ones", 16421, 64, (("flat_shape", 32),)),
          ("x16", 15500, 30, ()), ("p16", 2203, 130, ())]        # (D no multiple of 4: the queries are padded for the exact filter)
NQS = (1, 15, 16, 17, 33, 130)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("route,n,d,opts", ROUTES, ids=[f"{r[0]}-{r[1]}x{r[2]}" for r in ROUTES])
def test_parity_on_every_route(route, n, d, opts, metric, vdb, oracle):
    X, Q = _gauss(n, d, 100 + d), _gauss(max(NQS), d, 200 + d)
    keys = _keys(oracle, "parity", X, Q, metric)
    radii = [_radius_at(keys[0], metric, rank) for rank in (0, 10, n // 2)]
    for id_base in (0, 10 ** 6):
        idx = _index(vdb, X, metric, opts, id_base)
        try:
            assert idx.stats()["scan_shape"] == {"x16": 16, "p16": 0, "ones": 32}[route]
            for nq in NQS:
                for which, r in enumerate(radii):
                    what = f"{route} {n}x{d} {metric} nq={nq} id_base={id_base} radius#{which}={r}"
                    want = rc.expected(keys[:nq], r, metric, id_base)
                    got = idx.range_search(Q[:nq], r)
                    st = idx.stats()
                    _same(got, want, what)
                    total = int(want[0][-1])
                    assert st["last_path_name"] == "range" and st["last_nq"] == nq and st["scan_dtype"] == 0, (what, st)
                    if route == "ones":
                        assert st["last_fallback_queries"] == nq and st["last_candidates"] == nq * n, (what, st)
                    else:
                        assert st["last_fallback_queries"] == 0 and total <= st["last_candidates"] <= nq * n, (what, st)
                        if which == 1:      # the prefilter ran: far fewer pairs were scored than there are
                            assert st["last_candidates"] < nq * n / 4, (what, st)
        finally:
            idx.close()


# ---- census: every row, every bit position of every span ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(16421, 32), (2203, 160)], ids=["x16", "p16"])
def test_census_every_row_is_found_alone_and_none_beyond_n(n, d, vdb, oracle):
    X = _gauss(n, d, 300 + d)
    d2, _ = oracle.knn(X, X, 2, "l2")
    assert (d2[:, 0] == 0).all()
    radius = float(F32(d2[:, 1].min() / 2))                     # below the smallest pairwise distance, confirmed on the CPU
    assert radius > 0
    idx = _index(vdb, X, "l2")
    try:
        lims, D, I = idx.range_search(X, radius)                # query i is row i
        st = idx.stats()
        assert np.array_equal(lims, np.arange(n + 1)) and np.array_equal(I, np.arange(n)) and D.tobytes() == np.zeros(n, F32).tobytes()
        assert st["last_fallback_queries"] == 0 and n <= st["last_candidates"] < n * n / 4, st
        Q = X[np.linspace(0, n - 1, 33).astype(np.int64)]
        keys = _keys(oracle, "census", X, Q, "l2")
        for r in (FLT_MAX, float("inf")):
            lims, D, I = idx.range_search(Q, r)
            assert np.array_equal(lims, n * np.arange(34)), r
            assert np.array_equal(I, np.tile(np.arange(n), 33)) and I.max() < n, r
            _same((lims, D, I), rc.expected(keys, r, "l2"), f"radius {r}")
    finally:
        idx.close()


# ---- near-threshold: the `+ eps` of the threshold decides ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.id)
def test_near_threshold_cases(case, vdb, oracle):
    X, Q, radius = rc.make(case)
    keys = _keys(oracle, case.id, X, Q, case.metric)
    idx = _index(vdb, X, case.metric)
    try:
        got = idx.range_search(Q, float(radius))
        st = idx.stats()
        _same(got, rc.expected(keys, radius, case.metric), case.id)
        assert st["last_fallback_queries"] == 0 and st["last_candidates"] < len(Q) * len(X) / 4, st
    finally:
        idx.close()


# ---- query slabs ------------------------------------------------------------------------------------------------------------------
def test_slabs_return_the_bytes_of_one_slab(vdb, oracle):
    n, d = 16421, 64
    words = (n + 1023) // 1024 * 32
    per_slab = (1 << 20) // (words * 4) // 128 * 128              # range_plan.hpp with "range_bitmap_mb" = 1
    nq = 2 * per_slab + 100
    assert per_slab == 384 and -(-nq // per_slab) == 3 and nq % per_slab
    X, Q = _gauss(n, d, 100 + d), _gauss(nq, d, 777)
    keys = _keys(oracle, "slabs", X, Q, "l2")
    r = _radius_at(keys[0], "l2", 10)
    idx = _index(vdb, X, "l2")
    try:
        one = idx.range_search(Q, r)
        idx.set_option("range_bitmap_mb", 1)
        three = idx.range_search(Q, r)
        _same(three, one, "three slabs against one")
        _same(one, rc.expected(keys, r, "l2"), "one slab against the oracle")
        assert idx.stats()["last_fallback_queries"] == 0
    finally:
        idx.close()


# ---- hostile values ---------------------------------------------------------------------------------------------------------------
HOSTILE_SIZES = {"x16": (15872, 16), "p16": (9300, 136), "ones": (3000, 16)}      # the sizes of test_gpu_hostile.py's flat scans


@pytest.mark.parametrize("family", [f for f in hc.FAMILIES if f != "bytes"])
@pytest.mark.parametrize("route", list(HOSTILE_SIZES))
def test_hostile_values_follow_the_rule(route, family, vdb, oracle):
    n, d = HOSTILE_SIZES[route]
    problems = []
    for g in hc.groups(family, n, d):
        for metric in g.metrics:
            idx = _index(vdb, g.corpus.X, metric)
            try:
                for b in g.batches:
                    keys = _keys(oracle, (family, g.corpus.name, b.name), g.corpus.X, b.Q, metric)
                    with np.errstate(all="ignore"):
                        dist = (keys if metric == "l2" else -keys).astype(F32)
                    finite = np.sort(dist[np.isfinite(dist)])
                    radii = [float("inf") if metric == "l2" else float("-inf")]
                    if len(finite) > 40:        # about five results per query of the batch, whatever the magnitudes
                        radii.append(float(finite[40] if metric == "l2" else finite[::-1][40]))
                    for r in radii:
                        what = f"{route}/{g.corpus.name}/{b.name}/{metric}/r={r}"
                        want = rc.expected(keys, r, metric)
                        try:
                            _same(idx.range_search(b.Q, r), want, what)
                        except AssertionError as e:
                            problems.append(" ".join(str(e).split())[:300])
                        bad = set(g.corpus.expect.get("nan_rows", ()))
                        assert not bad & set(want[2].tolist())                  # (the rule itself never returns a NaN row ...)
                        for q in b.expect.get("bad_queries", ()) if family == "nan-query" else ():
                            assert want[0][q] == want[0][q + 1]                 # (... nor anything for a NaN query)
            finally:
                idx.close()
    assert not problems, f"{len(problems)} findings:\n" + "\n".join(problems[:40])


# ---- a cross-check that needs no oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_range_equals_the_leading_part_of_a_full_search(metric, vdb):
    n, d, nq = 1500, 24, 40
    X, Q = _gauss(n, d, 5), _gauss(nq, d, 6)
    idx = _index(vdb, X, metric)
    try:
        Dk, Ik = idx.search(Q, n)
        r = float(Dk[0, 25])
        lims, D, I = idx.range_search(Q, r)
        for q in range(nq):
            inside = Dk[q] < F32(r) if metric == "l2" else Dk[q] > F32(r)
            assert inside[:inside.sum()].all()                                   # (the search is sorted: a leading part)
            dq, iq = D[lims[q]:lims[q + 1]], I[lims[q]:lims[q + 1]]
            assert (np.diff(iq) > 0).all()
            order = np.lexsort((iq, dq if metric == "l2" else -dq))
            assert np.array_equal(iq[order], Ik[q, :inside.sum()]) and dq[order].tobytes() == Dk[q, :inside.sum()].tobytes(), q
    finally:
        idx.close()


# ---- byte-valued corpora: the fp16 copy serves the prefilter, the int8 row copy the all-ones path ------------------------------------
def test_byte_valued_corpus_and_int8_only(vdb, oracle):
    n, d = 40000, 16
    rng = np.random.default_rng(9)
    X = rng.integers(0, 256, size=(n, d)).astype(F32)
    batches = {"integer": rng.integers(0, 256, size=(33, d)).astype(F32), "fractional": (rng.random((33, d)) * 255).astype(F32)}
    plain, only = _index(vdb, X, "l2"), _index(vdb, X, "l2", (("int8_only", 1),))
    try:
        assert plain.stats()["has_i8_copy"] == 1 and only.stats()["has_i8_copy"] == 2
        for name, Q in batches.items():
            keys = _keys(oracle, ("bytes", name), X, Q, "l2")
            r = _radius_at(keys[0], "l2", 10)
            want = rc.expected(keys, r, "l2")
            _same(plain.range_search(Q, r), want, f"byte-valued, {name} queries")
            st = plain.stats()
            assert st["last_fallback_queries"] == 0 and st["last_candidates"] < 33 * n / 4 and st["scan_dtype"] == 0, st
            _same(only.range_search(Q, r), want, f"int8_only, {name} queries")
            st = only.stats()
            assert st["last_fallback_queries"] == 33 and st["last_candidates"] == 33 * n, st
    finally:
        plain.close()
        only.close()


# ---- device entry points ------------------------------------------------------------------------------------------------------------
def _device_range(torch, idx, Q, r, nq=None):
    q_t = torch.from_numpy(Q).cuda()
    nq = len(Q) if nq is None else nq
    lims_t = torch.empty((nq + 1,), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    total = idx.range_search_device(q_t.data_ptr(), nq, r, lims_t.data_ptr(), stream)
    D_t = torch.empty((max(total, 1),), dtype=torch.float32, device="cuda")
    I_t = torch.empty((max(total, 1),), dtype=torch.int64, device="cuda")
    idx.range_results_device(D_t.data_ptr(), I_t.data_ptr(), stream)
    torch.cuda.synchronize()
    return total, (lims_t.cpu().numpy(), D_t.cpu().numpy()[:total], I_t.cpu().numpy()[:total])


def test_device_entry_points_equal_the_host_ones(vdb, oracle):
    import torch

    n, d, nq = 16421, 64, 33
    X, Q = _gauss(n, d, 100 + d), _gauss(130, d, 200 + d)[:nq]
    keys = _keys(oracle, "parity", X, _gauss(130, d, 200 + d), "l2")[:nq]
    r = _radius_at(keys[0], "l2", 10)
    idx = _index(vdb, X, "l2")
    try:
        host = idx.range_search(Q, r)
        total, dev = _device_range(torch, idx, Q, r)
        assert total == host[0][-1]
        _same(dev, host, "device against host")
        total2, dev2 = _device_range(torch, idx, Q, r)
        assert total2 == total
        _same(dev2, dev, "two consecutive calls")
        Dk, Ik = idx.search(Q, 10)                              # a k-NN search in between: the result stays
        assert idx.stats()["last_path_name"] != "range"
        D, I = np.empty(total, F32), np.empty(total, np.int64)
        from vdbhip import _ffi
        _ffi.check(idx._lib.vdb_range_results(idx._handle(), _ffi.ptr(D), _ffi.ptr(I)))
        assert D.tobytes() == host[1].tobytes() and I.tobytes() == host[2].tobytes()
        Dk2, Ik2 = idx.search(Q, 10)                            # ... and the range calls change no other search's result
        assert Dk.tobytes() == Dk2.tobytes() and Ik.tobytes() == Ik2.tobytes()
    finally:
        idx.close()


# ---- admission, in both directions --------------------------------------------------------------------------------------------------
def _raw_range(lib, h, Q, r, nq=None, lims=True, q=True):
    from vdbhip import _ffi

    nq = len(Q) if nq is None else nq
    out = np.zeros(len(Q) + 1, np.int64)
    rc_ = lib.vdb_range_search(h, _ffi.ptr(Q) if q else None, nq, r, _ffi.ptr(out) if lims else None)
    return rc_, out


def test_admitted_kinds_return_the_flat_bytes(vdb, oracle):
    n, d = 2000, 32
    X, Q = _gauss(n, d, 41), _gauss(17, d, 42)
    keys = _keys(oracle, "admit", X, Q, "l2")
    r = _radius_at(keys[0], "l2", 10)
    want = rc.expected(keys, r, "l2")

    def lsh(idx):
        idx.lsh_set_projection(vdb.make_projection(d, 64, seed=5))

    def lsht(idx):
        idx.lsht_set_tables(np.random.default_rng(3).standard_normal((4, 8, d)).astype(F32))

    def knng(idx):
        idx.add(X)
        ring = np.full((n, 4), -1, np.int32)
        ring[:, 0] = (np.arange(n) + 1) % n
        from vdbhip import _ffi
        _ffi.check(idx._lib.vdb_knng_set(idx._handle(), 4, _ffi.ptr(ring)))

    for name, prepare in (("flat", None), ("lsh", lsh), ("lsht", lsht), ("knng", knng)):
        idx = vdb.FlatIndex(d, "l2", 0)
        try:
            if prepare:
                prepare(idx)
            if idx.stats()["ntotal"] == 0:
                idx.add(X)
            _same(idx.range_search(Q, r), want, name)
            assert idx.stats()["last_path_name"] == "range"
        finally:
            idx.close()


REFUSED = {"16_pq_rows": "U", "15_pq_codebooks": "U", "10_ivf_flat_built": "U", "09_ivf_flat_centroids": "U", "12_sq8_built": "U",
           "14_ivfpq_built": "U", "17_multi_flat_rows": "U", "18_multi_ivf_built": "U", "03_flat_graph_option": "U", "01_flat_empty": "S"}


@pytest.mark.parametrize("state", list(REFUSED))
def test_refused_kinds_and_states(state, vdb):
    import torch
    from vdbhip import _ffi

    lib = _ffi.load()
    s = ac.STATES[state]
    c = ac.ctx(s.d, s.n, s.byte_valued)
    code = _ffi.VDB_ERR_UNSUPPORTED if REFUSED[state] == "U" else _ffi.VDB_ERR_STATE
    h = ac.build(lib, s, c)
    try:
        before = ac.own_search(lib, s, c, h) if s.search else None
        lims_t = torch.zeros((ac.NQ + 1,), dtype=torch.int64, device="cuda")
        total = ctypes.c_int64(-1)
        calls = {
            "vdb_range_search": lambda: _raw_range(lib, h, c.Q, 1.0)[0],
            "vdb_range_search_device": lambda: lib.vdb_range_search_device(h, c.tQ.data_ptr(), ac.NQ, 1.0, lims_t.data_ptr(), ctypes.byref(total), None),
            "vdb_range_results": lambda: lib.vdb_range_results(h, _ffi.ptr(c.D), _ffi.ptr(c.I)),
            "vdb_range_results_device": lambda: lib.vdb_range_results_device(h, c.tD.data_ptr(), c.tI.data_ptr(), None),
        }
        for name, call in calls.items():
            lib.vdb_device_count(None)                          # leaves a sentinel in vdb_last_error
            got = call()
            # (a flat handle with rows under option "graph" admits vdb_range_results: it only has no result to give)
            want = _ffi.VDB_ERR_STATE if name.startswith("vdb_range_results") and state == "03_flat_graph_option" else code
            assert got == want, (state, name, got, _ffi.last_error())
            assert _ffi.last_error() not in ("", ac.SENTINEL), (state, name)
            if REFUSED[state] == "U" and state != "03_flat_graph_option":
                assert name in _ffi.last_error(), _ffi.last_error()            # the usual message: the call and the kind
        torch.cuda.synchronize()
        if before is not None:
            assert ac.own_search(lib, s, c, h) == before
    finally:
        lib.vdb_destroy(h)


def test_argument_and_state_errors(vdb):
    from vdbhip import _ffi

    X, Q = _gauss(2000, 32, 41), _gauss(5, 32, 42)
    idx = _index(vdb, X, "l2")
    lib, h = idx._lib, idx._handle()
    try:
        D, I = np.empty(16, F32), np.empty(16, np.int64)
        assert lib.vdb_range_results(h, _ffi.ptr(D), _ffi.ptr(I)) == _ffi.VDB_ERR_STATE            # before any range search
        want = idx.search(Q, 5)
        assert _raw_range(lib, h, Q, float("nan"))[0] == _ffi.VDB_ERR_INVALID and "NaN" in _ffi.last_error()
        assert _raw_range(lib, h, Q, 1.0, nq=0)[0] == _ffi.VDB_ERR_INVALID
        assert _raw_range(lib, h, Q, 1.0, nq=-3)[0] == _ffi.VDB_ERR_INVALID
        assert _raw_range(lib, h, Q, 1.0, lims=False)[0] == _ffi.VDB_ERR_INVALID
        assert _raw_range(lib, h, Q, 1.0, q=False)[0] == _ffi.VDB_ERR_INVALID
        assert lib.vdb_range_results(h, _ffi.ptr(D), _ffi.ptr(I)) == _ffi.VDB_ERR_STATE            # a refused call made no result
        got = idx.search(Q, 5)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert idx.range_search(Q, -1.0)[0].tolist() == [0] * 6 and idx.range_search(Q, 0.0)[0].tolist() == [0] * 6     # L2 radius <= 0
        assert idx.range_search(Q, float("-inf"))[0].tolist() == [0] * 6
        lims, _, _ = idx.range_search(Q, 40.0)
        assert lims[-1] > 0 and lib.vdb_range_results(h, None, None) == _ffi.VDB_ERR_INVALID
        # what drops the result: an option change, an add, a reset
        for drop in (lambda: idx.set_option("timing", 0), lambda: idx.add(X[:10]), idx.reset):
            assert idx.range_search(Q, 40.0)[0][-1] > 0
            drop()
            assert lib.vdb_range_results(h, _ffi.ptr(D), _ffi.ptr(I)) == _ffi.VDB_ERR_STATE and "no range result" in _ffi.last_error()
        assert _raw_range(lib, h, Q, 1.0)[0] == _ffi.VDB_ERR_STATE                                  # the index is empty now
        idx.add(X)
        idx.set_option("graph", 1)
        assert _raw_range(lib, h, Q, 1.0)[0] == _ffi.VDB_ERR_UNSUPPORTED and "graph" in _ffi.last_error()
        idx.set_option("graph", 0)
        assert _raw_range(lib, h, Q, 40.0)[0] == _ffi.VDB_OK
        for bad in (-1, 4097):
            assert lib.vdb_set_option(h, b"range_bitmap_mb", float(bad)) == _ffi.VDB_ERR_INVALID
    finally:
        idx.close()


# ---- footprint and balance ---------------------------------------------------------------------------------------------------------
def test_workspace_grows_by_bitmap_results_and_small_arrays_and_reset_gives_it_back(vdb):
    n, d, nq = 16421, 64, 130
    X, Q = _gauss(n, d, 100 + d), _gauss(nq, d, 200 + d)
    idx = _index(vdb, X, "l2")
    try:
        idx.set_option("range_bitmap_mb", 1)
        before = idx.stats()
        lims, D, I = idx.range_search(Q, float(np.median(((X[:200] - Q[0]) ** 2).sum(axis=1))))
        after = idx.stats()
        total, words = int(lims[-1]), (n + 1023) // 1024 * 32
        assert total > 1000
        # the bitmap of the slab (at most the budget), 12 bytes per result, and per query: 4 bytes per 2048-row segment, the
        # staged queries (4 d) and their fp16 fragments (2 d, padded to 32 queries), lims, eps, threshold, flag and total (28);
        # one statistics block (4096) and the batch's scales (64).  Buffers carry 1/8 growth slack and a 16-byte floor.
        small = nq * (4 * -(-words // 64) + 4 * d + 28) + 2 * d * (nq + 31) + 8 + 4096 + 64
        bound = 1.125 * (min(1 << 20, nq * words * 4) + 12 * total + small) + 16 * 16
        grown = after["bytes_workspace"] - before["bytes_workspace"]
        assert 12 * total <= grown <= bound, (grown, bound)
        assert after["bytes_resident"] - before["bytes_resident"] == grown
        idx.reset()
        st = idx.stats()
        assert st["bytes_workspace"] == before["bytes_workspace"], (st, before)
    finally:
        idx.close()


def child() -> None:
    """add -> range search (host and device) -> reset -> re-add -> range search -> destroy, on both scan routes and the all-ones path"""
    import torch
    import vdbhip

    report = {}
    for name, n, d in (("x16", 16421, 64), ("p16", 2203, 200), ("ones", 300, 16)):
        X, Q = _gauss(n, d, 1), _gauss(40, d, 2)
        r = float(np.sort(((X - Q[0]) ** 2).sum(axis=1))[10])
        idx = vdbhip.FlatIndex(d, "l2", 0)
        idx.set_option("range_bitmap_mb", 1)
        idx.add(X)
        host = idx.range_search(Q, r)
        total, dev = _device_range(torch, idx, Q, r)
        assert total == host[0][-1] and all(a.tobytes() == b.tobytes() for a, b in zip(host, dev))
        idx.range_search(Q, 4 * r)                              # a larger result: the buffers grow
        idx.reset()
        idx.add(X)
        again = idx.range_search(Q, r)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host, again))
        report[name] = {"total": int(total), "bytes_workspace": idx.stats()["bytes_workspace"]}
        idx.close()
    print("RANGE_BALANCE_REPORT " + json.dumps(report), flush=True)


def test_every_allocation_of_a_range_cycle_is_freed_once(tmp_path):
    from tests.test_gpu_alloc_balance import check_log

    log = tmp_path / "alloc.log"
    env = dict(os.environ, VDBHIP_ALLOC_LOG=str(log))
    run = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, cwd=str(ROOT), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert any(ln.startswith("RANGE_BALANCE_REPORT ") for ln in run.stdout.splitlines()), run.stdout[-4000:]
    problems, seen = check_log(log.read_text().splitlines())
    print(f"{seen} allocations, {len(problems)} problems")
    assert seen > 30 and not problems, "\n".join(problems[:40])


# ---- plugins ----------------------------------------------------------------------------------------------------------------------
def test_exact_search_plugin_raw_conventions_and_sort(vdb, oracle):
    n, d = 2000, 32
    X, Q = _gauss(n, d, 41), _gauss(17, d, 42)
    for metric in ("l2", "ip"):
        keys = _keys(oracle, "admit", X, Q, metric)
        r = _radius_at(keys[0], metric, 10)
        want = rc.expected(keys, r, metric)
        algo = vdb.get_algorithm_instance("HipExactSearch", d, name="range", metric=metric)
        algo.build_index(X)
        _same(algo.range_search(Q, r), want, f"plugin {metric}")
        lims, D, I = algo.range_search(Q, r, sort=True)
        assert np.array_equal(lims, want[0])
        for q in range(len(Q)):
            dq, iq = want[1][lims[q]:lims[q + 1]], want[2][lims[q]:lims[q + 1]]
            order = np.lexsort((iq, dq if metric == "l2" else -dq))
            assert D[lims[q]:lims[q + 1]].tobytes() == dq[order].tobytes() and np.array_equal(I[lims[q]:lims[q + 1]], iq[order])
        algo.index.close()


@pytest.mark.parametrize("metric", ["l2", "cosine", "ip"])
def test_linear_searcher_plugin_conventions(metric, vdb, oracle):
    from vdbhip.algorithms import HipBruteForceIndexer, HipLinearSearcher, _safe_normalize, query_batch

    n, d = 2000, 32
    X, Q = _gauss(n, d, 41), _gauss(17, d, 42)
    indexer = HipBruteForceIndexer("bf", d, metric=metric)
    artifact = indexer.build(X)
    searcher = HipLinearSearcher("lin", d, metric=metric)
    searcher.attach(artifact, X)
    # a NumPy statement of the conventions: the operands the library sees, the rule on canonical keys, then sqrt / negation
    Xl = _safe_normalize(X) if metric == "cosine" else X
    Ql = query_batch(Q, metric == "cosine")
    lib_metric = "l2" if metric == "l2" else "ip"
    keys = _keys(oracle, ("linear", metric), Xl, Ql, lib_metric)
    if metric == "l2":
        radius = float(np.sqrt(_radius_at(keys[0], "l2", 10)))
        lib_radius = F32(radius) * F32(radius)
    else:
        radius = lib_radius = _radius_at(keys[0], "ip", 10)
    lims, D, I = rc.expected(keys, lib_radius, lib_metric)
    want = (lims, np.sqrt(D, dtype=F32) if metric == "l2" else -D, I)
    assert 5 <= lims[1] <= 11
    _same(searcher.range_search(Q, radius), want, metric)
    artifact.metadata["hip_index"].close()


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()

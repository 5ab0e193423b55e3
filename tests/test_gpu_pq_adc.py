"""The lookup-table (ADC) scan of a flat PQ<M> index (option "pq_adc_max_batch", csrc/pq_adc.hpp) on the device.

Every index gets injected codebooks and codes (no training but in the plugin test).  The contract does not move with the option:
ids and distances are, bit for bit, the flat exact search over the decoded rows x^ (oracle.knn).  What is new is checked on its
own: the raw scores against tests/pq_adc_restatement.py bit for bit, the bound, the bin records through a census of every row,
the routing, the workspace, the admission of the test hook."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import admission_cases as ac
from tests import census
from tests import census_coded as cc
from tests import pq_adc_restatement as ar
from tests.test_gpu_census_flat import census_run, check
from tests.test_pq_adc_host import GUARD, guard_inputs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
ADC = {"last_path_name": "pq_adc", "scan_dtype": 3, "last_fallback_queries": 0}


def _random_pq(n, d, M, seed, nq=16):
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((M, 256, d // M)).astype(F32)
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    Q = rng.standard_normal((nq, d)).astype(F32)
    return cb, codes, Q


def _index(vdb, d, M, metric, cb, codes, opts=None, id_base=0):
    idx = vdb.PQIndex(d, M, metric, 0)
    for name, value in (opts or {}).items():
        idx.set_option(name, value)
    idx.set_codebooks(cb)
    idx.add_codes(codes, id_base=id_base)
    return idx


# ---- 1. scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,M", [(64, 8), (100, 50), (128, 128), (384, 64), (200, 25)])
def test_scores_bit_for_bit_and_within_the_bound(vdb, d, M):
    n = 3000
    cb, codes, Q = _random_pq(n, d, M, 7 * d + M)
    X = ar.decode(cb, codes)
    Xn = ar.xnorm_max(X)
    for metric in ("ip", "l2"):
        idx = _index(vdb, d, M, metric, cb, codes)
        cs_want = ar.cs_of(X, Q, metric)
        T = ar.tables(cb, Q, metric, cs_want)
        bias = ar.bias_of(X, metric)
        for row0, nrows in ((0, 2048), (n - 300, 300)):
            s, eps, cs = idx.debug_adc_scores(Q, row0, nrows)
            assert cs == cs_want
            want = ar.scores(T, codes[row0:row0 + nrows], bias[row0:row0 + nrows], cs)
            if metric == "ip":                                   # bias 0: the sum of the table entries alone, bit for bit
                np.testing.assert_array_equal(s.view(np.uint32), want.view(np.uint32))
            np.testing.assert_allclose(eps, ar.eps(Q, M, metric, Xn, cs), rtol=1e-6)
            keys = ar.exact_scaled_keys(X[row0:row0 + nrows], Q, metric, cs)
            worst = float((np.abs(s.astype(np.float64) - keys) / eps.astype(np.float64)[:, None]).max())
            print(f"D={d} M={M} {metric} rows {row0}+{nrows}: worst |score - key| / eps = {worst:.4f}")
            assert worst <= 1.0
        idx.close()


# ---- 2. census ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d,M,construction,kind,n", [s for s in cc.PQ_SHAPES if s[1] <= 128], ids=lambda v: str(v))
def test_census_every_row_through_the_adc_scan(vdb, oracle, d, M, construction, kind, n, metric):
    """Every decoded row is a query (k = 2: itself, then its planted twin), 512 per call: a bin record written to the wrong place, a
    group id off by one or a row scored from another row's codes loses a row's own group from the candidates."""
    g = census.scan_geometry(n, d, 2, 512, 2)
    assert g.ok and g.chunk_sizes() == {1, 2} and g.rem != 0 and n % census.span_rows(d) in (1, 11, 100)
    assert ar.admitted(n, d, M, 2, 512, 512, force_path=2, spans_per_chunk=2)
    c = cc.case(construction, kind, n, d, M)
    c.ref("twin", metric, 2)
    idx = _index(vdb, d, M, metric, c.cb, c.codes, {"force_path": 2, "spans_per_chunk": 2, "pq_adc_max_batch": 512})
    D, I = census_run(idx, c.X, 512, 2, np.arange(n), ADC)
    idx.close()
    check(oracle, c, "twin", metric, 2, D, I)


# ---- 3. guard -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,k,layout,metric,rel", GUARD)
def test_guard_cases_stay_exact(vdb, oracle, nb, k, layout, metric, rel):
    """The cases tests/test_pq_adc_host.py holds to the floor: a select without the 2 eps term answers a fifth of them wrongly."""
    cb, codes, Q = guard_inputs(nb, k, layout, rel)
    X = ar.decode(cb, codes)
    idx = _index(vdb, 64, 16, metric, cb, codes, {"pq_adc_max_batch": 512})
    D, I = idx.search(Q, k)
    st = idx.stats()
    idx.close()
    assert {key: st[key] for key in ADC} == ADC
    Do, Io = oracle.knn(X, Q, k, metric)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)


# ---- 4. parity and routing ------------------------------------------------------------------------------------------------------
N4, D4, M4 = 40_000, 64, 16


@pytest.fixture(scope="module")
def parity():
    cb, codes, Q = _random_pq(N4, D4, M4, 44, nq=17)
    return cb, codes, Q, ar.decode(cb, codes)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_parity_and_routing(vdb, oracle, parity, metric):
    cb, codes, Q, X = parity
    off = _index(vdb, D4, M4, metric, cb, codes)
    on = _index(vdb, D4, M4, metric, cb, codes, {"pq_adc_max_batch": 16})
    assert not census.scan_geometry(N4, D4, 100, 1).ok and census.scan_geometry_direct(N4, D4, 100).direct_rows   # k = 100: direct bins
    for k in (1, 10, 100, 2000):
        Do, Io = oracle.knn(X, Q, k, metric)
        for nq in (1, 2, 3, 16, 17):
            D0, I0 = off.search(Q[:nq], k)
            p0 = off.stats()["last_path_name"]
            D1, I1 = on.search(Q[:nq], k)
            st = on.stats()
            adc = nq <= 16 and k <= 10
            assert st["last_path_name"] == ("pq_adc" if adc else p0), (k, nq, st["last_path_name"], p0)
            assert p0 == ("exact_scan" if k == 2000 else "mfma_scan") and st["scan_dtype"] == (3 if adc else 0 if k == 2000 else 2)
            if adc:
                assert st["last_fallback_queries"] == 0 and st["last_candidates"] + st["last_rescan_bins"] >= nq
            np.testing.assert_array_equal(I1, I0)
            np.testing.assert_array_equal(D1, D0)
            np.testing.assert_array_equal(I1, Io[:nq])
            np.testing.assert_array_equal(D1, Do[:nq])
    # list_cap = 1: every work list overflows, the exhaustive pass answers, still exact
    on.set_option("list_cap", 1)
    D1, I1 = on.search(Q[:16], 10)
    st = on.stats()
    assert st["last_path_name"] == "pq_adc" and st["last_fallback_queries"] == 16
    Do, Io = oracle.knn(X, Q[:16], 10, metric)
    np.testing.assert_array_equal(I1, Io)
    np.testing.assert_array_equal(D1, Do)
    on.set_option("list_cap", 0)
    # a NaN query: whatever the option-0 handle returns
    Qn = Q[:3].copy()
    Qn[1, 5] = np.nan
    D0, I0 = off.search(Qn, 10)
    D1, I1 = on.search(Qn, 10)
    assert on.stats()["last_path_name"] == "pq_adc"
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1.view(np.uint32), D0.view(np.uint32))
    off.close()
    on.close()


def test_id_base_appends_and_reset(vdb, oracle, parity):
    cb, codes, Q, X = parity
    idx = vdb.PQIndex(D4, M4, "l2", 0)
    idx.set_option("pq_adc_max_batch", 16)
    idx.set_codebooks(cb)
    cut = 33_000                                             # (not a multiple of 512: the second add continues inside a span and a bin)
    idx.add_codes(codes[:cut], id_base=1000)
    idx.add_codes(codes[cut:], id_base=1000)
    Do, Io = oracle.knn(X, Q[:16], 10, "l2")
    D, I = idx.search(Q[:16], 10)
    assert idx.stats()["last_path_name"] == "pq_adc"
    np.testing.assert_array_equal(I, Io + 1000)
    np.testing.assert_array_equal(D, Do)
    idx.reset()
    idx.add_codes(codes[:36_000])
    Do, Io = oracle.knn(X[:36_000], Q[:5], 10, "l2")
    D, I = idx.search(Q[:5], 10)
    assert idx.stats()["last_path_name"] == "pq_adc" and idx.stats()["ntotal"] == 36_000
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    idx.close()


def test_m256_keeps_the_panel_pass(vdb, oracle):
    assert not ar.admitted(33_000, 256, 256, 5, 4, 16) and ar.admitted(33_000, 256, 128, 5, 4, 16)
    cb, codes, Q = _random_pq(33_000, 256, 256, 9, nq=4)
    idx = _index(vdb, 256, 256, "l2", cb, codes, {"pq_adc_max_batch": 16})
    D, I = idx.search(Q, 5)
    st = idx.stats()
    idx.close()
    assert st["last_path_name"] == "mfma_scan" and st["scan_dtype"] == 2
    Do, Io = oracle.knn(ar.decode(cb, codes), Q, 5, "l2")
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)


# ---- 5. footprint ---------------------------------------------------------------------------------------------------------------
def test_no_slab_of_panels_until_a_large_batch_comes(vdb):
    cb, codes, Q = _random_pq(200_000, 128, 16, 3, nq=600)
    idx = _index(vdb, 128, 16, "l2", cb, codes, {"pq_adc_max_batch": 16})
    slab = cc.PQ_SLAB_ROWS * 128 * 2
    for i in range(3):
        idx.search(Q[i:i + 1], 10)
        st = idx.stats()
        assert st["last_path_name"] == "pq_adc" and st["bytes_workspace"] < slab, st
    small = st["bytes_workspace"]
    print(f"bytes_workspace {small} after single-query ADC searches; the default slab alone is {slab}")
    idx.search(Q, 10)
    st = idx.stats()
    idx.close()
    assert st["last_path_name"] == "mfma_scan" and st["bytes_workspace"] >= small + slab


# ---- 6. admission and refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", list(ac.STATES))
def test_hook_admission(vdb, state):
    """vdb_debug_pq_adc_scores on every kind of handle: only a PQ handle with rows is served; a refusal names the call and the kind
    and leaves the handle as it was (the conventions of admission_cases.run_state)."""
    import ctypes

    import torch
    from vdbhip import _ffi

    lib = _ffi.load()
    s = ac.STATES[state]
    c = ac.ctx(s.d, s.n, s.byte_valued)
    h = ac.build(lib, s, c)
    try:
        want = ac.own_search(lib, s, c, h) if s.search else None
        lib.vdb_device_count(None)                              # leaves SENTINEL in vdb_last_error
        rc = lib.vdb_debug_pq_adc_scores(h, _ffi.ptr(c.Q), ac.NQ, 0, 16, _ffi.ptr(c.floats_out), _ffi.ptr(c.floats_out2),
                                         ctypes.byref(c.cscale))
        torch.cuda.synchronize()
        msg = _ffi.last_error()
        if state == "16_pq_rows":
            assert rc == _ffi.VDB_OK, msg
        else:
            assert rc == (_ffi.VDB_ERR_STATE if state == "15_pq_codebooks" else _ffi.VDB_ERR_UNSUPPORTED), (rc, msg)
            assert msg not in ("", ac.SENTINEL) and "vdb_debug_pq_adc_scores" in msg, msg
            if rc == _ffi.VDB_ERR_UNSUPPORTED:
                assert " is not available on " in msg
        if want is not None:
            assert ac.own_search(lib, s, c, h) == want
    finally:
        lib.vdb_destroy(h)


def test_option_range_and_other_kinds(vdb):
    from vdbhip import _ffi

    lib = _ffi.load()
    cb, codes, _ = _random_pq(2000, 32, 8, 1)
    idx = _index(vdb, 32, 8, "l2", cb, codes)
    for bad in (-1.0, 513.0, 1e9):
        assert lib.vdb_set_option(idx._h, b"pq_adc_max_batch", bad) == _ffi.VDB_ERR_INVALID
    for good in (0.0, 1.0, 512.0):
        assert lib.vdb_set_option(idx._h, b"pq_adc_max_batch", good) == _ffi.VDB_OK
    idx.close()
    flat = vdb.FlatIndex(32, "l2", 0)                           # accepted without effect, as "pq_scan_min_batch" is
    flat.set_option("pq_adc_max_batch", 16)
    X = np.random.default_rng(2).standard_normal((40_000, 32)).astype(F32)
    flat.add(X)
    flat.search(X[:4], 5)
    assert flat.stats()["last_path_name"] == "mfma_scan"
    flat.close()


# ---- 7. plugins -----------------------------------------------------------------------------------------------------------------
def test_searcher_keyword_reaches_the_handle(vdb):
    rng = np.random.default_rng(17)
    X = rng.standard_normal((33_000, 64)).astype(F32)
    Q = rng.standard_normal((6, 64)).astype(F32)

    def make(**searcher):
        algo = vdb.CompositeAlgorithm("pq", 64, indexer={"type": "HipPQIndexer", "metric": "l2", "index_key": "PQ16", "niter": 2,
                                                         "max_points_per_centroid": 16, "reserve_queries": 0},
                                      searcher=dict({"type": "HipPQSearcher", "metric": "l2"}, **searcher), metric="l2")
        algo.build_index(X)
        return algo

    plain, adc = make(), make(adc_max_batch=8)
    for q in Q:
        d0, i0 = plain.search(q, k=10)
        assert plain.searcher.index.stats()["last_path_name"] == "mfma_scan"
        d1, i1 = adc.search(q, k=10)
        assert adc.searcher.index.stats()["last_path_name"] == "pq_adc"
        np.testing.assert_array_equal(i1, i0)
        np.testing.assert_array_equal(d1, d0)
    assert adc.searcher.index.adc_max_batch == 8 and plain.searcher.index.adc_max_batch == 0


def test_algorithm_keyword_survives_save_and_load(vdb, tmp_path):
    rng = np.random.default_rng(18)
    X = rng.standard_normal((33_000, 64)).astype(F32)
    a = vdb.HipPQSearch("a", 64, index_type="PQ16", metric="l2", adc_max_batch=4, niter=2, max_points_per_centroid=16)
    a.build_index(X)
    d0, i0 = a.batch_search(X[:3], 5)
    assert a.index.stats()["last_path_name"] == "pq_adc"
    a.save_index(str(tmp_path / "art"))
    b = vdb.HipPQSearch("b", 64, index_type="PQ16", metric="l2", adc_max_batch=4)
    b.load_index(str(tmp_path / "art"))
    d1, i1 = b.batch_search(X[:3], 5)
    assert b.index.stats()["last_path_name"] == "pq_adc" and b.index.adc_max_batch == 4
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1, d0)
    manifest = json.loads(next((tmp_path / "art").rglob("manifest.json")).read_text())
    assert "adc_max_batch" not in json.dumps(manifest)          # a constructor parameter, not part of the artifact


# ---- 8. allocation balance ------------------------------------------------------------------------------------------------------
def child() -> None:
    """One PQ handle that alternates the two scans (and the hook), resets, re-fills and is destroyed."""
    import vdbhip

    cb, codes, Q = _random_pq(40_000, 64, 16, 5, nq=40)
    idx = vdbhip.PQIndex(64, 16, "l2", 0, adc_max_batch=16)
    idx.set_codebooks(cb)
    idx.add_codes(codes)
    paths = []
    for nq in (1, 40, 16, 40, 2):
        idx.search(Q[:nq], 10)
        paths.append(idx.stats()["last_path_name"])
    idx.debug_adc_scores(Q[:4], 0, 512)
    idx.reset()
    idx.add_codes(codes[:35_000])
    idx.search(Q[:3], 10)
    paths.append(idx.stats()["last_path_name"])
    idx.close()
    print("ADC_ALLOC_REPORT " + json.dumps(paths), flush=True)


def test_every_allocation_is_freed_once(tmp_path):
    from tests.test_gpu_alloc_balance import check_log

    log = tmp_path / "alloc.log"
    env = dict(os.environ, VDBHIP_ALLOC_LOG=str(log))
    code = f"import sys; sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'vectordb-retrieval_amd')!r}]; from tests.test_gpu_pq_adc import child; child()"
    run = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(ROOT), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    tail = [ln for ln in run.stdout.splitlines() if ln.startswith("ADC_ALLOC_REPORT ")]
    assert tail, run.stdout[-4000:]
    assert json.loads(tail[-1].split(" ", 1)[1]) == ["pq_adc", "mfma_scan", "pq_adc", "mfma_scan", "pq_adc", "pq_adc"]
    problems, seen = check_log(log.read_text().splitlines())
    assert seen > 20
    assert not problems, "\n".join(problems[:40])

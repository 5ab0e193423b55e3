"""The lookup-table (ADC) scan of the probed lists of an IVF<nlist>,PQ<M> index (option "ivfpq_adc_max_batch", csrc/ivf_pq_adc.hpp) on
the device.

The contract does not move with the option: ids and distances are, bit for bit, the IVF-Flat search over the decoded rows x^
(oracle.ivf_search).  What is new is checked on its own: the scan's scores against tests/ivfpq_adc_restatement.py bit for bit and
against the bound, every row through a census over lists that end at every boundary, the routing, the fallback, the lifecycle of
the resident norms, both output forms, the plugins and the allocations.  Where a test asserts that no query took the exact list
scan, tests/test_ivfpq_adc_host.py has restated that query's candidate count and held it under the cap."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import ivfpq_adc_cases as ac
from tests import ivfpq_adc_restatement as ir
from tests import ivfpq_cases as cases

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
ID0 = 1000
ADC = {"last_path_name": "ivfpq_adc", "scan_dtype": 3, "last_fallback_queries": 0}


def _index(vdb, d, M, C, cb, metric, **opts):
    idx = vdb.IVFPQIndex(d, len(C), M, metric, 0)
    for name, value in opts.items():
        idx.set_option(name, value)
    idx.set_centroids(C)
    idx.set_codebooks(cb)
    return idx


def _coded(vdb, c, metric, id_base=0, **opts):
    """an index holding the codes of a case under its lists"""
    M = c["cb"].shape[0]
    idx = _index(vdb, c["cb"].shape[2] * M, M, c["C"], c["cb"], metric, **opts)
    idx.add_codes(c["codes"], c["lor"], id_base=id_base)
    return idx


def _stats_are(idx, want):
    st = idx.stats()
    assert {key: st[key] for key in want} == want, st
    return st


# ---- 1. scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d,M", ac.SHAPES)
def test_scores_bit_for_bit_and_within_the_bound(vdb, oracle, d, M, metric):
    c = ac.shape_case(d, M, metric)
    Q = c["Q"][:16]
    idx = _coded(vdb, c, metric)            # (the option is not set: the hook makes the norms itself)
    np.testing.assert_array_equal(idx.reconstruct(), c["Xhat"])
    b = ir.Batch(c["Xhat"], c["C"], c["cb"], c["codes"], c["lor"], Q, metric)
    sizes = np.bincount(c["lor"], minlength=cases.PARITY_LISTS)
    for l in (int(np.argmax(sizes)), int(np.argmin(np.where(sizes > 0, sizes, 1 << 30))), 3):
        rows = np.flatnonzero(c["lor"] == l)              # id order inside a list = list order
        n = len(rows)
        for row0, nrows in ((0, n), (n // 3, n - n // 3)):
            s, eps, cs = idx.debug_adc_scores(Q, l, row0, nrows)
            assert cs == b.cs
            sel = rows[row0:row0 + nrows]
            want = ir.scores(b.T, c["codes"][sel], b.n2[sel], ir.B_of(Q, c["C"], [l], metric, cs)[:, 0], cs, metric)
            np.testing.assert_array_equal(s.view(np.uint32), want.view(np.uint32))
            np.testing.assert_allclose(eps, b.eps, rtol=1e-6)
            keys = b.keys()[:, sel]
            worst = float((np.abs(s.astype(np.float64) - keys) / eps.astype(np.float64)[:, None]).max())
            print(f"D={d} M={M} {metric} list {l} rows {row0}+{nrows}: worst |score - key| / eps = {worst:.4f}")
            assert worst <= 1.0
    st = idx.stats()
    assert st["ntotal"] == len(c["lor"])
    idx.close()


# ---- 2. search ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d,M", ac.SHAPES)
def test_search_equals_the_oracle_over_decoded_rows(vdb, oracle, d, M, metric):
    c = ac.shape_case(d, M, metric)
    idx = _coded(vdb, c, metric, id_base=ID0, ivfpq_adc_max_batch=512)
    for nprobe in ac.SEARCH_NPROBE:
        idx.set_nprobe(nprobe)
        for k in ac.SEARCH_K:
            Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], c["Q"], k, nprobe, metric, id_base=ID0)
            for nq in ac.SEARCH_NQ:
                D, I = idx.search(c["Q"][:nq], k)
                st = _stats_are(idx, ADC)
                assert st["last_candidates"] >= min(k, 1) * nq
                np.testing.assert_array_equal(I, Io[:nq])
                np.testing.assert_array_equal(D, Do[:nq])
    # duplicated rows (rows 40 .. 59 copy rows 0 .. 19): a query at such a row gets both, the smaller id first
    Xq = np.ascontiguousarray(c["Xhat"][:20])
    idx.set_nprobe(cases.PARITY_LISTS)
    Dd, Id = idx.search(Xq, 2)
    _stats_are(idx, ADC)
    Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], Xq, 2, cases.PARITY_LISTS, metric, id_base=ID0)
    np.testing.assert_array_equal(Id, Io)
    np.testing.assert_array_equal(Dd, Do)
    idx.close()


# ---- 3. routing -----------------------------------------------------------------------------------------------------------------
def test_routing(vdb, oracle):
    d, M, metric = 64, 8, "l2"
    c = ac.shape_case(d, M, metric)
    Q = np.ascontiguousarray(np.concatenate([c["Q"], c["Q"][:1] * F32(1.5)]))          # 513 queries
    idx = _coded(vdb, c, metric, id_base=ID0)
    idx.set_nprobe(4)

    def run(nq, k, path):
        D, I = idx.search(Q[:nq], k)
        st = idx.stats()
        assert st["last_path_name"] == path and st["scan_dtype"] == (3 if path == "ivfpq_adc" else st["scan_dtype"]), st
        Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], Q[:nq], k, 4, metric, id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)

    run(8, 10, "ivf")                                     # the option is 0
    idx.set_option("ivfpq_adc_max_batch", 512)
    run(8, 10, "ivfpq_adc")
    run(512, 10, "ivfpq_adc")
    run(513, 10, "ivf")
    run(8, 1024, "ivfpq_adc")
    run(8, 1025, "ivf")
    idx.set_option("force_path", 1)
    run(8, 10, "ivf")
    idx.set_option("force_path", 0)
    idx.set_option("ivfpq_adc_max_batch", 16)
    run(16, 10, "ivfpq_adc")
    run(17, 10, "ivf")
    idx.set_option("ivfpq_adc_max_batch", 0)
    run(8, 10, "ivf")
    idx.close()


def test_m256_stays_where_it_was(vdb, oracle):
    rng = np.random.default_rng(9)
    d = M = 256
    n, nlist = 3000, 8
    C = (rng.standard_normal((nlist, d)) * 3).astype(F32)
    cb = rng.standard_normal((M, 256, 1)).astype(F32)
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    lor = rng.integers(0, nlist, size=n).astype(np.int32)
    Xh = cases.ref.decode(codes, C, lor, cb)
    Q = (Xh[:6] + rng.standard_normal((6, d))).astype(F32)
    idx = _index(vdb, d, M, C, cb, "l2", ivfpq_adc_max_batch=16)
    idx.add_codes(codes, lor)
    idx.set_nprobe(3)
    D, I = idx.search(Q, 5)
    assert idx.stats()["last_path_name"] == "ivf"
    Do, Io = oracle.ivf_search(Xh, C, lor, Q, 5, 3, "l2")
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    with pytest.raises(Exception, match="does not serve this M"):
        idx.debug_adc_scores(Q, 0, 0, 1)
    idx.close()
    # M = 128 (D = 256): a table of 128 KiB, above what a kernel gets without opting in
    M = 128
    cb = rng.standard_normal((M, 256, 2)).astype(F32)
    codes = np.ascontiguousarray(codes[:, :M])
    Xh = cases.ref.decode(codes, C, lor, cb)
    idx = _index(vdb, d, M, C, cb, "l2", ivfpq_adc_max_batch=16)
    idx.add_codes(codes, lor)
    idx.set_nprobe(3)
    D, I = idx.search(Q, 5)
    _stats_are(idx, ADC)
    Do, Io = oracle.ivf_search(Xh, C, lor, Q, 5, 3, "l2")
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    idx.close()


def test_options_on_other_kinds_and_their_ranges(vdb):
    from vdbhip import _ffi

    lib = _ffi.load()
    flat = vdb.FlatIndex(32, "l2", 0)
    for name, good, bad in ((b"ivfpq_adc_max_batch", (0.0, 1.0, 512.0), (-1.0, 513.0)),
                            (b"ivfpq_adc_part_rows", (0.0, 256.0, 65536.0), (-256.0, 100.0, 255.0, 65792.0))):
        for v in bad:
            assert lib.vdb_set_option(flat._h, name, v) == _ffi.VDB_ERR_INVALID, (name, v)
        for v in good:
            assert lib.vdb_set_option(flat._h, name, v) == _ffi.VDB_OK, (name, v)
    flat.set_option("ivfpq_adc_max_batch", 16)            # accepted without effect
    X = np.random.default_rng(2).standard_normal((40_000, 32)).astype(F32)
    flat.add(X)
    flat.search(X[:4], 5)
    assert flat.stats()["last_path_name"] == "mfma_scan"
    rc = lib.vdb_debug_ivfpq_adc_scores(flat._h, _ffi.ptr(X), 1, 0, 0, 1, _ffi.ptr(np.zeros(4, F32)), _ffi.ptr(np.zeros(4, F32)), None)
    assert rc == _ffi.VDB_ERR_UNSUPPORTED and "vdb_debug_ivfpq_adc_scores is not available on a flat index" in _ffi.last_error()
    flat.close()


# ---- 4. census ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_census_every_row_at_every_boundary(vdb, oracle, metric):
    """Every decoded row is a query (k = 2), 500 per call, every list probed; lists of 0, 1, 255, 256, 257, 511, 513 and 1900 rows,
    row parts of 256 rows and the scan's own: a row skipped at the end of a part or a list is missing from its own result, a row
    scored twice appears in it twice."""
    c = ac.census_case(metric)
    nlist = len(ac.CENSUS_LISTS)
    idx = _index(vdb, c["d"], c["M"], c["C"], c["cb"], metric, ivfpq_adc_max_batch=512)
    idx.add(c["X"], list_of_row=c["lor"])                 # (vdb_ivf_add_assigned: the lists are the case's)
    np.testing.assert_array_equal(idx.codes(), c["codes"])
    assert list(np.bincount(idx.assignment(), minlength=nlist)) == list(ac.CENSUS_LISTS)
    idx.set_nprobe(nlist)
    n = len(c["lor"])
    Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], c["Xhat"], 2, nlist, metric)
    for part in (256, 0):
        idx.set_option("ivfpq_adc_part_rows", part)
        for q0 in range(0, n, 500):
            D, I = idx.search(c["Xhat"][q0:q0 + 500], 2)
            _stats_are(idx, ADC)
            np.testing.assert_array_equal(I, Io[q0:q0 + 500])
            np.testing.assert_array_equal(D, Do[q0:q0 + 500])
    idx.close()


# ---- 5. near ties, fallback, padding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties(vdb, oracle, metric):
    t = cases.near_tie_inputs(metric)
    idx = _index(vdb, cases.NEAR_TIE_D, cases.NEAR_TIE_M, t["C"], t["cb"], metric, ivfpq_adc_max_batch=512)
    idx.add_codes(t["codes"], t["lor"])
    idx.set_nprobe(4)
    D, I = idx.search(t["Q"], t["k"])
    st = _stats_are(idx, ADC)
    assert st["last_candidates"] > t["k"] * len(t["Q"])              # the replicas are within the bound of one another
    Do, Io = oracle.ivf_search(t["Xhat"], t["C"], t["lor"], t["Q"], t["k"], 4, metric)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    idx.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fallback_and_padding(vdb, oracle, metric):
    d, M = 128, 64
    c = ac.shape_case(d, M, metric)
    idx = _coded(vdb, c, metric, id_base=ID0, ivfpq_adc_max_batch=512, list_cap=1)
    nlist = cases.PARITY_LISTS
    idx.set_nprobe(nlist)
    Xq = np.ascontiguousarray(c["Xhat"][:20])             # rows 40 .. 59 copy rows 0 .. 19: two candidates at least, the cap is one
    D, I = idx.search(Xq, 2)
    st = idx.stats()
    assert st["last_path_name"] == "ivfpq_adc" and st["last_fallback_queries"] > 0, st
    Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], Xq, 2, nlist, metric, id_base=ID0)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    if metric == "l2":
        same = np.array([np.array_equal(c["Xhat"][i], c["Xhat"][40 + i]) for i in range(20)])
        assert same.any()
        assert (I[same, 0] == ID0 + np.flatnonzero(same)).all() and (I[same, 1] == ID0 + 40 + np.flatnonzero(same)).all()
    D, I = idx.search(c["Q"][:40], 10)
    assert idx.stats()["last_fallback_queries"] == 40     # ten candidates at least
    Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], c["Q"][:40], 10, nlist, metric, id_base=ID0)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    # fewer probed rows than k: -1 / +-FLT_MAX padding, as the oracle pads
    idx.set_option("list_cap", 0)
    idx.set_nprobe(1)
    sizes = np.bincount(c["lor"], minlength=nlist)
    k = int(sizes.max()) + 5
    assert k <= 1024
    D, I = idx.search(c["Q"][:9], k)
    _stats_are(idx, {"last_path_name": "ivfpq_adc", "scan_dtype": 3})
    Do, Io = oracle.ivf_search(c["Xhat"], c["C"], c["lor"], c["Q"][:9], k, 1, metric, id_base=ID0)
    assert (Io == -1).any()
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    # a NaN query and a zero query: whatever the option-0 path returns
    Qn = c["Q"][:4].copy()
    Qn[1, 5] = np.nan
    Qn[2] = 0.0
    idx.set_nprobe(4)
    D1, I1 = idx.search(Qn, 10)
    assert idx.stats()["last_path_name"] == "ivfpq_adc" and idx.stats()["last_fallback_queries"] >= 1
    idx.set_option("ivfpq_adc_max_batch", 0)
    D0, I0 = idx.search(Qn, 10)
    assert idx.stats()["last_path_name"] == "ivf"
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1.view(np.uint32), D0.view(np.uint32))
    idx.close()


# ---- 6. value families ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("kind", [kind for kind in ac.KINDS if kind != "gauss"])
def test_value_families_equal_the_oracle(vdb, oracle, kind, metric):
    """tiny (1e-20) and huge (1e18) handles lie outside the admitted range and keep their path; the others take the ADC scan, and the
    unit family (like the Gaussian search cases) may not use the fallback.  Query 1 of every family is a thousandth of the others."""
    f = ac.family(kind, 16)
    idx = _coded(vdb, f, metric, ivfpq_adc_max_batch=512)
    idx.set_nprobe(4)
    D, I = idx.search(f["Q"], 10)
    st = idx.stats()
    refused = kind in ("tiny", "huge")
    assert st["last_path_name"] == ("ivf" if refused else "ivfpq_adc"), st
    if kind == "unit":
        assert st["last_fallback_queries"] == 0
    print(f"{kind} {metric}: path {st['last_path_name']}, fallback queries {st['last_fallback_queries']}, rows re-scored {st['last_candidates']}")
    Do, Io = oracle.ivf_search(f["Xhat"], f["C"], f["lor"], f["Q"], 10, 4, metric)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    idx.close()


# ---- 7. lifecycle of the norms, footprint ---------------------------------------------------------------------------------------
def test_lifecycle_and_footprint(vdb, oracle):
    d, M, metric = 64, 8, "l2"
    c = ac.shape_case(d, M, metric)
    X, Q, C, cb, lor, Xh = c["X"], c["Q"][:8], c["C"], c["cb"], c["lor"], c["Xhat"]
    n = len(X)
    idx = _index(vdb, d, M, C, cb, metric)
    idx.set_nprobe(5)

    def index_bytes():
        st = idx.stats()
        return st["bytes_resident"] - st["bytes_workspace"]

    def check(rows, id_base=ID0):
        D, I = idx.search(Q, 10)
        Do, Io = oracle.ivf_search(Xh[:rows], C, lor[:rows], Q, 10, 5, metric, id_base=id_base)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)

    idx.add(X[:2500], id_base=ID0)
    idx.add(X[2500:], id_base=ID0)                         # a split add
    check(n)
    base = index_bytes()                                   # (after a search: the coarse result and the plan buffers of 8 queries are held)
    check(n)
    assert idx.stats()["last_path_name"] == "ivf" and index_bytes() == base        # option off: no norms, ever
    idx.set_option("ivfpq_adc_max_batch", 16)
    assert index_bytes() == base                           # ... nor before the first admitted batch
    check(n)
    _stats_are(idx, ADC)
    assert index_bytes() == base + 4 * n                   # the norms: 4 N bytes
    check(n)
    assert index_bytes() == base + 4 * n
    # reset, then codes: the norms are dropped with the rows and made anew for the new ones
    idx.reset()
    idx.add_codes(c["codes"][:3000], lor[:3000], id_base=ID0)
    before = index_bytes()
    check(3000)
    _stats_are(idx, ADC)
    assert index_bytes() == before + 4 * 3000
    idx.add_codes(c["codes"][3000:], lor[3000:], id_base=ID0)      # an append: other rows in every list, the norms go
    before = index_bytes()
    check(n)
    _stats_are(idx, ADC)
    assert index_bytes() == before + 4 * n
    # new codebooks, new centroids: the rows go at the next add, the norms at once
    cb2 = np.ascontiguousarray(cb[:, ::-1])
    idx.set_codebooks(cb2)
    idx.add(X, id_base=7)
    codes2 = idx.codes()
    Xh2 = cases.ref.decode(codes2, C, lor, cb2)
    D, I = idx.search(Q, 10)
    _stats_are(idx, ADC)
    Do, Io = oracle.ivf_search(Xh2, C, lor, Q, 10, 5, metric, id_base=7)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    C2 = np.ascontiguousarray(C[::-1])
    idx.set_centroids(C2)
    idx.add(X, id_base=7)
    lor2 = idx.assignment()
    Xh3 = cases.ref.decode(idx.codes(), C2, lor2, cb2)
    D, I = idx.search(Q, 10)
    _stats_are(idx, ADC)
    Do, Io = oracle.ivf_search(Xh3, C2, lor2, Q, 10, 5, metric, id_base=7)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    idx.close()


def test_one_query_reserves_no_panels(vdb):
    """D <= 128: the list-major path makes fp16 panels of the whole index per batch (ws.sq8_panels); an ADC batch does not."""
    rng = np.random.default_rng(4)
    n, d, M, nlist = 200_000, 128, 16, 64
    C = (rng.standard_normal((nlist, d)) * 3).astype(F32)
    cb = rng.standard_normal((M, 256, d // M)).astype(F32)
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    lor = rng.integers(0, nlist, size=n).astype(np.int32)
    Q = (C[:3] + rng.standard_normal((3, d))).astype(F32)
    idx = _index(vdb, d, M, C, cb, "l2", ivfpq_adc_max_batch=16)
    idx.add_codes(codes, lor)
    idx.set_nprobe(8)
    panels = n * d * 2
    for i in range(3):
        idx.search(Q[i:i + 1], 10)
        st = idx.stats()
        assert st["last_path_name"] == "ivfpq_adc" and st["bytes_workspace"] < panels // 4, st
    small = st["bytes_workspace"]
    D1, I1 = idx.search(Q[:1], 10)
    idx.set_option("ivfpq_adc_max_batch", 0)
    D0, I0 = idx.search(Q[:1], 10)
    st = idx.stats()
    assert st["last_path_name"] == "ivf" and st["scan_dtype"] == 2 and st["bytes_workspace"] >= small + panels
    print(f"bytes_workspace {small} after one-query ADC searches, {st['bytes_workspace']} after one on the panel pass")
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1, D0)
    idx.close()


# ---- 8. the partial device entry point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_partial_device_search_equals_the_full_search(vdb, metric):
    import torch

    d, M = 384, 64
    c = ac.shape_case(d, M, metric)
    idx = _coded(vdb, c, metric, id_base=ID0, ivfpq_adc_max_batch=512)
    idx.set_nprobe(4)
    for nq, k in ((1, 10), (9, 100), (40, 1)):
        Q = c["Q"][:nq]
        D, I = idx.search(Q, k)
        _stats_are(idx, ADC)
        q = torch.from_numpy(np.array(Q, dtype=F32, order="C")).cuda()
        keys = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        Dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        Id = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        idx.search_partial_device(q.data_ptr(), nq, k, keys.data_ptr(), ids.data_ptr())
        torch.cuda.synchronize()
        _stats_are(idx, ADC)
        idx.search_device(q.data_ptr(), nq, k, Dd.data_ptr(), Id.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ids.cpu().numpy(), I)
        np.testing.assert_array_equal(Id.cpu().numpy(), I)
        np.testing.assert_array_equal(Dd.cpu().numpy(), D)
        kk = keys.cpu().numpy()
        np.testing.assert_array_equal((kk if metric == "l2" else -kk).astype(F32), D)
    idx.close()


# ---- 9. plugins -----------------------------------------------------------------------------------------------------------------
def test_plugins_take_the_keyword(vdb, tmp_path):
    X, Q, _, _ = cases.parity_inputs(64, 8)

    def make(indexer=None, searcher=None):
        algo = vdb.CompositeAlgorithm("ivf_pq", 64,
                                      indexer=dict({"type": "HipIVFPQIndexer", "metric": "l2", "index_key": "IVF32,PQ16", "nprobe": 4, "niter": 3},
                                                   **(indexer or {})),
                                      searcher=dict({"type": "HipIVFSearcher", "metric": "l2"}, **(searcher or {})), metric="l2")
        algo.build_index(X)
        return algo

    plain, by_indexer, by_searcher = make(), make(indexer={"adc_max_batch": 8}), make(searcher={"adc_max_batch": 8})
    for q in Q[:4]:
        d0, i0 = plain.search(q, k=10)
        assert plain.searcher.index.stats()["last_path_name"] == "ivf"
        for algo in (by_indexer, by_searcher):
            d1, i1 = algo.search(q, k=10)
            assert algo.searcher.index.stats()["last_path_name"] == "ivfpq_adc"
            np.testing.assert_array_equal(i1, i0)
            np.testing.assert_array_equal(d1, d0)
    assert by_indexer.searcher.index.adc_max_batch == 8 and by_searcher.searcher.index.adc_max_batch == 8 and plain.searcher.index.adc_max_batch == 0
    D0, I0 = plain.batch_search(Q[:9], k=10)               # nine queries: beyond the option
    D1, I1 = by_searcher.batch_search(Q[:9], k=10)
    assert by_searcher.searcher.index.stats()["last_path_name"] == "ivf"
    np.testing.assert_array_equal(I1, I0)
    for algo in (plain, by_indexer, by_searcher):
        algo.searcher.index.close()
    a = vdb.HipIVFPQSearch("a", 64, index_type="IVF32,PQ16", metric="l2", nprobe=5, niter=3, adc_max_batch=4)
    a.build_index(X)
    d0, i0 = a.batch_search(Q[:3], 5)
    assert a.index.stats()["last_path_name"] == "ivfpq_adc"
    a.save_index(str(tmp_path / "art"))
    b = vdb.HipIVFPQSearch("b", 64, index_type="IVF32,PQ16", metric="l2", nprobe=5, adc_max_batch=4)
    b.load_index(str(tmp_path / "art"))
    d1, i1 = b.batch_search(Q[:3], 5)
    assert b.index.stats()["last_path_name"] == "ivfpq_adc" and b.index.adc_max_batch == 4
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1, d0)
    manifest = json.loads(next((tmp_path / "art").rglob("manifest.json")).read_text())
    assert "adc_max_batch" not in json.dumps(manifest)      # a constructor parameter, not part of the artifact
    a.index.close()
    b.index.close()


# ---- 10. allocation balance -----------------------------------------------------------------------------------------------------
def child() -> None:
    """One IVF-PQ handle that alternates the paths (and the hook), resets, re-fills and is destroyed."""
    import vdbhip

    c = ac.shape_case(64, 8, "l2")
    idx = vdbhip.IVFPQIndex(64, cases.PARITY_LISTS, 8, "l2", 0, adc_max_batch=16)
    idx.set_centroids(c["C"])
    idx.set_codebooks(c["cb"])
    idx.add_codes(c["codes"], c["lor"])
    idx.set_nprobe(4)
    paths = []
    for nq in (1, 40, 16, 40, 2):
        idx.search(c["Q"][:nq], 10)
        paths.append(idx.stats()["last_path_name"])
    idx.debug_adc_scores(c["Q"][:4], 3, 0, 5)
    idx.reset()
    idx.add_codes(c["codes"][:3500], c["lor"][:3500])
    idx.search(c["Q"][:3], 10)
    paths.append(idx.stats()["last_path_name"])
    idx.close()
    print("ADC_ALLOC_REPORT " + json.dumps(paths), flush=True)


def test_every_allocation_is_freed_once(tmp_path):
    from tests.test_gpu_alloc_balance import check_log

    log = tmp_path / "alloc.log"
    env = dict(os.environ, VDBHIP_ALLOC_LOG=str(log))
    code = f"import sys; sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'vectordb-retrieval_amd')!r}]; from tests.test_gpu_ivfpq_adc import child; child()"
    run = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(ROOT), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    tail = [ln for ln in run.stdout.splitlines() if ln.startswith("ADC_ALLOC_REPORT ")]
    assert tail, run.stdout[-4000:]
    assert json.loads(tail[-1].split(" ", 1)[1]) == ["ivfpq_adc", "ivf", "ivfpq_adc", "ivf", "ivfpq_adc", "ivfpq_adc"]
    problems, seen = check_log(log.read_text().splitlines())
    assert seen > 20
    assert not problems, "\n".join(problems[:40])

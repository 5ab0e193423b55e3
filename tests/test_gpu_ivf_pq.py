"""IVF<nlist>,PQ<M> on the GPU against the NumPy restatement of the codec (tests/ivfpq_restatement.py) and the IVF oracle over the
decoded rows.

The contract (include/vdbhip.h): codes equal the restatement bit for bit, and a search equals oracle.ivf_search over the decoded
rows x^ (same centroids, same lists, same nprobe) bit for bit in ids and distances, ties by the smaller id.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import ivfpq_cases as cases  # noqa: E402
import ivfpq_restatement as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
ID0 = 1000


def _index(vdb, d, M, C, cb, metric):
    idx = vdb.IVFPQIndex(d, len(C), M, metric, 0)
    idx.set_centroids(C)
    idx.set_codebooks(cb)
    return idx


_parity = {}


def _parity_case(vdb, oracle, d, M, metric):
    """index + the restatement's codes and decoded rows, computed once per (d, M, metric) and shared by the tests below"""
    key = (d, M, metric)
    if key not in _parity:
        X, Q, C, cb = cases.parity_inputs(d, M)
        idx = _index(vdb, d, M, C, cb, metric)
        idx.add(X, id_base=ID0)
        lor = oracle.ivf_assign(C, X, metric)
        codes = ref.encode(X, C, lor, cb)
        _parity[key] = (idx, lor, codes, ref.decode(codes, C, lor, cb))
    return _parity[key]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d,M", cases.PARITY_SHAPES)
def test_codes_bit_equal_to_the_restatement(vdb, oracle, d, M, metric):
    X, _, C, cb = cases.parity_inputs(d, M)
    idx, lor, codes, Xh = _parity_case(vdb, oracle, d, M, metric)
    np.testing.assert_array_equal(idx.assignment(), lor)
    got = idx.codes()
    assert got.dtype == np.uint8 and got.shape == (len(X), M)
    np.testing.assert_array_equal(got, codes)
    assert not (got == 200).any()                               # (entry 200 equals entry 17: the smaller c keeps the tie)
    np.testing.assert_array_equal(idx.reconstruct(), Xh)
    np.testing.assert_array_equal(idx.codebooks(), cb)
    st = idx.stats()
    assert st["ntotal"] == len(X) and st["nlist"] == cases.PARITY_LISTS


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d,M", cases.PARITY_SHAPES)
def test_search_equals_the_oracle_over_decoded_rows(vdb, oracle, d, M, metric):
    _, Q, C, _ = cases.parity_inputs(d, M)
    idx, lor, _, Xh = _parity_case(vdb, oracle, d, M, metric)
    nlist = len(C)
    idx.set_option("force_path", 0)
    idx.set_option("list_cap", 0)

    def check(nq, k, nprobe):
        idx.set_nprobe(nprobe)
        D, I = idx.search(Q[:nq], k)
        Do, Io = oracle.ivf_search(Xh, C, lor, Q[:nq], k, nprobe, metric, id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
        return D, I

    for nprobe in (1, 4, nlist):
        for k in (1, 10, 100):
            for nq in (1, 8, 300):
                check(nq, k, nprobe)
    # the large batch, every list probed: D <= 128 takes the list-major MFMA scan on panels made from the codes
    D, I = check(300, 10, nlist)
    st = idx.stats()
    assert st["last_path_name"] == "ivf", st
    if d <= 128:
        assert st["scan_dtype"] == 2 and st["last_candidates"] > 0, st
        idx.set_option("list_cap", 1)                           # a work list of one row: the queries that nominate more overflow
        D2, I2 = idx.search(Q[:300], 10)                        # into the tail's exact list scan over the codes
        assert idx.stats()["last_fallback_queries"] > 0
        idx.set_option("list_cap", 0)
        np.testing.assert_array_equal(I2, I)
        np.testing.assert_array_equal(D2, D)
    else:
        assert st["scan_dtype"] == 0 and st["last_candidates"] == 0, st      # D > 128: the exact list scan over the codes
    idx.set_option("force_path", 1)                             # the exact list scan: the same result
    D1, I1 = idx.search(Q[:300], 10)
    assert idx.stats()["last_candidates"] == 0
    idx.set_option("force_path", 0)
    np.testing.assert_array_equal(I1, I)
    np.testing.assert_array_equal(D1, D)
    # duplicated rows (rows 40 .. 59 copy rows 0 .. 19): a query at such a row gets both, the smaller id first
    Xq = np.ascontiguousarray(Xh[:20])
    idx.set_nprobe(nlist)
    Dd, Id = idx.search(Xq, 2)
    Do, Io = oracle.ivf_search(Xh, C, lor, Xq, 2, nlist, metric, id_base=ID0)
    np.testing.assert_array_equal(Id, Io)
    np.testing.assert_array_equal(Dd, Do)
    if metric == "l2":
        same = np.array([np.array_equal(Xh[i], Xh[40 + i]) for i in range(20)])
        assert same.any()
        assert (Id[same, 0] == ID0 + np.flatnonzero(same)).all() and (Id[same, 1] == ID0 + 40 + np.flatnonzero(same)).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_encode_with_the_codebook_read_from_global_memory(vdb, oracle, metric):
    """D = 128, M = 2: a sub-space of 256 x 64 floats (64 KiB) does not fit the 48 KiB of LDS pq_encode_kernel may use, so the
    residual encoder reads the codebook from global memory.  600 rows of parity_inputs in 4 lists; 8 rows per list are moved
    next to centroid + entry 17 of both sub-spaces, so that entry 17 and its copy, entry 200, tie for the minimum (asserted on
    the restatement before any GPU call).  The limit of the census corpora of this shape (tests/census_coded.py: L2 only, their
    rows must be their own nearest neighbours) does not apply: the reference here is the IVF oracle over the decoded rows,
    which serves both metrics."""
    d, M, n, nlist = 128, 2, 600, 4
    X, Q, C, cb = cases.parity_inputs(d, M)
    X, Q, C = X[:n].copy(), Q[:8], np.ascontiguousarray(C[:nlist])
    entry17 = np.concatenate([cb[0, 17], cb[1, 17]])
    for l in range(nlist):
        X[100 + 8 * l:108 + 8 * l] = C[l] + entry17 + (0.01 * np.random.default_rng(l).standard_normal((8, d))).astype(F32)
    lor = oracle.ivf_assign(C, X, metric)
    codes = ref.encode(X, C, lor, cb)
    assert ((codes == 17).sum(axis=0) >= 8).all() and not (codes == 200).any()
    Xh = ref.decode(codes, C, lor, cb)
    idx = _index(vdb, d, M, C, cb, metric)
    try:
        idx.add(X, id_base=ID0)
        np.testing.assert_array_equal(idx.assignment(), lor)
        np.testing.assert_array_equal(idx.codes(), codes)
        np.testing.assert_array_equal(idx.reconstruct(), Xh)
        idx.set_nprobe(2)
        D, I = idx.search(Q, 10)
        Do, Io = oracle.ivf_search(Xh, C, lor, Q, 10, 2, metric, id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
    finally:
        idx.close()


def test_parity_indexes_are_closed():
    for idx, *_ in _parity.values():
        idx.close()
    _parity.clear()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties_through_the_mfma_list_scan(vdb, oracle, metric):
    """Replicas that differ by one codebook entry per sub-space (below the fp16 resolution of the scan) and exact duplicates,
    every list probed: tests/test_ivf_pq_host.py holds the share of queries an unguarded scan gets wrong to guard_cases.FLOOR.
    As in the IVF-SQ8 near-tie cases no query may take the fallback."""
    t = cases.near_tie_inputs(metric)
    idx = _index(vdb, cases.NEAR_TIE_D, cases.NEAR_TIE_M, t["C"], t["cb"], metric)
    try:
        idx.add_codes(t["codes"], t["lor"])
        np.testing.assert_array_equal(idx.reconstruct(), t["Xhat"])
        idx.set_nprobe(4)
        D, I = idx.search(t["Q"], t["k"])
        st = idx.stats()
        Do, Io = oracle.ivf_search(t["Xhat"], t["C"], t["lor"], t["Q"], t["k"], 4, metric)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
        assert st["last_path_name"] == "ivf" and st["scan_dtype"] == 2 and st["last_candidates"] > 0, st
        assert st["last_fallback_queries"] == 0, st
        # the queries at duplicated rows return the two copies in id order
        dup = [r for r in range(32) if {r, cases.NEAR_TIE_NB + r} <= set(Io[r].tolist())]
        assert len(dup) >= 16
        for r in dup:
            row = I[r].tolist()
            assert row.index(r) + 1 == row.index(cases.NEAR_TIE_NB + r)
    finally:
        idx.close()


def test_adds_give_the_index_one_add_gives(vdb, oracle):
    d, M = 64, 8
    X, Q, C, cb = cases.parity_inputs(d, M)
    one = _index(vdb, d, M, C, cb, "l2")
    one.add(X, id_base=ID0)
    codes, lor = one.codes(), one.assignment()
    one.set_nprobe(6)
    D0, I0 = one.search(Q, 10)

    def same(idx):
        np.testing.assert_array_equal(idx.codes(), codes)
        np.testing.assert_array_equal(idx.assignment(), lor)
        idx.set_nprobe(6)
        D, I = idx.search(Q, 10)
        np.testing.assert_array_equal(I, I0)
        np.testing.assert_array_equal(D, D0)

    split = _index(vdb, d, M, C, cb, "l2")
    split.add(X[:2500], id_base=ID0)
    split.add(X[2500:2500], id_base=ID0)                        # an empty append
    split.add(X[2500:], id_base=ID0)
    same(split)
    given = _index(vdb, d, M, C, cb, "l2")
    given.add(X[:3000], id_base=ID0, list_of_row=lor[:3000])
    given.add(X[3000:], id_base=ID0, list_of_row=lor[3000:])
    same(given)
    loaded = _index(vdb, d, M, C, cb, "l2")
    loaded.add_codes(codes[:1000], lor[:1000], id_base=ID0)
    loaded.add_codes(codes[1000:], lor[1000:], id_base=ID0)
    same(loaded)
    loaded.reserve(200, 10)
    same(loaded)
    # refused appends leave the index as it was
    with pytest.raises(ValueError, match="id_base"):
        loaded.add(X[:10], id_base=5)
    with pytest.raises(ValueError, match="id_base"):
        loaded.add_codes(codes[:10], lor[:10], id_base=5)
    bad = lor[:10].copy()
    bad[3] = len(C)
    with pytest.raises(ValueError, match="row could not be assigned to a list"):
        loaded.add_codes(codes[:10], bad, id_base=ID0)
    with pytest.raises(ValueError, match="row could not be assigned to a list"):
        loaded.add(X[:10], id_base=ID0, list_of_row=bad)
    with pytest.raises(ValueError, match=r"expected \(n, 8\) codes"):
        loaded.add_codes(np.zeros((10, 16), np.uint8), lor[:10], id_base=ID0)
    with pytest.raises(ValueError, match="list ids"):
        loaded.add_codes(codes[:10], lor[:9], id_base=ID0)
    assert loaded.ntotal == len(X)
    same(loaded)
    # reset keeps centroids and codebooks
    loaded.reset()
    assert loaded.stats()["ntotal"] == 0
    np.testing.assert_array_equal(loaded.codebooks(), cb)
    np.testing.assert_array_equal(loaded.centroids(), C)
    loaded.add(X, id_base=ID0)
    same(loaded)
    # new codebooks drop the rows encoded under the old ones at the next add
    loaded.set_codebooks(cb[:, ::-1].copy())
    loaded.add(X[:500], id_base=7)
    assert loaded.stats()["ntotal"] == 500
    for h in (one, split, given, loaded):
        h.close()


def test_training_is_deterministic_and_lowers_the_reconstruction_error(vdb, oracle):
    d, M, nlist = 64, 16, 16
    X, _, _, _ = cases.parity_inputs(64, 8)
    C = np.ascontiguousarray(X[:nlist])
    lor = oracle.ivf_assign(C, X, "l2")

    def trained(niter, seed):
        idx = vdb.IVFPQIndex(d, nlist, M, "l2", 0)
        idx.set_centroids(C)
        idx.train_codebooks(X, niter=niter, seed=seed)
        cb = idx.codebooks()
        idx.add(X)
        np.testing.assert_array_equal(idx.assignment(), lor)
        np.testing.assert_array_equal(idx.codes(), ref.encode(X, C, lor, cb))
        err = float(np.mean((X.astype(np.float64) - idx.reconstruct().astype(np.float64)) ** 2))
        idx.close()
        return cb, err

    cb_a, err_a = trained(10, 3)
    cb_b, _ = trained(10, 3)
    cb_c, _ = trained(10, 4)
    np.testing.assert_array_equal(cb_a, cb_b)
    assert not np.array_equal(cb_a, cb_c)
    cb_0, err_0 = trained(0, 3)                                 # no iterations: the codebooks are rows of the residual sample
    R = ref.residual(X, C, lor)
    for m in (0, M - 1):
        sub = {tuple(v) for v in R[:, m * 4:(m + 1) * 4].tolist()}
        assert all(tuple(v) in sub for v in cb_0[m].tolist())
    print(f"mean squared reconstruction error: sample rows as codebooks {err_0:.5f}, 10 iterations {err_a:.5f}")
    assert err_a < err_0
    few = vdb.IVFPQIndex(d, nlist, M, "l2", 0)
    few.set_centroids(C)
    with pytest.raises(ValueError, match="256"):
        few.train_codebooks(X[:255])
    few.close()


def test_persistence_round_trip(vdb, tmp_path):
    X, Q, _, _ = cases.parity_inputs(64, 8)
    algo = vdb.HipIVFPQSearch("p", 64, index_type="IVF32,PQ16", metric="l2", nprobe=5, niter=4)
    algo.build_index(X)
    D, I = algo.batch_search(Q, 10)
    algo.save_index(str(tmp_path / "a"))
    man = json.loads((tmp_path / "a" / "manifest.json").read_text())
    assert man["format"] == "vdbhip-ivfpq-v1" and man["M"] == 16 and man["nlist"] == 32 and man["n_vectors"] == len(X)
    assert sorted(man["files"]) == ["centroids", "codebooks", "codes", "list_of_row"]
    back = vdb.HipIVFPQSearch("p", 64, index_type="IVF32,PQ16", metric="l2", nprobe=5)
    back.load_index(str(tmp_path / "a"))
    np.testing.assert_array_equal(back.index.codes(), algo.index.codes())
    np.testing.assert_array_equal(back.index.codebooks(), algo.index.codebooks())
    np.testing.assert_array_equal(back.index.assignment(), algo.index.assignment())
    D2, I2 = back.batch_search(Q, 10)
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    with pytest.raises(FileExistsError):
        algo.save_index(str(tmp_path / "a"))
    # mismatching instances and incomplete or altered artifacts are refused
    with pytest.raises(ValueError, match="index_type"):
        vdb.HipIVFPQSearch("p", 64, index_type="IVF32,PQ8", metric="l2").load_index(str(tmp_path / "a"))
    with pytest.raises(ValueError, match="metric"):
        vdb.HipIVFPQSearch("p", 64, index_type="IVF32,PQ16", metric="ip").load_index(str(tmp_path / "a"))
    with pytest.raises(ValueError, match="format"):
        vdb.HipApproximateSearch("f", 64, index_type="IVF32,Flat", metric="l2").load_index(str(tmp_path / "a"))
    algo.save_index(str(tmp_path / "b"))
    codes = np.load(tmp_path / "b" / "codes.npy")
    codes[0, 0] ^= 1
    np.save(tmp_path / "b" / "codes.npy", codes, allow_pickle=False)
    with pytest.raises(ValueError, match="fingerprint mismatch: codes"):
        vdb.HipIVFPQSearch("p", 64, index_type="IVF32,PQ16", metric="l2").load_index(str(tmp_path / "b"))
    np.save(tmp_path / "b" / "codes.npy", codes[:-1], allow_pickle=False)
    with pytest.raises(ValueError, match="do not match the manifest"):
        vdb.HipIVFPQSearch("p", 64, index_type="IVF32,PQ16", metric="l2").load_index(str(tmp_path / "b"))
    (tmp_path / "a" / "WRITE_COMPLETE").unlink()
    with pytest.raises(FileNotFoundError, match="WRITE_COMPLETE"):
        back.load_index(str(tmp_path / "a"))
    algo.index.close()
    back.index.close()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_plugins_reference_yaml_shape(vdb, metric):
    from vdbhip.algorithms import _safe_normalize

    X, Q, _, _ = cases.parity_inputs(64, 8)
    algo = vdb.CompositeAlgorithm("ivf_pq", 64,
                                  indexer={"type": "HipIVFPQIndexer", "metric": metric, "index_key": "IVF32,PQ16", "nprobe": 4, "niter": 4},
                                  searcher={"type": "HipIVFSearcher", "metric": metric, "nprobe": 8}, metric=metric)
    algo.build_index(X)
    D, I = algo.batch_search(Q[:60], k=10)
    assert algo.searcher.index.nprobe == 8 and isinstance(algo.searcher.index, vdb.IVFPQIndex)
    cos = metric == "cosine"
    ref_idx = vdb.IVFPQIndex(64, 32, 16, "ip" if cos else "l2", 0)
    ref_idx.train(_safe_normalize(X) if cos else X, niter=4)
    ref_idx.add(_safe_normalize(X) if cos else X)
    ref_idx.set_nprobe(8)
    Dr, Ir = ref_idx.search(_safe_normalize(Q[:60]) if cos else Q[:60], 10)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, -Dr if cos else Dr)
    assert algo.get_memory_usage() > 0
    ref_idx.close()
    algo.searcher.index.close()


def test_refusals(vdb):
    from vdbhip import _ffi

    lib = _ffi.load()
    X, Q, C, cb = cases.parity_inputs(64, 8)
    UNSUP, STATE, INVALID = _ffi.VDB_ERR_UNSUPPORTED, _ffi.VDB_ERR_STATE, _ffi.VDB_ERR_INVALID

    def refused(status, code, *words):
        assert status == code, (status, _ffi.last_error())
        for w in words:
            assert w in _ffi.last_error(), _ffi.last_error()

    idx = vdb.IVFPQIndex(64, len(C), 8, "l2", 0)
    h = idx._h
    refused(lib.vdb_ivfpq_train(h, 8, _ffi.ptr(X), len(X), 2, 0, 0), STATE, "no centroids")
    idx.set_centroids(C)
    refused(lib.vdb_ivf_add(h, _ffi.ptr(X), 10, 0), STATE, "IVF-PQ codebooks")               # an add before codebooks
    for m in (0, 7, 65):
        refused(lib.vdb_ivfpq_set_codebooks(h, m, _ffi.ptr(cb)), INVALID, "M")
    refused(lib.vdb_ivfpq_train(h, 8, _ffi.ptr(X), 255, 2, 0, 0), INVALID, "256")
    idx.set_codebooks(cb)
    idx.add(X, id_base=ID0)
    idx.set_nprobe(4)
    D0, I0 = idx.search(Q, 5)
    refused(lib.vdb_ivf_set_codec(h, 0), STATE, "before centroids or rows")
    for name in ("graph", "int8_only", "stream_panels"):
        refused(lib.vdb_set_option(h, name.encode(), 1.0), UNSUP, "IVF-PQ")
    refused(lib.vdb_add(h, _ffi.ptr(X), 10, ID0), UNSUP, "IVF-PQ")
    refused(lib.vdb_add_device(h, _ffi.ptr(X), 10, ID0, None), UNSUP, "IVF-PQ")        # (refused before the pointer is looked at)
    cand = np.zeros((len(Q), 4), np.int64)
    out_d, out_i = np.empty((len(Q), 2), F32), np.empty((len(Q), 2), np.int64)
    refused(lib.vdb_rerank(h, _ffi.ptr(Q), len(Q), _ffi.ptr(cand), 4, 2, _ffi.ptr(out_d), _ffi.ptr(out_i)), STATE, "IVF-PQ")
    proj = np.zeros((64, 64), F32)
    refused(lib.vdb_lsh_set_projection(h, 64, _ffi.ptr(proj)), UNSUP, "IVF-PQ")
    refused(lib.vdb_lsh_search(h, _ffi.ptr(Q), len(Q), 2, 16, _ffi.ptr(out_d), _ffi.ptr(out_i)), UNSUP, "IVF-PQ")
    refused(lib.vdb_lsh_get_codes(h, _ffi.ptr(np.zeros(8, np.uint32))), UNSUP, "IVF-PQ")
    refused(lib.vdb_pq_set_codebooks(h, 8, _ffi.ptr(cb)), UNSUP, "IVF")
    refused(lib.vdb_pq_train(h, 8, _ffi.ptr(X), len(X), 2, 0, 0), UNSUP, "IVF")
    refused(lib.vdb_pq_add(h, _ffi.ptr(X), 10, ID0), UNSUP, "IVF")
    refused(lib.vdb_pq_add_codes(h, _ffi.ptr(np.zeros((10, 8), np.uint8)), 10, ID0), UNSUP, "IVF")
    refused(lib.vdb_pq_get_codes(h, _ffi.ptr(np.zeros((len(X), 8), np.uint8))), UNSUP, "IVF")
    v = np.zeros(64, F32)
    refused(lib.vdb_ivf_sq8_train_ranges(h, _ffi.ptr(X), len(X)), UNSUP, "IVF-PQ")
    refused(lib.vdb_ivf_sq8_set_ranges(h, _ffi.ptr(v), _ffi.ptr(v)), UNSUP, "IVF-PQ")
    refused(lib.vdb_ivf_sq8_get_ranges(h, _ffi.ptr(v), _ffi.ptr(v)), UNSUP, "IVF-PQ")
    refused(lib.vdb_ivf_get_codes(h, _ffi.ptr(np.zeros((len(X), 64), np.uint8))), UNSUP, "IVF-PQ")
    D1, I1 = idx.search(Q, 5)                                    # ... and the index is as it was
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1, D0)
    assert idx.stats()["ntotal"] == len(X)
    idx.close()

    # the other order: the option, the projection or the flat codebooks first, then the codec
    for name in ("graph", "int8_only", "stream_panels"):
        f = vdb.FlatIndex(64, "l2", 0)
        f.set_option(name, 1)
        refused(lib.vdb_ivf_set_codec(f._h, 2), UNSUP, "IVF-PQ")
        f.close()
    f = vdb.FlatIndex(64, "l2", 0)
    f.lsh_set_projection(vdb.make_projection(64, 64, 0))
    refused(lib.vdb_ivf_set_codec(f._h, 2), UNSUP, "LSH")
    f.close()
    p = vdb.PQIndex(64, 8, "l2", 0)
    p.set_codebooks(cb)
    refused(lib.vdb_ivf_set_codec(p._h, 2), UNSUP, "flat PQ")
    refused(lib.vdb_ivfpq_set_codebooks(p._h, 8, _ffi.ptr(cb)), UNSUP, "flat PQ")
    p.close()
    # the calls of the codec on handles of another codec, and the codec on a multi-device handle
    for make in (lambda: vdb.IVFFlatIndex(64, 8, "l2", 0), lambda: vdb.IVFSQ8Index(64, 8, "l2", 0), lambda: vdb.FlatIndex(64, "l2", 0)):
        o = make()
        refused(lib.vdb_ivfpq_set_codebooks(o._h, 8, _ffi.ptr(cb)), STATE, "IVF-PQ")
        refused(lib.vdb_ivfpq_train(o._h, 8, _ffi.ptr(X), len(X), 2, 0, 0), STATE, "IVF-PQ")
        refused(lib.vdb_ivfpq_add_codes(o._h, _ffi.ptr(np.zeros((10, 8), np.uint8)), 10, 0, _ffi.ptr(np.zeros(10, np.int32))), STATE, "IVF-PQ")
        refused(lib.vdb_ivfpq_get_codes(o._h, _ffi.ptr(np.zeros((10, 8), np.uint8))), STATE, "IVF-PQ")
        o.close()
    m = _ffi.create_handle(64, 0, [0, 0])
    try:
        refused(lib.vdb_ivf_set_codec(m, 2), UNSUP, "multi-device", "IVF-PQ")
        refused(lib.vdb_ivfpq_set_codebooks(m, 8, _ffi.ptr(cb)), UNSUP, "multi-device")
    finally:
        lib.vdb_destroy(m)
    with pytest.raises(ValueError, match="one GPU"):
        vdb.IVFPQIndex(64, 8, 8, "l2", device=[0, 0])


def test_footprint(vdb):
    """codes + a list id and an id per row + one bias float per padded row + the constant tables: 0.16 x the float32 corpus.  The
    10 % cover the growth slack of the shared IVF arrays (bias, offsets, spans) and the coarse quantizer's own small index."""
    rng = np.random.default_rng(9)
    n, d, M, nlist = 200000, 128, 64, 64
    X = rng.standard_normal((n, d)).astype(F32)
    C = X[rng.choice(n, nlist, replace=False)].copy()
    cb = (rng.standard_normal((M, 256, d // M)) * 0.9).astype(F32)
    idx = _index(vdb, d, M, C, cb, "l2")
    idx.add(X)
    s = idx.stats()
    got = s["bytes_resident"] - s["bytes_workspace"]
    counts = np.bincount(idx.assignment(), minlength=nlist)
    n_padded = int(((counts + 255) // 256 * 256).sum())
    want = n * (M + 4 + 8) + n_padded * 4 + 256 * d * 4 + nlist * d * 4
    print(f"IVF-PQ resident {got} bytes = {got / (4 * n * d):.3f} x the float32 corpus; the formula gives {want} ({got / want:.3f} x)")
    assert abs(got - want) <= 0.10 * want, s
    assert got <= 0.18 * 4 * n * d
    idx.set_nprobe(8)
    idx.search(X[:1000], 10)
    s = idx.stats()
    assert s["scan_dtype"] == 2 and s["last_candidates"] > 0, s
    idx.close()


# ---- allocation balance: one child process under $VDBHIP_ALLOC_LOG, as tests/test_gpu_alloc_balance.py checks the other kinds ----
def child() -> None:
    sys.path[:0] = [str(ROOT), str(ROOT / "vectordb-retrieval_amd")]
    import torch
    import vdbhip

    from tests.test_gpu_alloc_balance import _device_search, _floats

    report = {}
    for name, d, M in (("ivf_pq_d64", 64, 16), ("ivf_pq_d192", 192, 48)):
        X, Q = _floats(20000, d, 31), _floats(64, d, 32)
        idx = vdbhip.IVFPQIndex(d, 32, M, "l2", 0)
        idx.train(X, niter=2)
        idx.add(X[:12000])
        idx.add(X[12000:])
        idx.reserve(len(Q), 10)
        rep = report.setdefault(name, {})
        for nprobe in (8, 1):
            idx.set_nprobe(nprobe)
            _, I_host = idx.search(Q, 10)
            rep[f"nprobe{nprobe}_dtype"] = idx.stats()["scan_dtype"]
            I_dev = _device_search(torch, idx.search_device, Q, 10)
            assert np.array_equal(I_host, I_dev)
        rep.update({key: idx.stats()[key] for key in ("bytes_resident", "bytes_workspace")})
        codes, lor = idx.codes(), idx.assignment()
        idx.reset()
        idx.add_codes(codes, lor)
        idx.set_nprobe(8)
        idx.search(Q, 10)
        idx.close()
    print("ALLOC_BALANCE_REPORT " + json.dumps(report), flush=True)


def test_every_allocation_is_freed_once(tmp_path):
    from tests.test_gpu_alloc_balance import check_log

    log = tmp_path / "alloc.log"
    env = dict(os.environ, VDBHIP_ALLOC_LOG=str(log))
    run = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, cwd=str(ROOT), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    tail = [ln for ln in run.stdout.splitlines() if ln.startswith("ALLOC_BALANCE_REPORT ")]
    assert tail, run.stdout[-4000:]
    report = json.loads(tail[-1].split(" ", 1)[1])
    print(json.dumps(report, indent=1))
    assert report["ivf_pq_d64"]["nprobe8_dtype"] == 2 and report["ivf_pq_d64"]["nprobe1_dtype"] == 0, report     # both list scans ran
    assert report["ivf_pq_d192"]["nprobe8_dtype"] == 0, report                                                       # (D > 128: exact only)
    problems, seen = check_log(log.read_text().splitlines())
    print(f"{seen} allocations, {len(problems)} problems")
    assert seen > 50
    assert not problems, "\n".join(problems[:40])


def test_published_random_ivf_pq_recall_point(vdb, golden_dir):
    """The reference's published `ivf_pq` point on the random dataset (IVF256,PQ64, nprobe 24), met within the tolerance of
    tests/golden/faiss_ivfpq_published.json: twice the largest deviation of ten training seeds from the published value."""
    from vdbhip import datasets, harness
    from vdbhip.metrics import recall_at_k

    man = json.loads((golden_dir / "manifest.json").read_text())["published_points"]["random_ivf_flat"]
    pub = json.loads((golden_dir / "faiss_ivfpq_published.json").read_text())
    opt = man["dataset_options"]
    train, test = datasets.random_reference(opt["dimensions"], opt["train_size"], opt["test_size"], opt["seed"])
    gt = harness.ground_truth(train, test, k=opt["ground_truth_k"], metric="l2")
    state = np.random.get_state()
    try:
        np.random.seed(man["config_seed"])
        sel = np.random.choice(len(test), man["n_queries"], replace=False)
    finally:
        np.random.set_state(state)
    q, g = test[sel], gt[sel]
    r10s, r1s = [], []
    for seed in pub["recorded"]["seeds"]:
        algo = vdb.get_algorithm_instance(
            "Composite", opt["dimensions"], name="ivf_pq", metric="l2",
            indexer={"type": "HipIVFPQIndexer", "index_key": pub["index_key"], "nprobe": pub["nprobe"], "seed": seed, "reserve_queries": 0},
            searcher={"type": "HipIVFSearcher", "nprobe": pub["nprobe"]})
        algo.build_index(train)
        _, ids = algo.batch_search(q, pub["topk"])
        r10s.append(recall_at_k(g, ids, 10))
        r1s.append(recall_at_k(g, ids, 1))
        algo.searcher.index.close()
    print(f"published recall@10 {pub['recall@10']:.7f} / recall@1 {pub['recall@1']:.7f}; ten seeds: recall@10 "
          f"{min(r10s):.4f}..{max(r10s):.4f} {[round(float(v), 7) for v in r10s]}, recall@1 {min(r1s):.4f}..{max(r1s):.4f} "
          f"{[round(float(v), 7) for v in r1s]}")
    assert np.allclose(r10s, pub["recorded"]["recall@10"], rtol=0, atol=1e-9), r10s
    assert np.allclose(r1s, pub["recorded"]["recall@1"], rtol=0, atol=1e-9), r1s
    assert abs(r10s[0] - pub["recall@10"]) <= pub["tolerance_recall@10"], r10s
    assert abs(r1s[0] - pub["recall@1"]) <= pub["tolerance_recall@1"], r1s


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()

"""IVF-Flat on the GPU vs the CPU restatement (oracle/ivf_oracle.c).

FAISS's k-means is not reproducible without FAISS (SURVEY 7 hard part 6), so parity is pinned as:
 (a) with INJECTED centroids: list assignment and search results bit-exact against the oracle, i.e. an IVF
     result == brute force restricted to the probed lists;
 (b) with the library's own k-means: clustering quality comparable to a plain Lloyd reference, recall grows
     with nprobe and reaches brute force at nprobe = nlist.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ref_semantics as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    import vdbhip

    return vdbhip


def _data(n, d, nq, seed, clustered=True):
    rng = np.random.default_rng(seed)
    if clustered:
        centers = rng.standard_normal((40, d)).astype(np.float32) * 3
        X = (centers[rng.integers(0, 40, n)] + rng.standard_normal((n, d))).astype(np.float32)
        Q = (centers[rng.integers(0, 40, nq)] + rng.standard_normal((nq, d))).astype(np.float32)
    else:
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n,d,nlist,nq,k", [(20000, 64, 100, 77, 10), (5000, 50, 37, 20, 20), (60000, 128, 256, 300, 10)])
def test_injected_centroids_bit_exact(vdb, oracle, metric, n, d, nlist, nq, k):
    X, Q = _data(n, d, nq, seed=n + nlist)
    rng = np.random.default_rng(1)
    C = X[rng.choice(n, nlist, replace=False)].copy()
    idx = vdb.IVFFlatIndex(d, nlist, metric, 0)
    idx.set_centroids(C)
    np.testing.assert_array_equal(idx.centroids(), C)
    idx.add(X, id_base=1000)
    lor = idx.assignment()
    np.testing.assert_array_equal(lor, oracle.ivf_assign(C, X, metric))
    for nprobe in (1, 4, 16, nlist, 5 * nlist):
        idx.set_nprobe(nprobe)
        D, I = idx.search(Q, k)
        Do, Io = oracle.ivf_search(X, C, lor, Q, k, min(nprobe, nlist), metric, id_base=1000)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
    # probing every list == brute force
    Db, Ib = oracle.knn(X, Q, k, metric, id_base=1000)
    np.testing.assert_array_equal(I, Ib)
    np.testing.assert_array_equal(D, Db)
    st = idx.stats()
    assert st["last_path_name"] == "ivf" and st["nlist"] == nlist
    # the exact list scan (force_path=1) and the list-major MFMA scan must agree bit for bit
    idx.set_nprobe(16)
    D1, I1 = idx.search(Q, k)
    idx.set_option("force_path", 1)
    D2, I2 = idx.search(Q, k)
    np.testing.assert_array_equal(I1, I2)
    np.testing.assert_array_equal(D1, D2)
    idx.close()


def test_list_major_mfma_scan_is_used_and_exact(vdb, oracle):
    X, Q = _data(200000, 128, 1000, 21, clustered=False)
    nlist = 256
    C = X[np.random.default_rng(2).choice(len(X), nlist, replace=False)].copy()
    for metric in ("l2", "ip"):
        idx = vdb.IVFFlatIndex(128, nlist, metric, 0)
        idx.set_centroids(C)
        idx.add(X)
        lor = idx.assignment()
        for nprobe in (8, 64):
            idx.set_nprobe(nprobe)
            D, I = idx.search(Q, 10)
            st = idx.stats()
            Do, Io = oracle.ivf_search(X, C, lor, Q, 10, nprobe, metric)
            np.testing.assert_array_equal(I, Io)
            np.testing.assert_array_equal(D, Do)
            assert st["last_candidates"] > 0, st            # the MFMA path served the batch
            assert st["last_fallback_queries"] < 50, st
        idx.set_option("list_cap", 1)                       # every query overflows -> exact list scan per query
        D, I = idx.search(Q, 10)
        np.testing.assert_array_equal(I, Io)
        assert idx.stats()["last_fallback_queries"] == len(Q)
        idx.close()


def test_small_lists_padding_and_errors(vdb, oracle):
    X, Q = _data(300, 16, 9, 5)
    C = X[:64].copy()
    idx = vdb.IVFFlatIndex(16, 64, "l2", 0)
    with pytest.raises(RuntimeError):
        idx.search(Q, 3)                      # not built
    idx.set_centroids(C)
    with pytest.raises(RuntimeError):
        idx.search(Q, 3)                      # centroids but no vectors
    idx.add(X)
    idx.set_nprobe(1)
    D, I = idx.search(Q, 30)                  # lists hold ~5 rows: FAISS-style -1 / FLT_MAX padding
    Do, Io = oracle.ivf_search(X, C, idx.assignment(), Q, 30, 1, "l2")
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    assert (I == -1).any() and np.all(D[I == -1] == np.finfo(np.float32).max)
    # a list id out of range in `add_assigned` is refused before the add touches the handle: same lists, same results
    bad = np.zeros(5, np.int32)
    bad[2] = 64
    with pytest.raises(ValueError, match="row could not be assigned to a list"):
        idx.add(X[:5], list_of_row=bad)
    assert idx.stats()["ntotal"] == len(X)
    D2, I2 = idx.search(Q, 30)
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    idx.close()


@pytest.mark.parametrize("codec", ["flat", "sq8"])
def test_rerank_refuses_rows_in_list_order(vdb, codec):
    """vdb_rerank / vdb_rerank_device score rows by id; an index filed by vdb_ivf_add keeps them in list order (SQ8: no float32
    rows at all).  Both calls return VDB_ERR_STATE before any kernel runs, on one device and on a multi-device handle, and the
    index searches as before."""
    import torch
    from vdbhip import _ffi

    lib = _ffi.load()
    X, Q = _data(3000, 32, 8, 6)
    C = X[:16].copy()
    cand = np.tile(np.arange(20, dtype=np.int64), (len(Q), 1))
    D = np.empty((len(Q), 5), np.float32)
    I = np.empty((len(Q), 5), np.int64)
    q_t, c_t = torch.from_numpy(Q).cuda(), torch.from_numpy(cand).cuda()
    D_t = torch.empty((len(Q), 5), dtype=torch.float32, device="cuda")
    I_t = torch.empty((len(Q), 5), dtype=torch.int64, device="cuda")
    handles = [(vdb.IVFSQ8Index if codec == "sq8" else vdb.IVFFlatIndex)(32, 16, "l2", 0)]
    if codec == "flat":
        handles.append(vdb.IVFFlatIndex(32, 16, "l2", [0, 0]))
    for idx in handles:
        idx.set_centroids(C)
        if codec == "sq8":
            idx.train_ranges(X)
        idx.add(X)
        idx.set_nprobe(4)
        before = idx.search(Q, 5)
        rc = lib.vdb_rerank(idx._h, _ffi.ptr(Q), len(Q), _ffi.ptr(cand), 20, 5, _ffi.ptr(D), _ffi.ptr(I))
        assert rc == _ffi.VDB_ERR_STATE and "not been built" in _ffi.last_error(), (rc, _ffi.last_error())
        rc = lib.vdb_rerank_device(idx._h, q_t.data_ptr(), len(Q), c_t.data_ptr(), 20, 5, D_t.data_ptr(), I_t.data_ptr(), None)
        assert rc == _ffi.VDB_ERR_STATE and "not been built" in _ffi.last_error(), (rc, _ffi.last_error())
        after = idx.search(Q, 5)
        np.testing.assert_array_equal(after[1], before[1])
        np.testing.assert_array_equal(after[0], before[0])
        idx.close()


def test_multi_device_add_assigned_refuses_a_bad_list_id_up_front(vdb):
    X, Q = _data(3000, 32, 8, 7)
    idx = vdb.IVFFlatIndex(32, 16, "l2", [0, 0])
    idx.set_centroids(X[:16].copy())
    idx.add(X)
    idx.set_nprobe(4)
    before = idx.search(Q, 5)
    bad = np.zeros(10, np.int32)
    bad[8] = 16                         # (in the second shard's block of the add)
    with pytest.raises(ValueError, match="row could not be assigned to a list"):
        idx.add(X[:10], list_of_row=bad)
    assert idx.stats()["ntotal"] == len(X)
    after = idx.search(Q, 5)
    np.testing.assert_array_equal(after[1], before[1])
    np.testing.assert_array_equal(after[0], before[0])
    idx.close()


def test_kmeans_quality_and_recall_curve(vdb, oracle):
    X, Q = _data(50000, 32, 400, 11)
    nlist = 128
    idx = vdb.IVFFlatIndex(32, nlist, "l2", 0)
    idx.train(X, niter=10, seed=1234)
    C = idx.centroids()
    assert np.isfinite(C).all() and C.shape == (nlist, 32)
    obj = oracle.kmeans_objective(C, X)
    # plain Lloyd reference from the same kind of init (numpy, float64 means)
    rng = np.random.default_rng(7)
    Cr = X[rng.choice(len(X), nlist, replace=False)].astype(np.float64)
    for _ in range(10):
        a = oracle.ivf_assign(Cr.astype(np.float32), X, "l2")
        for j in range(nlist):
            m = a == j
            if m.any():
                Cr[j] = X[m].astype(np.float64).mean(0)
    obj_ref = oracle.kmeans_objective(Cr.astype(np.float32), X)
    assert obj <= obj_ref * 1.05, (obj, obj_ref)
    idx.train(X, niter=10, seed=1234)               # deterministic
    np.testing.assert_array_equal(idx.centroids(), C)
    idx.add(X)
    assert np.bincount(idx.assignment(), minlength=nlist).min() > 0
    _, gt = oracle.knn(X, Q, 10, "l2")
    recalls = []
    for nprobe in (1, 4, 16, 64, nlist):
        idx.set_nprobe(nprobe)
        _, I = idx.search(Q, 10)
        recalls.append(rs.recall_at_k(gt, I, 10))
    assert all(b >= a - 1e-9 for a, b in zip(recalls, recalls[1:])), recalls
    assert recalls[-1] == 1.0 and recalls[2] > 0.8, recalls
    idx.close()


def test_plugin_conventions(vdb, oracle):
    """FaissSearcher sign flips / cosine normalisation vs ApproximateSearch raw conventions."""
    X, Q = _data(8000, 24, 33, 3)
    # ApproximateSearch-like: raw inner product, descending, nprobe from kwargs
    a = vdb.get_algorithm_instance("HipApproximateSearch", 24, name="ivf", index_type="IVF32,Flat", metric="ip",
                                   nprobe=32, niter=5)
    a.build_index(X)
    d, i = a.batch_search(Q, k=5)
    do, io = oracle.knn(X, Q, 5, "ip")                 # all lists probed -> brute force
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(d, do)
    d1, i1 = a.search(Q[0], k=5)
    np.testing.assert_array_equal(i1, io[0])
    with pytest.raises(ValueError):
        vdb.get_algorithm_instance("HipApproximateSearch", 24, name="x", index_type="IVF32,PQ8")
    # modular pair, cosine: normalise both sides, distances = -score; searcher nprobe overrides indexer nprobe
    c = vdb.CompositeAlgorithm(name="ivf_cos", dimension=24, metric="cosine",
                               indexer={"type": "HipIVFIndexer", "index_type": "IVF32,Flat", "metric": "cosine",
                                        "nprobe": 1, "niter": 5},
                               searcher={"type": "HipIVFSearcher", "metric": "cosine", "nprobe": 32})
    c.build_index(X)
    d, i = c.batch_search(Q, k=5)
    Xn, Qn = rs.safe_normalize(X), rs.safe_normalize(Q)
    do, io = oracle.knn(Xn, Qn, 5, "ip")
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(d, -do)
    assert c.searcher.index.nprobe == 32
    assert d.dtype == np.float32 and i.dtype == np.int64
    # modular pair, l2 keeps SQUARED distances (FaissSearcher)
    c = vdb.CompositeAlgorithm(name="ivf_l2", dimension=24, metric="l2",
                               indexer={"type": "HipIVFIndexer", "index_type": "IVF32,Flat", "metric": "l2",
                                        "nprobe": 32, "niter": 5},
                               searcher={"type": "HipIVFSearcher", "metric": "l2"})
    c.build_index(X)
    d, i = c.batch_search(Q, k=5)
    do, io = oracle.knn(X, Q, 5, "l2")
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(d, do)


def test_ivf_persistence_round_trip(vdb, tmp_path):
    """save_index / load_index hook (base_algorithm.py:98-120) with the reference's artifact protocol:
    manifest + WRITE_COMPLETE sentinel, refusal of incomplete or mismatching artifacts
    (idiom of the reference's tests/algorithms/test_covertree_v2_2.py persistence tests)."""
    X, Q = _data(6000, 16, 25, 8)
    a = vdb.get_algorithm_instance("HipApproximateSearch", 16, name="ivf", index_type="IVF16,Flat", metric="l2",
                                   nprobe=4, niter=5)
    with pytest.raises(RuntimeError):
        a.save_index(str(tmp_path / "art"))
    a.build_index(X)
    d0, i0 = a.batch_search(Q, k=5)
    info = a.save_index(str(tmp_path / "art"), context={"build_metrics": {"build_time_s": 1.5}, "config_hash": "abc"})
    assert (tmp_path / "art" / "WRITE_COMPLETE").is_file() and info["build_time_s"] == 1.5
    with pytest.raises(FileExistsError):
        a.save_index(str(tmp_path / "art"))
    a.save_index(str(tmp_path / "art"), context={"force_rebuild": True, "config_hash": "abc"})
    b = vdb.get_algorithm_instance("HipApproximateSearch", 16, name="ivf2", index_type="IVF16,Flat", metric="l2",
                                   nprobe=4)
    b.load_index(str(tmp_path / "art"), context={"config_hash": "abc"})
    d1, i1 = b.batch_search(Q, k=5)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1, d0)
    with pytest.raises(ValueError):
        b.load_index(str(tmp_path / "art"), context={"config_hash": "zzz"})
    c = vdb.get_algorithm_instance("HipApproximateSearch", 16, name="ivf3", index_type="IVF32,Flat", metric="l2")
    with pytest.raises(ValueError):
        c.load_index(str(tmp_path / "art"))
    # files that do not belong together are refused: a regenerated corpus, a quantizer from another run --
    # through the stored fingerprint, and for artifacts written before it existed through a sampled re-assignment
    import json
    import shutil

    for victim, make in (("vectors.npy", lambda: _data(6000, 16, 1, 9)[0]),
                         ("centroids.npy", lambda: np.load(tmp_path / "art" / "centroids.npy")[::-1].copy())):
        for drop_fingerprint in (False, True):
            bad = tmp_path / f"bad_{victim}_{int(drop_fingerprint)}"
            shutil.copytree(tmp_path / "art", bad)
            np.save(bad / victim, make(), allow_pickle=False)
            if drop_fingerprint:
                m = json.loads((bad / "manifest.json").read_text())
                m.pop("sha256")
                (bad / "manifest.json").write_text(json.dumps(m))
            with pytest.raises(ValueError, match="do not belong together|do not match"):
                b.load_index(str(bad))
    old = tmp_path / "old_format"           # an intact artifact without the fingerprint still loads
    shutil.copytree(tmp_path / "art", old)
    m = json.loads((old / "manifest.json").read_text())
    m.pop("sha256")
    (old / "manifest.json").write_text(json.dumps(m))
    b.load_index(str(old), context={"config_hash": "abc"})
    np.testing.assert_array_equal(b.batch_search(Q, k=5)[1], i0)
    (tmp_path / "art" / "WRITE_COMPLETE").unlink()
    with pytest.raises(FileNotFoundError):
        b.load_index(str(tmp_path / "art"))
    with pytest.raises(FileNotFoundError):
        b.load_index(str(tmp_path / "missing"))
    # algorithms without persistence keep the base-class behaviour
    with pytest.raises(NotImplementedError):
        vdb.HipExactSearch("e", 4).save_index(str(tmp_path / "x"))


@pytest.mark.parametrize("metric,nshards", [("l2", 2), ("ip", 3)])
def test_row_sharded_ivf_partials_merge_to_unsharded_result(vdb, oracle, metric, nshards):
    """SURVEY 8e for IVF: shared centroids, the rows of every list split over shards, per-shard partial top-k
    (vdb_ivf_search_partial_device) merged by (float64 key, id) == the unsharded index, bit for bit.  Covers the
    list-major MFMA scan (300 queries) and the exact list scan (20 queries) on the shards."""
    import torch

    n, d, nlist, k = 60000, 64, 128, 10
    X, Q = _data(n, d, 300, seed=99)
    C = X[np.random.default_rng(5).choice(n, nlist, replace=False)].copy()
    full = vdb.IVFFlatIndex(d, nlist, metric, 0)
    full.set_centroids(C)
    full.add(X, id_base=7)
    shards = []
    for r in range(nshards):
        lo, hi = vdb.sharded.shard_bounds(n, nshards, r)
        s = vdb.IVFFlatIndex(d, nlist, metric, 0)
        s.set_centroids(C)
        s.add(X[lo:hi], id_base=7 + lo)
        shards.append(s)
    dev = torch.device("cuda:0")
    for nq, nprobe in ((300, 8), (20, 8), (300, 1), (64, nlist)):
        q_t = torch.from_numpy(Q[:nq]).to(dev)
        full.set_nprobe(nprobe)
        D_ref, I_ref = full.search(Q[:nq], k)
        pack = torch.empty((nshards, 2, nq, k), dtype=torch.int64, device=dev)
        for r, s in enumerate(shards):
            s.set_nprobe(nprobe)
            s.search_partial_device(q_t.data_ptr(), nq, k, pack[r, 0].data_ptr(), pack[r, 1].data_ptr())
        D_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
        vdb.merge_packed_partials_device(metric, 0, pack.data_ptr(), nshards, nq, k, D_t.data_ptr(), I_t.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(I_t.cpu().numpy(), I_ref)
        np.testing.assert_array_equal(D_t.cpu().numpy(), D_ref)
        # partial keys are sorted ascending with (+inf, -1) padding
        keys = pack[:, 0].cpu().numpy().view(np.float64)
        assert np.all(np.diff(keys, axis=-1) >= 0)
    Do, Io = oracle.ivf_search(X, C, full.assignment(), Q[:64], k, nlist, metric, id_base=7)
    np.testing.assert_array_equal(I_ref, Io)
    for s in shards + [full]:
        s.close()


@pytest.mark.parametrize("metric,window,d", [("l2", "u8", 128), ("ip", "u8", 96), ("l2", "s8", 64), ("l2", "u8", 50)])
def test_int8_list_scan_bit_exact(vdb, oracle, metric, window, d):
    """Byte-valued corpora: the list-major scan runs on the int8 copy (scan_i8.hpp, items mode) when the query batch is
    integer too -- same results as the oracle, as the fp16 list scan and as the exact list scan."""
    rng = np.random.default_rng(31)
    n, nq, nlist, k = 150_000, 700, 128, 10
    off = 0 if window == "u8" else -128
    X = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(np.float32) + off
    Q = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(nq, d))), 0, 255).astype(np.float32) + off
    C = X[rng.choice(n, nlist, replace=False)] + rng.uniform(-0.25, 0.25, (nlist, d)).astype(np.float32)
    idx = vdb.IVFFlatIndex(d, nlist, metric, 0)
    idx.set_centroids(C)
    idx.add(X, id_base=7)
    lor = idx.assignment()
    for nprobe in (4, 16, 64):
        idx.set_nprobe(nprobe)
        D, I = idx.search(Q, k)
        st = idx.stats()
        assert st["last_path_name"] == "ivf" and st["has_i8_copy"] == 1 and st["scan_dtype"] == 1, st
        Do, Io = oracle.ivf_search(X, C, lor, Q, k, nprobe, metric, id_base=7)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
        idx.set_option("panel_dtype", 1)            # fp16 list scan of the same index
        D1, I1 = idx.search(Q, k)
        assert idx.stats()["scan_dtype"] == 0
        idx.set_option("panel_dtype", 0)
        np.testing.assert_array_equal(I1, I)
        np.testing.assert_array_equal(D1, D)
    Q2 = Q.copy()
    Q2[3, 5] += 0.25                                 # one non-integer value: the batch takes the fp16 scan
    D2, I2 = idx.search(Q2, k)
    assert idx.stats()["scan_dtype"] == 0
    Do2, Io2 = oracle.ivf_search(X, C, lor, Q2, k, 64, metric, id_base=7)
    np.testing.assert_array_equal(I2, Io2)
    np.testing.assert_array_equal(D2, Do2)
    idx.close()


@pytest.mark.parametrize("kind", ["bytes", "gauss"])
def test_small_query_batches_and_row_parts_bit_exact(vdb, oracle, kind):
    """Serving-shaped IVF batches (1 ... 65 queries) go through the list-major MFMA scan too (`ivf_min_batch`), the
    coarse quantizer through the split exhaustive scan; long lists are scanned in row parts (`ivf_part`).  Skewed list
    sizes (a third of the rows sit in four lists), every part size, the int8 and the fp16 list scan: the oracle's bits."""
    rng = np.random.default_rng(17)
    n, d, nlist, k = 120_000, 128, 96, 10
    if kind == "bytes":
        X = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(np.float32)
        Q = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(700, d))), 0, 255).astype(np.float32)
    else:
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = rng.standard_normal((700, d)).astype(np.float32)
    X[: n // 3] = X[:4].repeat(n // 12, axis=0) + (np.rint(rng.uniform(-3, 3, (n // 3, d))) if kind == "bytes"
                                                     else 0.05 * rng.standard_normal((n // 3, d))).astype(np.float32)
    if kind == "bytes":
        X = np.clip(X, 0, 255)
    C = X[rng.choice(n, nlist, replace=False)] + rng.uniform(-0.25, 0.25, (nlist, d)).astype(np.float32)
    C[:4] = X[:4]
    idx = vdb.IVFFlatIndex(d, nlist, "l2", 0)
    idx.set_centroids(C)
    idx.add(X)
    lor = idx.assignment()
    assert np.bincount(lor, minlength=nlist).max() > 5 * n // nlist        # the skew is there
    idx.set_nprobe(12)
    Do, Io = oracle.ivf_search(X, C, lor, Q, k, 12, "l2")
    for nq in (1, 3, 8, 63, 64, 65, 700):
        for part in (0, 1, 3, 1024):
            idx.set_option("ivf_part", part)
            D, I = idx.search(Q[:nq], k)
            st = idx.stats()
            assert st["last_path_name"] == "ivf" and st["scan_dtype"] == (1 if kind == "bytes" else 0), (nq, part, st)
            np.testing.assert_array_equal(I, Io[:nq], err_msg=f"nq={nq} ivf_part={part}")
            np.testing.assert_array_equal(D, Do[:nq], err_msg=f"nq={nq} ivf_part={part}")
    idx.set_option("ivf_part", 0)
    idx.set_option("ivf_min_batch", 64)              # the exact list scan for small batches, as before: same bits
    D, I = idx.search(Q[:8], k)
    np.testing.assert_array_equal(I, Io[:8])
    np.testing.assert_array_equal(D, Do[:8])
    idx.close()


# ---------------------------------------------------------------------------------------------------------
# D > 128: the items-mode K-loop scan (csrc/ivf_kloop.hpp)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,nlist,nq,k,metric,tps,nprobe", [
    (100_000, 384, 100, 1000, 20, "cosine", 0, 32),    # the reference's committed msmarco IVF shape (see test below)
    (30_000, 200, 64, 300, 10, "l2", 0, 8),            # D not a multiple of 64, L2
    (40_000, 768, 50, 129, 10, "ip", 0, 10),           # 768 dims, a batch that leaves padding waves in its work items
    (60_000, 256, 16, 200, 10, "l2", 64, 4),           # long lists on 1024-row spans (256-row bins)
    (60_000, 256, 16, 200, 10, "ip", 16, 16),          # the same lists on 256-row spans, every list probed
])
def test_kloop_list_scan_bit_exact(vdb, oracle, n, d, nlist, nq, k, metric, tps, nprobe):
    """IVF-Flat on embeddings-sized vectors: the list-major MFMA scan serves D > 128 (it used to stop at 128 dims and
    leave 384 / 768-dim indexes to the exhaustive float64 list scan).  Result == brute force over the probed lists, bit
    for bit, from the MFMA path (candidates > 0), equal to the exact list scan (force_path = 1), for both span sizes."""
    X, Q = _data(n, d, nq, seed=n + d)
    m = "ip" if metric == "cosine" else metric
    if metric == "cosine":
        X, Q = rs.safe_normalize(X), rs.safe_normalize(Q)
    C = X[np.random.default_rng(d).choice(n, nlist, replace=False)].copy()
    idx = vdb.IVFFlatIndex(d, nlist, m, 0)
    idx.set_centroids(C)
    if tps:
        idx.set_option("ivf_tps", tps)
    idx.add(X, id_base=5)
    lor = idx.assignment()
    np.testing.assert_array_equal(lor, oracle.ivf_assign(C, X, m))
    idx.set_nprobe(nprobe)
    D, I = idx.search(Q, k)
    st = idx.stats()
    Do, Io = oracle.ivf_search(X, C, lor, Q, k, nprobe, m, id_base=5)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    assert st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st      # the MFMA path served the batch
    assert st["last_fallback_queries"] <= nq // 20, st
    assert st["last_rows_scanned"] > 0
    idx.set_option("force_path", 1)
    D1, I1 = idx.search(Q, k)
    idx.set_option("force_path", 0)
    np.testing.assert_array_equal(I1, I)
    np.testing.assert_array_equal(D1, D)
    # row parts of one span and whole lists give the same bins
    for part in (1, 1024):
        idx.set_option("ivf_part", part)
        D2, I2 = idx.search(Q, k)
        np.testing.assert_array_equal(I2, I, err_msg=f"ivf_part={part}")
        np.testing.assert_array_equal(D2, D, err_msg=f"ivf_part={part}")
    idx.set_option("ivf_part", 0)
    # round 4: every candidate group (rows / pairs / quads on 64-row bins) and both workgroup tiles give the same result
    for opt, values in (("ivf_group", (4, 2, 1, 0)), ("ivf_tile", (2, 0))):
        for v in values:
            idx.set_option(opt, v)
            D3, I3 = idx.search(Q, k)
            np.testing.assert_array_equal(I3, I, err_msg=f"{opt}={v}")
            np.testing.assert_array_equal(D3, D, err_msg=f"{opt}={v}")
    idx.set_option("ivf_tile", 2)
    idx.set_option("ivf_group", 2)
    D3, I3 = idx.search(Q[:130], k)            # (square tile + pairs, a batch that leaves waves without slots)
    np.testing.assert_array_equal(I3, Io[:130])
    np.testing.assert_array_equal(D3, Do[:130])
    idx.set_option("ivf_tile", 0)
    idx.set_option("ivf_group", 0)
    # small batches (one partly filled work item per list) and a forced overflow of every work list
    for nqs in (1, 7, 70):
        Ds, Is = idx.search(Q[:nqs], k)
        np.testing.assert_array_equal(Is, Io[:nqs], err_msg=f"nq={nqs}")
        np.testing.assert_array_equal(Ds, Do[:nqs], err_msg=f"nq={nqs}")
    idx.set_option("list_cap", 1)
    Df, If = idx.search(Q[:64], k)
    np.testing.assert_array_equal(If, Io[:64])
    np.testing.assert_array_equal(Df, Do[:64])
    assert idx.stats()["last_fallback_queries"] >= 48         # (a query with a single candidate row does not overflow)
    idx.close()


def test_msmarco_shaped_ivf_through_the_plugins(vdb, oracle):
    """The reference's own IVF benchmark on embeddings (benchmark_results/benchmark_20260305_070532/msmarco/
    ivf_flat_results.json: 100 000 x 384, cosine, FaissIVFIndexer IVF100,Flat + FaissSearcher nprobe 32, topk 20, 70
    queries; modular.py:418-449, 536-548) through HipIVFIndexer + HipIVFSearcher with the library's own k-means: the
    searcher's conventions (normalised queries, negated scores) over results that equal the CPU restatement of IVF-Flat
    on the trained centroids, served by the MFMA list scan."""
    rng = np.random.default_rng(384)
    centres = rng.standard_normal((64, 384)).astype(np.float32)
    X = (centres[rng.integers(0, 64, 100_000)] + 1.5 * rng.standard_normal((100_000, 384))).astype(np.float32)
    Q = (centres[rng.integers(0, 64, 70)] + 1.5 * rng.standard_normal((70, 384))).astype(np.float32)
    algo = vdb.CompositeAlgorithm(name="ivf_flat", dimension=384, metric="cosine",
                                  indexer={"type": "HipIVFIndexer", "index_type": "IVF100,Flat", "metric": "cosine",
                                           "nprobe": 10},
                                  searcher={"type": "HipIVFSearcher", "metric": "cosine", "nprobe": 32})
    algo.build_index(X)
    d, i = algo.batch_search(Q, k=20)
    index = algo.searcher.index
    st = index.stats()
    assert index.nprobe == 32 and st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st
    Xn, Qn = rs.safe_normalize(X), rs.safe_normalize(Q)
    do, io = oracle.ivf_search(Xn, index.centroids(), index.assignment(), Qn, 20, 32, "ip")
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(d, -do)
    _, ie = oracle.knn(Xn, Qn, 20, "ip")
    r10 = rs.recall_at_k(ie, i, 10)
    print(f"msmarco-shaped IVF100,Flat nprobe 32: recall@10 vs exact {r10:.4f} (the reference reports 0.9529 on its MS MARCO subset)")
    assert r10 > 0.85
    d1, i1 = algo.search(Q[0], k=20)
    np.testing.assert_array_equal(i1, io[0])


@pytest.mark.parametrize("d,metric,kind", [(64, "l2", "gauss"), (128, "l2", "bytes"), (200, "ip", "gauss")])
def test_add_appends_to_the_lists_like_faiss(vdb, oracle, d, metric, kind):
    """`faiss.IndexIVF.add` appends (a second vdb_add used to replace the corpus silently).  Three adds build
    the index one add of the concatenated rows builds: same assignment, ids and results, bit for bit; the id base belongs
    to the index; `reset` drops the rows and keeps the centroids; new centroids drop the rows."""
    n, nlist, nq, k = 30000, 64, 150, 10
    rng = np.random.default_rng(d)
    if kind == "bytes":
        X = rng.integers(0, 256, (n, d)).astype(np.float32)
        Q = rng.integers(0, 256, (nq, d)).astype(np.float32)
    else:
        X, Q = _data(n, d, nq, seed=d)
    C = X[rng.choice(n, nlist, replace=False)].copy()
    whole = vdb.IVFFlatIndex(d, nlist, metric, 0)
    whole.set_centroids(C)
    whole.add(X, id_base=500)
    parts = vdb.IVFFlatIndex(d, nlist, metric, 0)
    parts.set_centroids(C)
    cuts = [0, 9000, 9001, 22000, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.add(X[a:b], id_base=500)
        assert parts.ntotal == b
    parts.add(X[:0], id_base=500)                       # (an empty append changes nothing)
    np.testing.assert_array_equal(parts.assignment(), whole.assignment())
    for nprobe in (1, 8, nlist):
        whole.set_nprobe(nprobe)
        parts.set_nprobe(nprobe)
        Dw, Iw = whole.search(Q, k)
        Dp, Ip = parts.search(Q, k)
        np.testing.assert_array_equal(Ip, Iw)
        np.testing.assert_array_equal(Dp, Dw)
    Do, Io = oracle.ivf_search(X, C, whole.assignment(), Q, k, nlist, metric, id_base=500)
    np.testing.assert_array_equal(Ip, Io)
    np.testing.assert_array_equal(Dp, Do)
    with pytest.raises(ValueError, match="id base"):
        parts.add(X[:10], id_base=0)
    # stored assignment, appended
    given = vdb.IVFFlatIndex(d, nlist, metric, 0)
    given.set_centroids(C)
    lor = whole.assignment()
    given.add(X[:12345], id_base=500, list_of_row=lor[:12345])
    given.add(X[12345:], id_base=500, list_of_row=lor[12345:])
    given.set_nprobe(8)
    whole.set_nprobe(8)
    np.testing.assert_array_equal(given.search(Q, k)[1], whole.search(Q, k)[1])
    # reset: rows gone, centroids kept, another id base is fine
    parts.reset()
    assert parts.ntotal == 0
    with pytest.raises(RuntimeError):
        parts.search(Q, k)
    parts.add(X[:5000], id_base=7)
    parts.set_nprobe(nlist)
    Db, Ib = oracle.knn(X[:5000], Q, k, metric, id_base=7)
    Dr, Ir = parts.search(Q, k)
    np.testing.assert_array_equal(Ir, Ib)
    np.testing.assert_array_equal(Dr, Db)
    parts.set_centroids(C[::-1].copy())                 # new centroids: the next add starts over
    assert parts.ntotal == 0
    parts.add(X[:4000], id_base=0)
    assert parts.stats()["ntotal"] == 4000
    for i in (whole, parts, given):
        i.close()

"""IVF<nlist>,SQ8 on the GPU against a NumPy float32 restatement of the codec and the IVF oracle over the decoded rows.

The contract (include/vdbhip.h): ranges and codes equal the float32 formulas bit for bit, and a search equals
oracle.ivf_search over the decoded rows x^ (same centroids, same lists) bit for bit in ids and distances.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

from tests.helpers import np_decode, np_encode, np_ranges

pytestmark = pytest.mark.gpu

F32 = np.float32


def _data(n, d, nq, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((24, d)).astype(F32) * 3
    X = (centers[rng.integers(0, 24, n)] + rng.standard_normal((n, d))).astype(F32)
    Q = (centers[rng.integers(0, 24, nq)] + rng.standard_normal((nq, d))).astype(F32)
    X[:, 3] = F32(0.75)                   # a constant column: vdiff = 0 -> code 0
    return X, Q


def _sq8(vdb, X, C, metric, train_rows=None, id_base=1000):
    idx = vdb.IVFSQ8Index(X.shape[1], len(C), metric, 0)
    idx.set_centroids(C)
    idx.train_ranges(X if train_rows is None else train_rows)
    idx.add(X, id_base=id_base)
    return idx


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [50, 64, 128, 384])
def test_ranges_and_codes_bit_exact(vdb, oracle, metric, d):
    n = 5000 if d == 384 else 20000
    X, _ = _data(n, d, 1, seed=d)
    C = X[np.random.default_rng(1).choice(n, 32, replace=False)].copy()
    Xt = X[: n // 2]                       # ranges from half the rows: the other half has values that clamp
    idx = _sq8(vdb, X, C, metric, train_rows=Xt)
    lor_t = oracle.ivf_assign(C, Xt, metric)
    vmin, vdiff = np_ranges(Xt, C, lor_t)
    gv, gd = idx.ranges()
    np.testing.assert_array_equal(gv, vmin)
    np.testing.assert_array_equal(gd, vdiff)
    assert gd[3] == 0
    lor = idx.assignment()
    np.testing.assert_array_equal(lor, oracle.ivf_assign(C, X, metric))
    codes = idx.codes()
    want = np_encode(X, C, lor, vmin, vdiff)
    np.testing.assert_array_equal(codes, want)
    assert (codes[:, 3] == 0).all()
    R = X[n // 2:] - C[lor[n // 2:]]
    assert ((R < vmin) | (R > vmin + vdiff)).any()    # (some values did clamp)
    st = idx.stats()
    assert st["ntotal"] == n and st["nlist"] == 32
    idx.close()


def _check_search(idx, oracle, Xh, C, lor, Q, k, nprobe, metric):
    idx.set_nprobe(nprobe)
    D, I = idx.search(Q, k)
    Do, Io = oracle.ivf_search(Xh, C, lor, Q, k, min(nprobe, len(C)), metric, id_base=1000)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    return D, I


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_search_parity_with_the_oracle_over_decoded_rows(vdb, oracle, metric):
    n, d, nlist = 20000, 64, 64
    X, Q = _data(n, d, 10000, seed=7)
    X[5000:5040] = X[100:140]                        # duplicated rows (ties broken by the smaller id)
    X[5040:5060] = X[200:220]
    X[5040:5060, 0] += F32(8.0 / 255.0)              # ... and rows about one code step apart in one dimension
    C = X[np.random.default_rng(2).choice(n, nlist, replace=False)].copy()
    idx = vdb.IVFSQ8Index(d, nlist, metric, 0)
    idx.set_centroids(C)
    idx.set_ranges(np.full(d, -4.0, F32), np.full(d, 8.0, F32))
    idx.add(X, id_base=1000)
    lor = idx.assignment()
    vmin, vdiff = idx.ranges()
    Xh = np_decode(idx.codes(), C, lor, vmin, vdiff)
    for nprobe in (1, 4, 16, nlist):
        for k in (1, 10, 100):
            for nq in (1, 7, 300):
                _check_search(idx, oracle, Xh, C, lor, Q[:nq], k, nprobe, metric)
    # the 10 000-query batch: a fixed sample of 500 queries against the oracle
    idx.set_nprobe(16)
    D, I = idx.search(Q, 10)
    st = idx.stats()
    assert st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st     # the MFMA list scan served the batch
    assert st["scan_dtype"] == 2, st                                           # ... on fp16 panels from the codes
    pick = np.random.default_rng(3).choice(len(Q), 500, replace=False)
    Do, Io = oracle.ivf_search(Xh, C, lor, Q[pick], 10, 16, metric, id_base=1000)
    np.testing.assert_array_equal(I[pick], Io)
    np.testing.assert_array_equal(D[pick], Do)
    idx.set_option("force_path", 1)
    D1, I1 = idx.search(Q, 10)
    np.testing.assert_array_equal(I1, I)
    np.testing.assert_array_equal(D1, D)
    idx.close()


def test_mfma_list_scan_over_codes_is_used_and_exact(vdb, oracle):
    rng = np.random.default_rng(21)
    X = rng.standard_normal((200000, 128)).astype(F32)
    Q = rng.standard_normal((1000, 128)).astype(F32)
    C = X[np.random.default_rng(2).choice(len(X), 256, replace=False)].copy()
    for metric in ("l2", "ip"):
        idx = _sq8(vdb, X, C, metric, id_base=1000)
        lor = idx.assignment()
        vmin, vdiff = idx.ranges()
        Xh = np_decode(idx.codes(), C, lor, vmin, vdiff)
        for nprobe in (8, 64):
            D, I = _check_search(idx, oracle, Xh, C, lor, Q, 10, nprobe, metric)
            st = idx.stats()
            assert st["last_candidates"] > 0 and st["scan_dtype"] == 2, st
            assert st["last_fallback_queries"] < 50, st
        idx.set_option("list_cap", 1)                    # every query overflows -> the tail's exact list scan over codes
        D2, I2 = idx.search(Q, 10)
        np.testing.assert_array_equal(I2, I)
        np.testing.assert_array_equal(D2, D)
        assert idx.stats()["last_fallback_queries"] == len(Q)
        idx.set_option("list_cap", 0)
        idx.set_option("force_path", 1)                  # the exact list scan: the same result
        D3, I3 = idx.search(Q, 10)
        np.testing.assert_array_equal(I3, I)
        np.testing.assert_array_equal(D3, D)
        assert idx.stats()["last_candidates"] == 0
        idx.close()


def test_search_parity_d384(vdb, oracle):
    X, Q = _data(5000, 384, 50, seed=11)
    C = X[np.random.default_rng(4).choice(len(X), 16, replace=False)].copy()
    for metric in ("l2", "ip"):
        idx = _sq8(vdb, X, C, metric)
        lor = idx.assignment()
        vmin, vdiff = idx.ranges()
        Xh = np_decode(idx.codes(), C, lor, vmin, vdiff)
        for nprobe in (1, 4, 16):
            _check_search(idx, oracle, Xh, C, lor, Q, 10, nprobe, metric)
        idx.close()


def test_append_reserve_and_train(vdb, oracle):
    X, Q = _data(12000, 64, 40, seed=5)
    C = X[:48].copy()
    idx = vdb.IVFSQ8Index(64, 48, "l2", 0)
    idx.set_centroids(C)
    idx.train_ranges(X)
    idx.add(X[:7000], id_base=1000)
    idx.add(X[7000:], id_base=1000)                   # append: same lists as one add
    one = _sq8(vdb, X, C, "l2")
    np.testing.assert_array_equal(idx.codes(), one.codes())
    np.testing.assert_array_equal(idx.assignment(), one.assignment())
    idx.set_nprobe(8)
    one.set_nprobe(8)
    idx.reserve(500, 10)
    np.testing.assert_array_equal(idx.search(Q, 10)[1], one.search(Q, 10)[1])
    # vdb_ivf_train on an SQ8 handle: centroids, then ranges over the same rows
    t = vdb.IVFSQ8Index(64, 48, "l2", 0)
    t.train(X)
    lor_all = oracle.ivf_assign(t.centroids(), X, "l2")
    vmin, vdiff = np_ranges(X, t.centroids(), lor_all)
    np.testing.assert_array_equal(t.ranges()[0], vmin)
    np.testing.assert_array_equal(t.ranges()[1], vdiff)
    for h in (idx, one, t):
        h.close()


def test_footprint(vdb):
    rng = np.random.default_rng(9)
    n, d = 200000, 128
    X = rng.standard_normal((n, d)).astype(F32)
    C = X[rng.choice(n, 64, replace=False)].copy()
    sq = vdb.IVFSQ8Index(d, 64, "l2", 0)
    sq.set_centroids(C)
    sq.train_ranges(X)
    sq.add(X)
    s = sq.stats()
    sq_bytes = s["bytes_resident"] - s["bytes_workspace"]
    fl = vdb.IVFFlatIndex(d, 64, "l2", 0)
    fl.set_centroids(C)
    fl.add(X)
    f = fl.stats()
    fl_bytes = f["bytes_resident"] - f["bytes_workspace"]
    print(f"SQ8 {sq_bytes / (4 * n * d):.3f} x the float32 corpus, IVF-Flat {fl_bytes / (4 * n * d):.3f} x")
    assert sq_bytes <= 0.6 * 4 * n * d, s
    assert fl_bytes >= 3 * sq_bytes, (f, s)
    sq.close()
    fl.close()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_plugins_reference_yaml_shape(vdb, metric):
    from vdbhip.algorithms import _safe_normalize

    X, Q = _data(20000, 64, 60, seed=13)
    algo = vdb.CompositeAlgorithm("ivf_sq8", 64,
                                  indexer={"type": "HipFactoryIndexer", "metric": metric, "index_key": "IVF64,SQ8",
                                           "nprobe": 4},
                                  searcher={"type": "HipIVFSearcher", "metric": metric, "nprobe": 8}, metric=metric)
    algo.build_index(X)
    D, I = algo.batch_search(Q, k=10)
    assert algo.searcher.index.nprobe == 8 and isinstance(algo.searcher.index, vdb.IVFSQ8Index)
    cos = metric == "cosine"
    ref = vdb.IVFSQ8Index(64, 64, "ip" if cos else "l2", 0)
    ref.train(_safe_normalize(X) if cos else X)
    ref.add(_safe_normalize(X) if cos else X)
    ref.set_nprobe(8)
    Dr, Ir = ref.search(_safe_normalize(Q) if cos else Q, 10)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, -Dr if cos else Dr)
    ref.close()


def test_approximate_search_raw_conventions(vdb):
    X, Q = _data(20000, 64, 30, seed=17)
    for metric in ("l2", "ip"):
        algo = vdb.HipApproximateSearch("sq8", 64, index_type="IVF64,SQ8", metric=metric, nprobe=6)
        algo.build_index(X)
        D, I = algo.batch_search(Q, 10)
        ref = vdb.IVFSQ8Index(64, 64, metric, 0)
        ref.train(X)
        ref.add(X)
        ref.set_nprobe(6)
        Dr, Ir = ref.search(Q, 10)
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)
        assert algo.get_memory_usage() > 0
        ref.close()
    with pytest.raises(ValueError):
        vdb.HipApproximateSearch("pq", 64, index_type="IVF32,PQ8")


def test_persistence_round_trip(vdb, tmp_path):
    X, Q = _data(8000, 64, 25, seed=19)
    algo = vdb.HipApproximateSearch("sq8", 64, index_type="IVF32,SQ8", metric="l2", nprobe=5)
    algo.build_index(X)
    D, I = algo.batch_search(Q, 10)
    algo.save_index(str(tmp_path / "a"))
    assert json.loads((tmp_path / "a" / "manifest.json").read_text())["format"] == "vdbhip-ivfsq8-v1"
    back = vdb.HipApproximateSearch("sq8", 64, index_type="IVF32,SQ8", metric="l2", nprobe=5)
    back.load_index(str(tmp_path / "a"))
    np.testing.assert_array_equal(back.index.codes(), algo.index.codes())
    for a, b in zip(back.index.ranges(), algo.index.ranges()):
        np.testing.assert_array_equal(a, b)
    D2, I2 = back.batch_search(Q, 10)
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    flat = vdb.HipApproximateSearch("f", 64, index_type="IVF32,Flat", metric="l2", nprobe=5)
    with pytest.raises(ValueError, match="format"):
        flat.load_index(str(tmp_path / "a"))


def test_refusals_leave_the_index_usable(vdb):
    from vdbhip import _ffi

    X, Q = _data(6000, 32, 12, seed=23)
    C = X[:16].copy()
    idx = _sq8(vdb, X, C, "l2")
    idx.set_nprobe(4)
    D0, I0 = idx.search(Q, 5)
    lib = _ffi.load()
    assert lib.vdb_ivf_set_codec(idx._h, 0) == _ffi.VDB_ERR_STATE        # rows exist
    assert "before centroids or rows" in _ffi.last_error()
    with pytest.raises(_ffi.VdbError, match="SQ8"):
        idx.set_option("graph", 1)
    with pytest.raises(_ffi.VdbError, match="SQ8"):
        idx.set_option("int8_only", 1)
    with pytest.raises(ValueError, match="id_base"):
        idx.add(X[:10], id_base=5)                                          # appends keep the index's id base
    assert lib.vdb_add(idx._h, _ffi.ptr(X), 10, 0) == _ffi.VDB_ERR_UNSUPPORTED
    bad = np.zeros(10, np.int32)
    bad[3] = 16
    with pytest.raises(ValueError, match="row could not be assigned to a list"):    # (checked before the add touches the handle)
        idx.add(X[:10], id_base=1000, list_of_row=bad)
    D1, I1 = idx.search(Q, 5)
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1, D0)
    assert idx.stats()["ntotal"] == len(X)
    idx.close()
    # the codec on a multi-device handle (two shards on GPU 0)
    h = _ffi.create_handle(32, 0, [0, 0])
    try:
        assert lib.vdb_ivf_set_codec(h, 1) == _ffi.VDB_ERR_UNSUPPORTED
        assert "multi-device" in _ffi.last_error()
    finally:
        lib.vdb_destroy(h)
    with pytest.raises(ValueError, match="one GPU"):
        vdb.IVFSQ8Index(32, 16, "l2", device=[0, 0])


def test_published_random_ivf_sq8_recall_point(vdb, golden_dir):
    from vdbhip import datasets, harness
    from vdbhip.metrics import recall_at_k

    man = json.loads((golden_dir / "manifest.json").read_text())["published_points"]["random_ivf_flat"]
    pub = json.loads((golden_dir / "ivf_sq8_published.json").read_text())
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
    topk, nprobe, key = pub["topk"], pub["nprobe"], pub["index_type"]
    nlist = vdb.parse_index_key(key)[0]
    r10s, r1s = [], []
    for seed in [1234] + list(range(1, 10)):
        sq = vdb.IVFSQ8Index(opt["dimensions"], nlist, "l2", 0)
        sq.train(train, seed=seed)
        sq.add(train)
        sq.set_nprobe(nprobe)
        _, i_sq = sq.search(q, topk)
        r10s.append(recall_at_k(g, i_sq, 10))
        r1s.append(recall_at_k(g, i_sq, 1))
        if seed == 1234:        # IVF-Flat on the same centroids and nprobe: SQ8 costs at most 0.02 of recall@10
            fl = vdb.IVFFlatIndex(opt["dimensions"], nlist, "l2", 0)
            fl.set_centroids(sq.centroids())
            fl.add(train)
            fl.set_nprobe(nprobe)
            _, i_fl = fl.search(q, topk)
            assert abs(recall_at_k(g, i_fl, 10) - r10s[0]) <= 0.02, (recall_at_k(g, i_fl, 10), r10s[0])
            fl.close()
        sq.close()
    print(f"published recall@10 {pub['recall@10']:.4f} / recall@1 {pub['recall@1']:.4f}; own k-means seed 1234: "
          f"{r10s[0]:.4f} / {r1s[0]:.4f}; ten seeds: recall@10 {min(r10s):.4f}..{max(r10s):.4f}, "
          f"recall@1 {min(r1s):.4f}..{max(r1s):.4f}")
    assert abs(r10s[0] - pub["recall@10"]) <= pub["tolerance_recall@10"], r10s
    assert abs(r1s[0] - pub["recall@1"]) <= pub["tolerance_recall@1"], r1s
    assert abs(float(np.mean(r10s)) - pub["recall@10"]) <= pub["tolerance_mean_recall@10"], r10s

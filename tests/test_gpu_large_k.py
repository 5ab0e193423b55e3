"""Every path that ends in the wave top-k, at the list widths no other test runs: k = 257 ... 512 (8 registers per lane) and
k = 1025 ... 2048 (32), and both sides of every gate that depends on k.

End to end against `oracle.knn` / `oracle.ivf_search`; the re-rank against np.lexsort over `oracle.pair_keys`.  Exact
comparisons (ids and float32 distances).  Each test asserts through `stats()` the path it means to reach.  The gates, as the
code has them (search_flat.inc, ivf.inc, vdbhip.hip):

  * `search_batch` offers the MFMA scan up to k = 1024, and only while `scan_geometry` or `scan_geometry_direct` can give
    4k superbins: at 131 072 rows, D = 32, that ends at k = 512 (2048 bins of 64 rows), restated below;
  * `search_exact` takes the 4-queries-per-wave kernel for kpl_for(k) <= 2, i.e. k <= 128;
  * `search_dense` takes `dense_select_reg_kernel` for kpl_for(k) <= 4 AND at most 2048 padded rows; a 4096-row corpus runs
    `dense_select_kernel<KPL>` at every k, so the crossing between the two is tested at 2048 rows, k = 256 / 257; the dense
    path ends at k = 1024 and at 2k = N;
  * the IVF list-major scan serves k <= 256 only, and only while the probed lists give 4k bins: 20 000 rows in 32 lists are
    too few for k = 256 (the exact list scan `ivf_scan_kernel<KPL>` serves them), 80 000 rows reach it;
  * `vdb_rerank`, the partial search + merge and the multi-device handle accept k <= 2048.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(F32)


def _bytes(rng, n, d):
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(F32)


def _make(kind, seed, n, d, nq):
    rng = np.random.default_rng(seed)
    f = _bytes if kind == "bytes" else _gauss
    return f(rng, n, d), f(rng, nq, d)


def _flat(vdb, X, metric, id_base=0, device=0, **opts):
    idx = vdb.FlatIndex(X.shape[1], metric, device)
    for name, value in opts.items():
        idx.set_option(name, value)
    idx.add(X, id_base=id_base)
    return idx


def _equal(got, want, msg=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)


# ---- exhaustive kernel -----------------------------------------------------------------------------------------------------
LARGE_KS = (1024, 1025, 2047, 2048)


@pytest.mark.parametrize("kind", ["gauss", "bytes"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_exhaustive_scan_large_k(vdb, oracle, metric, kind):
    """40 000 rows, 5 queries: 64 splits of 640 rows, fewer than k each, so merge_splits merges padded lists with 32 (k = 1024:
    16) registers per lane.  The byte-valued corpus (D = 8) has real ties, inside the list and at its end.  id_base != 0."""
    X, Q = _make(kind, 11, 40_000, 8 if kind == "bytes" else 16, 5)
    idx = _flat(vdb, X, metric, id_base=1000, force_path=1)
    for k in LARGE_KS:
        got = idx.search(Q, k)
        assert idx.stats()["last_path_name"] == "exact_scan"
        _equal(got, oracle.knn(X, Q, k, metric, id_base=1000), f"k={k}")
        if kind == "bytes":
            assert (np.diff(got[0], axis=1) == 0).any()
    idx.close()


@pytest.mark.parametrize("kind", ["gauss", "bytes"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_exhaustive_scan_large_k_small_corpora(vdb, oracle, metric, kind):
    """One query; 3000 rows (k of them returned), N = k, N = k - 1 and N = 1500 < k (padding)."""
    X, Q = _make(kind, 12, 3000, 8 if kind == "bytes" else 16, 1)
    for k in LARGE_KS:
        for n in (3000, k, k - 1, 1500):
            idx = _flat(vdb, X[:n], metric, id_base=5, force_path=1)
            got = idx.search(Q, k)
            assert idx.stats()["last_path_name"] == "exact_scan"
            idx.close()
            _equal(got, oracle.knn(X[:n], Q, k, metric, id_base=5), f"k={k} n={n}")
            assert (got[1] == -1).sum() == max(0, k - n)


@pytest.mark.parametrize("metric,kind", [("l2", "gauss"), ("ip", "bytes")])
def test_four_queries_per_wave_gate(vdb, oracle, metric, kind):
    """force_path = 1, 600 queries on 40 000 rows: the query-blocked exhaustive kernel (4 queries per wave, 1 or 2 registers per
    lane) up to k = 128, the one-query kernel from k = 129 on."""
    X, Q = _make(kind, 13, 40_000, 16, 600)
    idx = _flat(vdb, X, metric, force_path=1)
    for k in (64, 65, 128, 129):
        got = idx.search(Q, k)
        assert idx.stats()["last_path_name"] == "exact_scan"
        _equal(got, oracle.knn(X, Q, k, metric), f"k={k}")
    idx.close()


# ---- the scan's k gate -----------------------------------------------------------------------------------------------------
def _scan_serves(n, d, k, nq):
    """search_batch + scan_geometry + scan_geometry_direct (search_flat.inc) for a D <= 128 flat index under force_path = 2:
    does the MFMA scan serve this k?"""
    assert d <= 128
    if k > 1024:
        return False
    G, span, bin_rows = 2, 512, 256
    npad = (n + span - 1) // span * span
    nspans = npad // (G * bin_rows)
    if nspans * G < 16:
        return False
    spc_hi = nspans * G // (4 * k)
    spc_lo = (nspans * G + 1023) // 1024
    if spc_hi >= 1 and spc_hi >= spc_lo:
        spc_want = 32 // G
        if nq <= 512:
            spc_want = max(1, min(spc_want, nspans // 512))
        spc = max(min(spc_want, spc_hi), spc_lo)
        if spc < 2 and nspans * G >= 128:
            spc = min(2, spc_hi)
        nchunks = (nspans + spc - 1) // spc
        if nchunks >= 16:
            n8 = (nchunks + 7) // 8 * 8
            if n8 * G <= 1024 and nspans // n8 >= 1:
                nchunks = n8
        cap = 256 // G
        if nq > 512 and cap < nchunks <= 2 * cap and cap * G >= 4 * k:
            nchunks = cap
        if nspans // nchunks >= 1 and G * nchunks <= 16 * 64:
            return True
    for rows in (128, 64):
        nb = nspans * G * (bin_rows // rows)
        if 4 * k <= nb <= 2048:
            return True
    return False


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_scan_k_gate(vdb, oracle, metric):
    """131 072 rows, D = 32, force_path = 2: the scan serves k up to 512 (direct bins of 64 rows) and hands k = 513 to the
    exhaustive kernel; k = 300 and 512 run refine_tail_kernel with 8 registers per lane.  The restatement and stats() must agree."""
    n, d, nq = 131_072, 32, 16
    kmax = max(k for k in range(1, 1100) if _scan_serves(n, d, k, nq))
    assert kmax == 512 and not _scan_serves(n, d, kmax + 1, nq)
    X, Q = _make("gauss", 14, n, d, nq)
    idx = _flat(vdb, X, metric, force_path=2)
    for k in (300, kmax, kmax + 1):
        got = idx.search(Q, k)
        st = idx.stats()
        want_path = "mfma_scan" if _scan_serves(n, d, k, nq) else "exact_scan"
        assert st["last_path_name"] == want_path, (k, st)       # (a disagreement is a failure of the restatement: fix it, do not skip)
        _equal(got, oracle.knn(X, Q, k, metric), f"k={k}")
    idx.close()


# ---- dense path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_dense_path_k_gates(vdb, oracle, metric):
    """64 queries, D = 64.  4096 rows: dense_select_kernel<4 | 8 | 16> (k = 256, 257 / 512, 1024).  2048 rows: the register select
    at k = 256, dense_select_kernel<8> at 257, and k = 1024 with 2k = N still dense.  2047 rows, k = 1024: 2k > N, exhaustive."""
    X, Q = _make("gauss", 15, 4096, 64, 64)
    for n, ks, path in ((4096, (256, 257, 512, 1024), "mfma_scan"), (2048, (256, 257, 1024), "mfma_scan"), (2047, (1024,), "exact_scan")):
        idx = _flat(vdb, X[:n], metric)
        for k in ks:
            got = idx.search(Q, k)
            st = idx.stats()
            assert st["last_path_name"] == path, (n, k, st)
            _equal(got, oracle.knn(X[:n], Q, k, metric), f"n={n} k={k}")
        idx.close()


# ---- partial search + merge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_partial_search_and_merge_large_k(vdb, oracle, metric):
    """Three unequal shards of 30 000 rows, one of them (400 rows) smaller than k: merged == unsharded == oracle."""
    import torch

    dev = torch.device("cuda", 0)
    X, Q = _make("bytes", 16, 30_000, 24, 6)
    q_t = torch.from_numpy(Q).to(dev)
    bounds = [0, 400, 17_000, 30_000]
    full = _flat(vdb, X, metric)
    shards = [_flat(vdb, X[bounds[p]:bounds[p + 1]], metric, id_base=bounds[p]) for p in range(3)]
    for k in (513, 2048):
        want = oracle.knn(X, Q, k, metric)
        _equal(full.search(Q, k), want, f"unsharded k={k}")
        pack = torch.empty((3, 2, len(Q), k), dtype=torch.int64, device=dev)
        for p, s in enumerate(shards):
            s.search_partial_device(q_t.data_ptr(), len(Q), k, pack[p, 0].data_ptr(), pack[p, 1].data_ptr())
        D = torch.empty((len(Q), k), dtype=torch.float32, device=dev)
        I = torch.empty((len(Q), k), dtype=torch.int64, device=dev)
        vdb.merge_packed_partials_device(metric, 0, pack.data_ptr(), 3, len(Q), k, D.data_ptr(), I.data_ptr())
        torch.cuda.synchronize()
        _equal((D.cpu().numpy(), I.cpu().numpy()), want, f"packed k={k}")
        keys, ids = pack[:, 0].contiguous().view(torch.float64), pack[:, 1].contiguous()
        assert (ids[0, :, 400:] == -1).all() and torch.isinf(keys[0, :, 400:]).all()       # the small shard's list is padded
        D.zero_()
        I.zero_()
        vdb.merge_partials_device(metric, 0, keys.data_ptr(), ids.data_ptr(), 3, len(Q), k, D.data_ptr(), I.data_ptr())
        torch.cuda.synchronize()
        _equal((D.cpu().numpy(), I.cpu().numpy()), want, f"split k={k}")
    for s in shards + [full]:
        s.close()


# ---- re-rank ---------------------------------------------------------------------------------------------------------------
def _rerank_reference(oracle, X, Q, cand, k, metric, id_base):
    """Top k by (canonical float64 key, id) among the candidates that name a row of the index."""
    n = len(X)
    ok = (cand >= id_base) & (cand < id_base + n)
    rows = np.where(ok, cand - id_base, 0)
    keys = oracle.pair_keys(X, Q, rows, metric)
    fmax = np.finfo(F32).max
    D = np.full((len(Q), k), fmax if metric == "l2" else -fmax, F32)
    I = np.full((len(Q), k), -1, np.int64)
    for q in range(len(Q)):
        kq, iq = keys[q][ok[q]], cand[q][ok[q]]
        o = np.lexsort((iq, kq))[:k]
        D[q, :len(o)] = (kq[o] if metric == "l2" else -kq[o]).astype(F32)
        I[q, :len(o)] = iq[o]
    return D, I


def _candidates(rng, nq, ncand, n, id_base, must=()):
    """Distinct rows per query (the rows `must` among them when they fit), then holes (-1) and ids outside
    [id_base, id_base + n) on both sides."""
    must = np.asarray(must, np.int64)
    rest = np.setdiff1d(np.arange(n), must)
    cand = np.stack([rng.permutation(np.concatenate([must, rng.permutation(rest)])[:ncand]) if len(must) <= ncand
                     else rng.permutation(n)[:ncand] for _ in range(nq)]).astype(np.int64) + id_base
    r = rng.random(cand.shape)
    cand[r < 0.10] = -1
    out = (r >= 0.10) & (r < 0.15)
    cand[out] = np.where(rng.random(int(out.sum())) < 0.5, id_base - 1 - rng.integers(0, 50, int(out.sum())),
                         id_base + n + rng.integers(0, 50, int(out.sum())))
    return cand


@pytest.fixture(scope="module", params=["default-d40", "default-d200", "int8_only-d40"])
def rerank_index(request, vdb):
    kind = request.param
    rng = np.random.default_rng(17)
    if kind == "int8_only-d40":
        n, d, id_base = 33_000, 40, 9
        X, Q = _bytes(rng, n, d), _bytes(rng, 4, d)
    else:
        n, d, id_base = 4000, int(kind.split("-d")[1]), 77
        X, Q = _gauss(rng, n, d), _gauss(rng, 4, d)
    X[n // 2:n // 2 + 600] = X[:600]                 # duplicate rows: equal keys, the smaller id wins
    opts = {"int8_only": 1} if kind.startswith("int8") else {}
    idx = _flat(vdb, X, "l2", id_base=id_base, **opts)
    if opts:
        assert idx.stats()["has_i8_copy"] == 2, "the int8_only build did not take effect"
    yield kind, X, Q, id_base, idx
    idx.close()


@pytest.mark.parametrize("k", [64, 65, 1025, 2048])
def test_rerank_large_k(vdb, oracle, rerank_index, k):
    """ncand = k - 1 (padding), k and 3000; holes, foreign ids and duplicate rows among the candidates."""
    kind, X, Q, id_base, idx = rerank_index
    rng = np.random.default_rng(k)
    for ncand in (k - 1, k, 3000):
        half = len(X) // 2
        dup = np.concatenate([np.arange(150), half + np.arange(150)])
        cand = _candidates(rng, len(Q), ncand, len(X), id_base, must=dup)
        got = idx.rerank(Q, cand, k)
        want = _rerank_reference(oracle, X, Q, cand, k, "l2", id_base)
        _equal(got, want, f"{kind} k={k} ncand={ncand}")
        assert (want[1] == -1).any() or ncand > k
        if ncand == 3000 and k >= 1025:                   # both copies of a duplicated row made the list, smaller id first
            pos = {int(i): j for j, i in enumerate(got[1][0])}
            pairs = [(i, i + half) for i in range(id_base, id_base + 150) if i in pos and i + half in pos]
            assert pairs and all(pos[a] < pos[b] and got[0][0][pos[a]] == got[0][0][pos[b]] for a, b in pairs)


@pytest.mark.parametrize("k", [65, 2048])
def test_rerank_large_k_ip(vdb, oracle, k):
    rng = np.random.default_rng(18)
    X, Q = _gauss(rng, 4000, 40), _gauss(rng, 3, 40)
    idx = _flat(vdb, X, "ip", id_base=3)
    for ncand in (k - 1, k, 3000):
        cand = _candidates(rng, len(Q), ncand, len(X), 3)
        _equal(idx.rerank(Q, cand, k), _rerank_reference(oracle, X, Q, cand, k, "ip", 3), f"k={k} ncand={ncand}")
    idx.close()


# ---- IVF-Flat --------------------------------------------------------------------------------------------------------------
def _ivf(vdb, X, nlist, metric):
    C = X[:nlist].copy()
    idx = vdb.IVFFlatIndex(X.shape[1], nlist, metric, 0)
    idx.set_centroids(C)
    idx.add(X)
    return idx, C, idx.assignment()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivf_large_k(vdb, oracle, metric):
    """20 000 rows in 32 lists, injected centroids, nprobe 4 and 32, k = 256, 257 and 2048: `ivf_scan_kernel<4 | 8 | 32>` (the
    probed lists are too few for the list-major scan at these k).  With 4 probes some queries find fewer than 2048 rows."""
    X, Q = _make("gauss", 19, 20_000, 32, 40)
    idx, C, lor = _ivf(vdb, X, 32, metric)
    for nprobe in (4, 32):
        idx.set_nprobe(nprobe)
        for k in (256, 257, 2048):
            got = idx.search(Q, k)
            st = idx.stats()
            assert st["last_path_name"] == "ivf" and st["last_candidates"] == 0, st      # (the exact list scan: no candidates)
            _equal(got, oracle.ivf_search(X, C, lor, Q, k, nprobe, metric), f"nprobe={nprobe} k={k}")
            if k == 2048:
                assert (got[1] == -1).any() == (nprobe == 4)
    idx.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivf_list_major_k_gate(vdb, oracle, metric):
    """80 000 rows in 32 lists, 32 probes: about 1300 bins of 64 rows per query, enough for the list-major scan at its last k, 256
    (`last_candidates > 0`); k = 257 takes the exact list scan."""
    X, Q = _make("gauss", 20, 80_000, 16, 64)
    idx, C, lor = _ivf(vdb, X, 32, metric)
    idx.set_nprobe(32)
    for k in (256, 257):
        got = idx.search(Q, k)
        st = idx.stats()
        print(f"ivf k={k}: {st}")
        assert st["last_path_name"] == "ivf" and (st["last_candidates"] > 0) == (k == 256), st
        _equal(got, oracle.ivf_search(X, C, lor, Q, k, 32, metric), f"k={k}")
    idx.close()


# ---- multi-device handle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_multi_device_handle_k2048(vdb, oracle, metric):
    """vdb_create_multi over [0, 0, 0], 20 000 rows, k = 2048: search and re-rank equal the single-device handle (and the oracle)."""
    X, Q = _make("bytes", 21, 20_000, 16, 5)
    one = _flat(vdb, X, metric, id_base=11)
    multi = _flat(vdb, X, metric, id_base=11, device=[0, 0, 0])
    assert multi.stats()["ndevices"] == 3
    want = oracle.knn(X, Q, 2048, metric, id_base=11)
    _equal(one.search(Q, 2048), want, "single")
    _equal(multi.search(Q, 2048), want, "multi")
    rng = np.random.default_rng(22)
    cand = _candidates(rng, len(Q), 3000, len(X), 11)
    ref = _rerank_reference(oracle, X, Q, cand, 2048, metric, 11)
    _equal(one.rerank(Q, cand, 2048), ref, "single rerank")
    _equal(multi.rerank(Q, cand, 2048), ref, "multi rerank")
    one.close()
    multi.close()

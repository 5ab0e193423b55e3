"""tests/census.py on the host: the Gram-matrix reference against the CPU oracle, the invariants of the corpora, and the restated
scan geometry against the one test_gpu_scan_i8_pipelined.py keeps for its own cases."""
from __future__ import annotations

import numpy as np
import pytest

from tests import census
from tests.test_gpu_scan_i8_pipelined import _geometry as pipelined_geometry

N, SEED = 1500, 3


def _dim(kind):
    return {"bytes": 64, "wide": 128, "gauss": 48}[kind]


@pytest.mark.parametrize("k", [1, 2, 40])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("kind", census.KINDS)
def test_gram_topk_equals_oracle(oracle, kind, metric, k):
    d = _dim(kind)
    X = census.corpus(kind, N, d, SEED)
    _, pair = census.multiset(kind, d, SEED)
    T, _ = census.twins(X, 64, pair)
    rows = np.arange(0, N, 7)
    for C in (X, T):
        D, I = census.gram_topk(C, rows, k, metric)
        Do, Io = oracle.knn(C, C[rows], k, metric)
        np.testing.assert_array_equal(I, Io)
        if census.is_integer_kind(C):
            np.testing.assert_array_equal(D, Do)
        else:       # (float64 Gram keys against the oracle's canonical arithmetic: the ids are what the reference is used for)
            np.testing.assert_allclose(D, Do, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_gram_topk_tie_at_the_kth_place(oracle, metric):
    """Rows 900, 5 and 311 are the same swap of row 40, so places 2..4 of query 40 tie: k = 2 and k = 3 cut through the tie and keep
    the smaller ids."""
    X = census.corpus("bytes", N, 64, SEED)
    _, pair = census.multiset("bytes", 64, SEED)
    X[[900, 5, 311]] = census._swap_pair(X, np.array([40, 40, 40]), pair)
    rows = np.array([40, 5, 311, 900, 41])
    for k in (1, 2, 3, 4, 5):
        D, I = census.gram_topk(X, rows, k, metric)
        Do, Io = oracle.knn(X, X[rows], k, metric)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
    _, I = census.gram_topk(X, rows[:1], 3, metric)
    assert I.tolist() == [[40, 5, 311]]


@pytest.mark.parametrize("kind", census.KINDS)
def test_corpus_invariants(kind):
    d = _dim(kind)
    X = census.corpus(kind, N, d, SEED)
    ms, pair = census.multiset(kind, d, SEED)
    assert len(np.unique(X, axis=0)) == N
    np.testing.assert_array_equal(np.sort(X, axis=1), np.broadcast_to(np.sort(ms), X.shape))      # one multiset: equal norms
    if kind == "gauss":
        n2 = (X.astype(np.float64) ** 2).sum(axis=1)
        assert np.ptp(n2) <= 1e-9 * n2.max()
        assert not census.is_integer_kind(X)
    else:
        assert len(set((X.astype(np.int64) ** 2).sum(axis=1).tolist())) == 1
    if kind == "bytes":
        assert X.min() >= 0 and X.max() <= 255
    if kind == "wide":
        assert X.min() < -128 and X.max() > 127


@pytest.mark.parametrize("mask", census.MASKS + ("mixed",))
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("kind", census.KINDS)
def test_twins_are_the_second_neighbours(kind, metric, mask):
    d = _dim(kind)
    n = 2100 if mask == "mixed" else N          # (mixed: more than one 2048-row block)
    X = census.corpus(kind, n, d, SEED)
    _, pair = census.multiset(kind, d, SEED)
    T, p = census.twins_mixed(X, pair) if mask == "mixed" else census.twins(X, mask, pair)
    r = np.arange(n)
    has = p >= 0
    np.testing.assert_array_equal(p[p[has]], r[has])            # an involution
    assert has.sum() >= n - 1024              # rows whose partner lies past the corpus stay single
    if mask != "mixed":
        np.testing.assert_array_equal(p[has], r[has] ^ mask)
    np.testing.assert_array_equal(np.sort(T, axis=1), np.sort(X, axis=1))          # the swap keeps the multiset
    D, I = census.gram_topk(T, r, 2, metric)
    np.testing.assert_array_equal(I[:, 0], r)
    np.testing.assert_array_equal(I[has, 1], p[has])
    if kind != "gauss":
        n2 = float((T[0].astype(np.float64) ** 2).sum())
        np.testing.assert_array_equal(D[has], np.broadcast_to(np.float32([0, 2] if metric == "l2" else [n2, n2 - 1]), (has.sum(), 2)))
        # a single row's second neighbour is some other permutation: at least as far as a swap, in practice far away
        assert (D[~has, 1] >= 2).all() if metric == "l2" else (D[~has, 1] <= n2 - 1).all()


def test_stride_order_is_a_permutation():
    o = census.stride_order(17409, 4099)
    assert sorted(o.tolist()) == list(range(17409)) and o[1] == 4099


@pytest.mark.parametrize("n,nq,spc", [(127_900, 2048, 2), (131_072, 2048, 2), (70_001, 1100, 0)])
def test_restated_geometry_matches_the_pipelined_scan_tests(n, nq, spc):
    nspans, starts = pipelined_geometry(n, nq, spc, k=10)
    for d in (64, 128):
        g = census.scan_geometry(n, d, 10, nq, spc)
        assert g.ok and g.nspans == nspans and g.starts == starts and g.direct_rows == 0
    assert census.wide_tiles(len(starts) - 1, nq) == (spc == 2)


def test_restated_geometry_shapes():
    # 1024-row spans above D = 128, four bins each
    g = census.scan_geometry(20_011, 192, 1, 40)
    assert g.ok and g.nspans == 20 and census.bins_per_span(192) == 4
    # the standard geometry declines when 4 k superbins do not fit: direct bins of 128 rows, then of 64
    assert census.scan_geometry(17_409, 64, 17, 700).ok and not census.scan_geometry(17_409, 64, 18, 700).ok
    assert census.geometry(17_409, 64, 18, 700).direct_rows == 128 and census.geometry(17_409, 64, 35, 700).direct_rows == 128
    assert census.geometry(17_409, 64, 36, 700).direct_rows == 64 and census.geometry(17_409, 64, 70, 700).direct_rows == 64
    assert not census.geometry(17_409, 64, 71, 700).ok
    assert [census.nw_small(q) for q in (40, 64, 65, 128, 256, 257, 700)] == [1, 1, 2, 2, 4, 8, 8] and census.nw_small(40, 0) == 8


@pytest.mark.parametrize("kind", ["bytes", "wide"])
def test_case_reference_serves_both_metrics(oracle, kind):
    """Case.ref derives the L2 distances from the inner products of one Gram pass (equal norms): same as gram_topk under L2, and as
    the oracle."""
    c = census.case(kind, 2100, 64, SEED)
    for which in ("plain", "twin", "twin2"):
        for metric in ("l2", "ip"):
            D, I = c.ref(which, metric, 3)
            Dg, Ig = census.gram_topk(c.rows(which), np.arange(c.n), 3, metric)
            np.testing.assert_array_equal(I, Ig)
            np.testing.assert_array_equal(D, Dg)
            s = census.sample_rows(c.n)
            Do, Io = oracle.knn(c.rows(which), c.rows(which)[s], 3, metric)
            np.testing.assert_array_equal(I[s], Io)
            np.testing.assert_array_equal(D[s], Do)
    for which in ("twin", "twin2"):
        has = c.partner(which) >= 0
        np.testing.assert_array_equal(c.ref(which, "l2", 2)[1][has, 1], c.partner(which)[has])
    assert (c.partner("twin") != c.partner("twin2")).any()
    np.testing.assert_array_equal(census.mixed_masks(5000, 1)[[0, 2048, 4096]], census.MASKS[1:4])
    # the launch rules restated next to the geometry
    assert not census.exact_blocked(256, 9001, 1) and census.exact_blocked(1024, 9001, 1) and not census.exact_blocked(1024, 9001, 1, 3)
    assert not census.exact_blocked(1024, 9001, 200) and not census.exact_blocked(4, 9001, 1)
    assert census.i8_batch_form(3, 24, 700, True) == (512, 8, 8, 0) and census.i8_batch_form(3, 53, 5120, True) == (1024, 8, 8, 0)
    assert census.i8_batch_form(5, 53, 5120, False) == (512, 16, 16, 0) and census.i8_batch_form(6, 53, 5120, False) == (1024, 8, 8, 1)
    assert census.i8_batch_form(6, 53, 5120, False, 4) == (1024, 8, 8, 0) and census.i8_batch_form(4, 24, 700, False) == (512, 4, 8, 0)


# ---- the coded census corpora (tests/census_coded.py) -----------------------------------------------------------------------------
from tests import census_coded as cc  # noqa: E402
from tests import pq_restatement  # noqa: E402

HOST_N = 4300                      # three 2048-row blocks: with `rot` 0 and 3 the masks 4, 8, 64 and 128, 256, 512 are dealt


def _coded_invariants(construction, kind, d, M, cb, codes, xh, p, pin0=False):
    n = len(xh)
    dsub = d // M
    assert cb.shape == (M, 256, dsub) and cb.dtype == np.float32 and codes.shape == (n, M) and codes.dtype == np.uint8
    np.testing.assert_array_equal(pq_restatement.reconstruct(codes, cb), xh)
    assert len(np.unique(xh, axis=0)) == n
    for m in range(M):
        used = np.unique(codes[:, m])
        assert used[0] == 0 and used[-1] == 255 and (used[:-1] >= 128).any(), (m, used)
        if construction == "entries":
            assert len(used) == 256
            assert len(np.unique(cb[m], axis=0)) == 256
        elif not (pin0 and m == 0):                 # the codes in use sit elsewhere in every sub-space; the decoys are far from S
            assert len(used) == M - pin0
            if m > pin0:
                assert not np.array_equal(used, np.unique(codes[:, m - 1]))
            far = np.abs(cb[m][np.setdiff1d(np.arange(256), used), 0]).min() - np.abs(cb[m][used, 0]).max()
            assert far >= (40 if kind == "int" else 8)
    n2 = (xh.astype(np.float64) ** 2).sum(axis=1)
    if kind == "int":
        assert census.is_integer_kind(xh) and len(set(n2.tolist())) == 1
        assert np.array_equal(xh.astype(np.float16).astype(np.float32), xh)
    else:
        assert not census.is_integer_kind(xh) and np.ptp(n2) <= 1e-6 * n2.max()


@pytest.mark.parametrize("rot", [0, 3])
@pytest.mark.parametrize("d,M,construction,kind", sorted({s[:4] for s in cc.PQ_SHAPES}))
def test_coded_corpora_are_census_corpora(d, M, construction, kind, rot):
    """Every (D, M, construction, kind) of the flat PQ census at 4300 rows: decoded rows pairwise distinct, equal norms, every row its
    own first and its planted twin its second neighbour under both metrics, codes 0, 255 and >= 128 in use in every sub-space, x^
    equal to the restated reconstruction."""
    p = cc.flat_partner(HOST_N, rot)
    cb, codes, xh, p = cc.build(construction, kind, d, M, p, seed=1)
    _coded_invariants(construction, kind, d, M, cb, codes, xh, p)
    has = p >= 0
    assert has.sum() > HOST_N - 1100
    for metric in ("l2", "ip"):
        D, I = census.gram_topk(xh, np.arange(HOST_N), 2, metric, margin_rows=has)
        np.testing.assert_array_equal(I[:, 0], np.arange(HOST_N))
        np.testing.assert_array_equal(I[has, 1], p[has])
        if kind == "int":
            n2 = float((xh[0].astype(np.float64) ** 2).sum())
            np.testing.assert_array_equal(D[has], np.broadcast_to(np.float32([0, 2] if metric == "l2" else [n2, n2 - 1]), (has.sum(), 2)))


@pytest.mark.parametrize("d,M,construction,kind,n", cc.PQ_SHAPES)
def test_coded_corpora_at_full_size(d, M, construction, kind, n):
    """The corpora of the GPU cases themselves: distinct rows (M = 8: 17 409 of the 40 320 permutations, drawn by twin class), the
    codes in use, the reconstruction.  (Their neighbours are asserted where the reference is made: CodedCase.ref.)"""
    c = cc.case(construction, kind, n, d, M)
    _coded_invariants(construction, kind, d, M, c.cb, c.codes, c.X, c.p)
    has = c.p >= 0
    assert has.sum() >= n - 1024 and {int(m) for m in np.unique((np.arange(n) ^ c.p)[has])} == set(census.MASKS)


@pytest.mark.parametrize("d,M,construction,kind,metrics", cc.IVFPQ_SHAPES)
def test_ivfpq_corpora(oracle, d, M, construction, kind, metrics):
    """The IVF-PQ census corpora: list sizes 0, 1, 255, 256, 257 and 1900, partners inside the lists at masks 4, 64, 256, residual rows
    that pass the flat invariants, decoded rows pairwise distinct; from the IVF oracle over the decoded rows, for every metric the
    shape runs under: EVERY row finds itself first and every paired row its twin second (8 probes of 64 lists)."""
    C, cb, codes, lor, p, xh = cc.ivfpq_corpus(d, M, construction, kind)
    sizes = np.bincount(lor, minlength=cc.IVF_NLIST)
    assert [sizes[l] for l in (0, 2, 4, 5, 6, 1)] == [0, 1, 255, 256, 257, 1900] and (sizes[8:12] == 0).all()
    has = p >= 0
    assert (lor[p[has]] == lor[has]).all() and has.sum() > len(lor) // 2
    _coded_invariants(construction, kind, d, M, cb, codes, pq_restatement.reconstruct(codes, cb), p, pin0=construction == "slots")
    assert len(np.unique(xh, axis=0)) == len(xh)
    for metric in metrics:
        _, I = oracle.ivf_search(xh, C, lor, xh, 2, 8, metric)
        np.testing.assert_array_equal(I[:, 0], np.arange(len(xh)))
        np.testing.assert_array_equal(I[has, 1], p[has])


def test_restated_panel_launches():
    """The branch every shape of the GPU cases names, from the restated launch_pq_panels / ivf_pq_panels."""
    L = {(d, M): cc.pq_panel_launch(d, M) for d, M, *_ in cc.PQ_SHAPES}
    pick = lambda d, M, *keys: tuple(L[(d, M)][k] for k in keys)  # noqa: E731
    assert pick(64, 8, "p16", "W", "vec", "table", "gy") == (False, 8, True, "lds", 1)
    assert pick(128, 32, "p16", "W", "vec", "table") == (False, 4, True, "lds")
    assert pick(100, 50, "p16", "W", "vec", "table", "partial", "pad8") == (False, 2, False, "lds", True, True)
    assert pick(50, 50, "p16", "W", "vec", "table", "pad8") == (False, 1, False, "lds", True)
    assert pick(128, 128, "p16", "W", "vec", "table", "gy") == (False, 1, True, "cache", 1)
    assert pick(384, 64, "p16", "W", "vec", "table", "slice_ks", "gy", "last") == (True, 2, True, "sliced", 3, 4, 3)
    assert pick(384, 96, "p16", "W", "vec", "table", "slice_ks", "gy", "last") == (True, 4, True, "sliced", 4, 3, 4)
    assert pick(200, 25, "p16", "W", "vec", "table", "slice_ks", "gy", "partial") == (True, 8, False, "sliced", 4, 2, True)
    assert pick(240, 16, "p16", "W", "vec", "table", "gy") == (True, 1, True, "cache", 1)
    assert pick(320, 40, "p16", "W", "vec", "table", "slice_ks", "gy", "last") == (True, 8, True, "sliced", 4, 3, 2)
    assert {v["W"] for v in L.values()} == {1, 2, 4, 8}
    assert {(v["p16"], v["vec"]) for v in L.values()} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(v["p16"], v["table"]) for v in L.values()} == {(False, "lds"), (False, "cache"), (True, "sliced"), (True, "cache")}
    I = {(d, M): cc.ivfpq_panel_launch(d, M) for d, M, *_ in cc.IVFPQ_SHAPES}
    assert I[(48, 12)] == dict(lds=True, slice_ks=4, gy=1, vec=True, pad16=False)
    assert I[(128, 64)] == dict(lds=True, slice_ks=2, gy=4, vec=True, pad16=False)
    assert I[(100, 25)] == dict(lds=True, slice_ks=2, gy=4, vec=False, pad16=True)
    assert I[(128, 2)] == dict(lds=False, slice_ks=8, gy=1, vec=False, pad16=False)


def test_restated_slab_cut():
    g = census.scan_geometry(17_409, 64, 2, 700, 2)
    assert g.nchunks == 24 and g.rem == 11
    one, three, default = cc.slab_cut(g, 64, 1), cc.slab_cut(g, 64, 3), cc.slab_cut(g, 64)
    assert len(one) == 24 and {s[3] for s in one} == {1, 2} and len(default) == 1 and default[0] == (0, 24, 0, 35)
    assert len(three) == 8 and three[3] == (9, 3, 18, 5) and three[4] == (12, 3, 23, 3) and sum(s[3] for s in three) == 35
    g = census.scan_geometry(18_443, 384, 2, 700, 2)
    assert g.nchunks == 10 and [s[1] for s in cc.slab_cut(g, 384, 3)] == [3, 3, 3, 1] and cc.slab_cut(g, 384, 3)[-1] == (9, 1, 18, 1)

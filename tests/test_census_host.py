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

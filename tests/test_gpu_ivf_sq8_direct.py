"""Option `ivf_sq8_direct`: the list-major scan of an IVF-SQ8 index reads the 8-bit codes themselves (csrc/ivf_sq8_scan.hpp).

Every search is compared bit for bit with oracle.ivf_search over the decoded rows, and with the same handle's answer under option 0
(fp16 panels converted per batch).  `scan_dtype == 4` says the new kernel served the batch.

Shapes: nlist 8 with lists of 0, 1, 511, 512, 513, 1100 and two of 11 500 rows, filed by hand -- an empty list, a one-row list, both
sides of a 512-row edge, several spans and row parts.  The (nprobe, k) pairs are those the list-major rule admits at this size (it
wants 4 k bins per query, ivf_geometry): k = 100 is admitted with all 8 lists probed, which is why two lists are long.  The centroids
of the five short lists lie far out, so that with nprobe < 8 almost no query probes a list with fewer bins than k.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.helpers import np_decode

pytestmark = pytest.mark.gpu

F32 = np.float32
ID0 = 1000
SIZES = (0, 1, 511, 512, 513, 1100, 11500, 11500)
PAIRS = ((1, 1), (1, 10), (3, 1), (3, 10), (8, 1), (8, 10), (8, 100))        # (nprobe, k)


@functools.lru_cache(maxsize=None)
def _data(d):
    rng = np.random.default_rng(d)
    lor = rng.permutation(np.repeat(np.arange(8), SIZES)).astype(np.int32)
    C = rng.standard_normal((8, d)).astype(F32)
    C[:5] += F32(6.0) * np.eye(8, d, dtype=F32)[:5]                          # the short lists: rarely a query's nearest
    X = (C[lor] + rng.standard_normal((len(lor), d))).astype(F32)
    Q = (C[rng.integers(5, 8, 600)] + rng.standard_normal((600, d))).astype(F32)
    return X, C, lor, Q


def _index(vdb, X, C, lor, metric, direct=None, adds=1):
    ix = vdb.IVFSQ8Index(X.shape[1], len(C), metric, 0, direct_codes=direct)
    ix.set_centroids(C)
    ix.train_ranges(X)
    for part in np.array_split(np.arange(len(X)), adds):
        ix.add(X[part], id_base=ID0, list_of_row=lor[part])
    return ix


def _check(ix, oracle, Xh, C, lor, Q, k, nprobe, metric, fb_cap):
    """direct == oracle == the option-0 route; the new kernel served the batch with at most fb_cap flagged queries"""
    ix.set_nprobe(nprobe)
    ix.set_option("ivf_sq8_direct", 1)
    D, I = ix.search(Q, k)
    st = ix.stats()
    Do, Io = oracle.ivf_search(Xh, C, lor, Q, k, nprobe, metric, id_base=ID0)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    assert st["scan_dtype"] == 4 and st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st
    assert st["last_fallback_queries"] <= fb_cap, st
    ix.set_option("ivf_sq8_direct", 0)
    D0, I0 = ix.search(Q, k)
    assert ix.stats()["scan_dtype"] == 2
    np.testing.assert_array_equal(I, I0)
    np.testing.assert_array_equal(D, D0)
    return st


@pytest.mark.parametrize("metric,d,adds", [(m, d, 1) for m in ("l2", "ip") for d in (50, 64, 128)] + [("l2", 50, 2), ("ip", 128, 2)])
def test_parity_with_the_oracle_and_with_the_panel_route(vdb, oracle, metric, d, adds):
    """adds == 2: the rows arrive in two adds (an append rebuilds the lists), then the two widest cases"""
    X, C, lor, Q = _data(d)
    ix = _index(vdb, X, C, lor, metric, adds=adds)
    np.testing.assert_array_equal(ix.assignment(), lor)
    Xh = np_decode(ix.codes(), C, lor, *ix.ranges())
    for nprobe, k in PAIRS if adds == 1 else PAIRS[-2:]:
        for nq in (1, 70, 600):
            _check(ix, oracle, Xh, C, lor, Q[:nq], k, nprobe, metric, fb_cap=nq // 100)
    ix.close()


def test_inputs_of_the_panel_route_test_stay_under_its_fallback_cap(vdb, oracle):
    """the corpus, queries and cap (< 50 of 1000) of test_gpu_ivf_sq8.test_mfma_list_scan_over_codes_is_used_and_exact"""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((200000, 128)).astype(F32)
    Q = rng.standard_normal((1000, 128)).astype(F32)
    C = X[np.random.default_rng(2).choice(len(X), 256, replace=False)].copy()
    for metric in ("l2", "ip"):
        ix = vdb.IVFSQ8Index(128, 256, metric, 0)
        ix.set_centroids(C)
        ix.train_ranges(X)
        ix.add(X, id_base=ID0)
        lor = ix.assignment()
        Xh = np_decode(ix.codes(), C, lor, *ix.ranges())
        for nprobe in (8, 64):
            st = _check(ix, oracle, Xh, C, lor, Q, 10, nprobe, metric, fb_cap=49)
            print(metric, nprobe, "fallback queries", st["last_fallback_queries"], "candidates", st["last_candidates"])
        ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties_are_ordered_as_the_float64_keys_order_them(vdb, oracle, metric):
    """Duplicated rows (equal keys, the smaller id first) and rows one code step apart in a dimension where |q_d| <= 2^-20 ||q||,
    decoded symmetrically about 0 there (codes 127 / 128, centroid coordinate -4 / 255), so both metrics see a gap far below the 6
    packed id bits: in one bin, across bins, across lists (lists 2 and 3 share a centroid).  No query may be flagged."""
    d, dz, n = 64, 17, 8192
    rng = np.random.default_rng(5)
    C = rng.standard_normal((4, d)).astype(F32)
    C[3] = C[2]
    C[:, dz] = F32(-4.0 / 255.0)
    lor = np.repeat(np.arange(4), n // 4).astype(np.int32)
    X = (C[lor] + rng.standard_normal((n, d))).astype(F32)
    lo, hi = F32(-4.0 + 127.6 / 255.0 * 8.0), F32(-4.0 + 128.6 / 255.0 * 8.0)
    base = np.array([4200, 4300, 4400, 4500, 4600, 4700])                     # rows of list 2
    twin = np.array([4201, 5000, 6300, 4501, 5100, 6400])                     # same bin | another bin | list 3
    X[twin] = X[base] - C[lor[base]] + C[lor[twin]]
    X[base[3:], dz] = C[2, dz] + lo                                           # the last three pairs: one code step apart
    X[twin[3:], dz] = C[2, dz] + hi
    Q = np.repeat(X[base], 4, axis=0) + F32(0.05) * rng.standard_normal((24, d)).astype(F32)
    Q[:, dz] = 0
    Q[:, dz] = (np.linalg.norm(Q, axis=1) * 2.0 ** -21).astype(F32)
    ix = vdb.IVFSQ8Index(d, 4, metric, 0, direct_codes=True)
    ix.set_centroids(C)
    ix.set_ranges(np.full(d, -4.0, F32), np.full(d, 8.0, F32))
    ix.add(X, id_base=ID0, list_of_row=lor)
    codes = ix.codes()
    assert (codes[base[3:], dz] == 127).all() and (codes[twin[3:], dz] == 128).all()
    Xh = np_decode(codes, C, lor, *ix.ranges())
    q64, a, b = Q.astype(np.float64)[::4], Xh[base].astype(np.float64), Xh[twin].astype(np.float64)
    key = (lambda x: ((x - q64) ** 2).sum(1)) if metric == "l2" else (lambda x: -(x * q64).sum(1))
    gap = key(a) - key(b)
    assert (gap[:3] == 0).all() and (gap[3:] != 0).all() and (np.abs(gap[3:]) < 2.0 ** -17 * (a[3:] ** 2).sum(1)).all(), gap
    for nprobe in (2, 4):
        ix.set_nprobe(nprobe)
        D, I = ix.search(Q, 10)
        st = ix.stats()
        Do, Io = oracle.ivf_search(Xh, C, lor, Q, 10, nprobe, metric, id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
        assert st["scan_dtype"] == 4 and st["last_candidates"] > 0 and st["last_fallback_queries"] == 0, st
    ix.close()


@pytest.mark.parametrize("scale", [1e-15, 1e15])
def test_hostile_ranges_and_an_infinite_query_stay_exact(vdb, oracle, scale):
    X, C, lor, Q = _data(64)
    ix = vdb.IVFSQ8Index(64, 8, "l2", 0, direct_codes=True)
    ix.set_centroids(C)
    ix.set_ranges(np.full(64, -4.0 * scale, F32), np.full(64, 8.0 * scale, F32))
    ix.add(X, id_base=ID0, list_of_row=lor)
    Xh = np_decode(ix.codes(), C, lor, *ix.ranges())
    ix.set_nprobe(8)
    Qi = Q[:70].copy()
    Qi[3, 5] = np.inf
    for q in (Q[:70], Qi):
        D, I = ix.search(q, 10)
        Do, Io = oracle.ivf_search(Xh, C, lor, q, 10, 8, "l2", id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
    st = ix.stats()
    assert st["scan_dtype"] == 4 and st["last_fallback_queries"] == 70, st     # the infinite query flags its whole batch
    ix.close()


def test_workspace_holds_no_panel_slab_and_a_multi_device_handle_refuses(vdb, oracle):
    X, C, lor, Q = _data(128)
    slab = sum(-(-s // 256) for s in SIZES) * 8 * 8 * 64 * 16                  # ntiles x ksteps x 64 lanes x 16 bytes
    for direct, below in ((1, True), (0, False)):
        ix = _index(vdb, X, C, lor, "l2", direct=direct)
        ix.set_nprobe(3)
        ix.search(Q[:70], 10)
        st = ix.stats()
        assert st["scan_dtype"] == (4 if direct else 2) and (st["bytes_workspace"] < slab) == below, (st, slab)
        ix.close()
    two = vdb.IVFFlatIndex(128, 8, "l2", device=[0, 0])
    with pytest.raises(Exception, match="multi-device"):
        two.set_option("ivf_sq8_direct", 1)
    two.set_option("ivf_sq8_direct", 0)
    two.set_centroids(C)
    two.add(X, id_base=ID0, list_of_row=lor)
    two.set_nprobe(8)
    D, I = two.search(Q[:70], 10)
    Do, Io = oracle.ivf_search(X, C, lor, Q[:70], 10, 8, "l2", id_base=ID0)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    two.close()

"""Option `pq_kloop`: a flat PQ<M> index of more than 128 dimensions scans its codes on the matrix cores directly (csrc/pq_kloop.hpp).

Every search is compared bit for bit, ids and distances, with oracle.knn over the decoded rows x^ (`reconstruct()`) and with the same
handle under option 0 (the panel pass of the parent commit).  `scan_dtype == 7` says the new kernel served the batch (on the parent
commit it is never 7); switched off it is 2 again.

Shapes: N = 256 * 81 = 20 736 rows are 21 p16 spans; with `spans_per_chunk` = 2 they make 11 chunks of two spans and one of one, 44
superbins >= 4 k at k = 10, so the standard geometry admits every batch (`force_path` = 2: the corpus is below the 32 768 rows at which
the scan is chosen unasked).  One (d, M) also runs at N - 1 and N + 1, and once filled by two adds.  (d, M):
  192 / 24  dsub 8: no padding                      192 / 16  dsub 12: P = 16
  132 / 22  dsub 6: Kp = 176, a K-step tail behind Kp, code rows that are no whole dwords
  136 /  8  dsub 17: P = 24                         195 / 65  dsub 3: the 256-byte code pitch
  768 / 64  sixteen K-steps
nq: 1 and 17 (NARROW, one and two column blocks), 70, 600 (two query tiles); k: 1 and 10.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, N0 = np.float32, 256 * 81
SHAPES = ((192, 24), (192, 16), (132, 22), (136, 8), (195, 65), (768, 64))
# (metric, d, M, n, adds)
CASES = [(m, d, M, N0, 1) for d, M in SHAPES for m in ("l2", "ip")] + [("l2", 192, 16, N0 - 1, 1), ("ip", 192, 16, N0 + 1, 1), ("l2", 132, 22, N0, 2)]


@functools.lru_cache(maxsize=2)
def data(d, M, n):
    rng = np.random.default_rng(1000 * d + M)
    return rng.standard_normal((M, 256, d // M)).astype(F32), rng.standard_normal((n, d)).astype(F32), rng.standard_normal((600, d)).astype(F32)


def pq_index(vdb, d, M, metric, n=N0, adds=1, **opts):
    cb, X, Q = data(d, M, n)
    ix = vdb.PQIndex(d, M, metric, 0)
    for name, value in {"force_path": 2, "spans_per_chunk": 2, **opts}.items():
        ix.set_option(name, value)
    ix.set_codebooks(cb)
    for part in np.array_split(X, adds):
        ix.add(part)
    return ix, Q


def search(ix, Q, k, kloop):
    ix.set_option("pq_kloop", kloop)
    D, I = ix.search(Q, k)
    return D, I, ix.stats()


@pytest.mark.parametrize("metric,d,M,n,adds", CASES)
def test_parity_with_the_oracle_and_option_0(vdb, oracle, metric, d, M, n, adds):
    ix, Q = pq_index(vdb, d, M, metric, n, adds)
    Do, Io = oracle.knn(ix.reconstruct(), Q, 10, metric)       # (rows of a batch are independent, k = 1 is its first column)
    for nq in (1, 17, 70, 600):
        for k in (1, 10):
            D, I, st = search(ix, Q[:nq], k, 1)
            D0, I0, s0 = search(ix, Q[:nq], k, 0)
            print(f"{metric} d{d} M{M} n{n} nq{nq} k{k}: fallback {st['last_fallback_queries']} (option 0: {s0['last_fallback_queries']}), "
                  f"candidates {st['last_candidates']} ({s0['last_candidates']})")
            assert st["scan_dtype"] == 7 and st["last_path_name"] == "mfma_scan" and st["last_candidates"] > 0, st
            assert s0["scan_dtype"] == 2 and s0["last_path_name"] == "mfma_scan", s0
            for Dx, Ix in ((Do[:nq, :k], Io[:nq, :k]), (D0, I0)):
                np.testing.assert_array_equal(I, Ix)
                np.testing.assert_array_equal(D, Dx)
            assert st["last_fallback_queries"] <= s0["last_fallback_queries"] + nq // 100, (st, s0)
    ix.close()


def test_toggling_returns_the_same_bytes_and_option_1_alone_allocates_no_slab(vdb):
    ix, Q = pq_index(vdb, 192, 24, "l2")
    twin, _ = pq_index(vdb, 192, 24, "l2")
    D1, I1, st = search(ix, Q[:70], 10, 1)
    D0, I0, s0 = search(twin, Q[:70], 10, 0)
    assert (st["scan_dtype"], s0["scan_dtype"]) == (7, 2) and st["bytes_workspace"] < s0["bytes_workspace"], (st, s0)
    for kloop in (0, 1, 0):
        D, I, _ = search(twin, Q[:70], 10, kloop)
        assert D.tobytes() == D1.tobytes() == D0.tobytes() and I.tobytes() == I1.tobytes() == I0.tobytes()
    ix.close()
    twin.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_an_infinite_a_nan_and_a_huge_query_return_what_option_0_returns(vdb, metric):
    ix, Q = pq_index(vdb, 192, 16, metric)
    Qh = Q[:70].copy()
    Qh[0, 0], Qh[1, 1], Qh[2] = np.inf, np.nan, F32(1e38)
    D, I, st = search(ix, Qh, 10, 1)
    D0, I0, _ = search(ix, Qh, 10, 0)
    assert st["scan_dtype"] == 7
    np.testing.assert_array_equal(I, I0)
    np.testing.assert_array_equal(D, D0)
    ix.close()


def test_the_adc_scan_keeps_its_batches_and_other_handles_take_the_option_without_effect(vdb, oracle):
    ix, Q = pq_index(vdb, 192, 24, "l2", pq_adc_max_batch=16)
    assert search(ix, Q[:8], 10, 1)[2]["scan_dtype"] == 3 and search(ix, Q[:17], 10, 1)[2]["scan_dtype"] == 7
    for bad in (-1, 2, 0.5):
        with pytest.raises(Exception, match="pq_kloop"):
            ix.set_option("pq_kloop", bad)
    ix.close()
    rng = np.random.default_rng(3)
    cb, X, Q = rng.standard_normal((16, 256, 8)).astype(F32), rng.standard_normal((N0, 128)).astype(F32), rng.standard_normal((70, 128)).astype(F32)
    low = vdb.PQIndex(128, 16, "l2", 0)
    low.set_option("force_path", 2)
    low.set_codebooks(cb)
    low.add(X)
    flat = vdb.FlatIndex(128, "l2", 0)
    flat.set_option("force_path", 2)
    flat.add(X)
    for idx, rows, dtype in ((low, low.reconstruct(), 2), (flat, X, 0)):
        D, I, st = search(idx, Q, 10, 1)
        Do, Io = oracle.knn(rows, Q, 10, "l2")
        assert st["scan_dtype"] == dtype and st["last_path_name"] == "mfma_scan", st
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
        idx.close()

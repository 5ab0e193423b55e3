"""Option `ivf_pq_direct`: the list-major scan of an IVF-PQ index of at most 128 dimensions decodes the product codes in LDS from a
resident fp16 table of the codebooks (csrc/ivf_pq_scan.hpp) instead of reading fp16 panels made per batch.  Every search equals, bit for
bit, oracle.ivf_search over the decoded rows x^ and the same handle's answer under option 0 (`scan_dtype` 2); `scan_dtype == 6` says
the new kernel served the batch (never on the parent commit).  Fallback cap: what option 0 flags on the same batch, plus nq // 100.
Corpus, lists and (nprobe, k) pairs of test_gpu_ivf_sq8_direct.py, seeded Gaussian codebooks.  (d, M): 128 / 64 dsub 2 (4-byte lookups),
128 / 16 dsub 8 (16-byte), 64 / 64 dsub 1 (2-byte), 48 / 8 dsub 6 (straddles the 8-dim groups, padded dims), 50 / 10 dsub 5 (D4 = 52),
66 / 22 dsub 3 (code rows that are no whole dwords: byte copies)."""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))      # (ivfpq_restatement imports its neighbour by its bare name)

from tests import ivfpq_restatement  # noqa: E402

pytestmark = pytest.mark.gpu

F32, ID0 = np.float32, 1000
SIZES = (0, 1, 511, 512, 513, 1100, 11500, 11500)
PAIRS = ((1, 1), (1, 10), (3, 1), (3, 10), (8, 1), (8, 10), (8, 100))        # (nprobe, k)
DM = ((128, 64), (128, 16), (64, 64), (48, 8), (50, 10), (66, 22))


@functools.lru_cache(maxsize=None)
def data(d, M):
    rng = np.random.default_rng(1000 * d + M)
    lor = rng.permutation(np.repeat(np.arange(8), SIZES)).astype(np.int32)
    C = rng.standard_normal((8, d)).astype(F32)
    C[:5] += F32(6.0) * np.eye(8, d, dtype=F32)[:5]                          # the short lists: rarely a query's nearest
    X = (C[lor] + rng.standard_normal((len(lor), d))).astype(F32)
    Q = (C[rng.integers(5, 8, 600)] + rng.standard_normal((600, d))).astype(F32)
    cb = rng.standard_normal((M, 256, d // M)).astype(F32)
    return X, C, lor, Q, cb


def pq_index(vdb, X, C, lor, cb, metric, direct=None, adds=1):
    ix = vdb.IVFPQIndex(X.shape[1], len(C), cb.shape[0], metric, 0, direct_codes=direct)
    ix.set_centroids(C)
    ix.set_codebooks(cb)
    for part in np.array_split(np.arange(len(X)), adds):
        ix.add(X[part], id_base=ID0, list_of_row=lor[part])
    return ix


def check(ix, Q, k, nprobe, Do, Io, extra_cap):
    """option 1 == the oracle rows (Do, Io) == option 0 on the same handle; served by the new kernel, flags <= the panel route's + extra_cap"""
    ix.set_nprobe(nprobe)
    ix.set_option("ivf_pq_direct", 0)
    D0, I0 = ix.search(Q, k)
    s0 = ix.stats()
    assert s0["scan_dtype"] == 2, s0
    ix.set_option("ivf_pq_direct", 1)
    D, I = ix.search(Q, k)
    st = ix.stats()
    print("nprobe", nprobe, "k", k, "nq", len(Q), "fallback", st["last_fallback_queries"], "panel route", s0["last_fallback_queries"])
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    np.testing.assert_array_equal(I, I0)
    np.testing.assert_array_equal(D, D0)
    assert st["scan_dtype"] == 6 and st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st
    assert st["last_fallback_queries"] <= s0["last_fallback_queries"] + extra_cap, (st, s0)


@pytest.mark.parametrize("metric,d,M,adds", [(m, d, M, 1) for m in ("l2", "ip") for d, M in DM] + [("l2", 66, 22, 2)])
def test_parity_with_the_oracle_and_with_the_panel_route(vdb, oracle, metric, d, M, adds):
    """adds == 2: the rows arrive in two adds (an append rebuilds the lists), then the two widest pairs"""
    X, C, lor, Q, cb = data(d, M)
    ix = pq_index(vdb, X, C, lor, cb, metric, adds=adds)
    np.testing.assert_array_equal(ix.assignment(), lor)
    Xh = ivfpq_restatement.decode(ix.codes(), C, lor, cb)
    for nprobe, k in PAIRS if adds == 1 else PAIRS[-2:]:
        Do, Io = oracle.ivf_search(Xh, C, lor, Q, k, nprobe, metric, id_base=ID0)      # (rows of a batch are independent: one reference)
        for nq in (1, 70, 600):
            check(ix, Q[:nq], k, nprobe, Do[:nq], Io[:nq], nq // 100)
    ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties_are_ordered_as_the_float64_keys_order_them(vdb, oracle, metric):
    """Duplicated code rows (equal keys, the smaller id first) and pairs one codebook entry apart: entries 0 and 1 of sub-space mz
    differ by 2^-14 at 0.5 in dimension dz only -- the fp16 table rounds both to 0.5 -- and |q_dz| <= 2^-20 ||q||, so the scan
    cannot separate the two rows; the guard and the exact tail must.  In one bin, across bins, across lists (2 and 3 share a centroid)."""
    d, M, n = 64, 16, 8192
    dsub, dz = d // M, 17
    mz, jz = dz // dsub, dz % dsub
    rng = np.random.default_rng(5)
    C = rng.standard_normal((4, d)).astype(F32)
    C[3] = C[2]
    C[:, dz] = 0
    cb = rng.standard_normal((M, 256, dsub)).astype(F32)
    cb[mz, 0, jz] = F32(0.5)
    cb[mz, 1] = cb[mz, 0]
    cb[mz, 1, jz] = F32(0.5 + 2.0 ** -14)
    lor = np.repeat(np.arange(4), n // 4).astype(np.int32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    codes[:, mz] = rng.integers(2, 256, n)
    base = np.array([4200, 4300, 4400, 4500, 4600, 4700])                     # rows of list 2
    twin = np.array([4201, 5000, 6300, 4501, 5100, 6400])                     # same bin | another bin | list 3
    codes[twin] = codes[base]
    codes[base[3:], mz], codes[twin[3:], mz] = 0, 1                           # the last three pairs: one entry apart
    ix = vdb.IVFPQIndex(d, 4, M, metric, 0)
    ix.set_centroids(C)
    ix.set_codebooks(cb)
    ix.add_codes(codes, lor, id_base=ID0)
    Xh = ivfpq_restatement.decode(codes, C, lor, cb)
    Q = np.repeat(Xh[base], 4, axis=0) + F32(0.05) * rng.standard_normal((24, d)).astype(F32)
    Q[:, dz] = 0
    Q[:, dz] = (np.linalg.norm(Q, axis=1) * 2.0 ** -21).astype(F32)
    q64, a, b = Q.astype(np.float64)[::4], Xh[base].astype(np.float64), Xh[twin].astype(np.float64)
    key = (lambda x: ((x - q64) ** 2).sum(1)) if metric == "l2" else (lambda x: -(x * q64).sum(1))
    gap = key(a) - key(b)
    assert (gap[:3] == 0).all() and (gap[3:] != 0).all() and (np.abs(gap[3:]) < 2.0 ** -17 * (a[3:] ** 2).sum(1)).all(), gap
    for nprobe in (2, 4):
        Do, Io = oracle.ivf_search(Xh, C, lor, Q, 10, nprobe, metric, id_base=ID0)
        check(ix, Q, 10, nprobe, Do, Io, 0)          # (expected: nobody flagged; the cap is the panel route's own count)
    ix.close()


@pytest.mark.parametrize("scale", [1e-15, 1e15])
def test_hostile_codebooks_and_an_infinite_query_stay_exact(vdb, oracle, scale):
    X, C, lor, Q, cb = data(64, 64)
    cbs = (cb.astype(np.float64) * scale).astype(F32)
    ix = pq_index(vdb, X, C, lor, cbs, "l2", direct=True)
    Xh = ivfpq_restatement.decode(ix.codes(), C, lor, cbs)
    ix.set_nprobe(8)
    Qi = Q[:70].copy()
    Qi[3, 5] = np.inf
    for q in (Q[:70], Qi):
        D, I = ix.search(q, 10)
        Do, Io = oracle.ivf_search(Xh, C, lor, q, 10, 8, "l2", id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
    st = ix.stats()
    assert st["scan_dtype"] == 6 and st["last_fallback_queries"] == 70, st     # the infinite query flags its whole batch
    ix.close()


def test_workspace_holds_no_panel_slab_and_a_multi_device_handle_refuses(vdb, oracle):
    X, C, lor, Q, cb = data(128, 64)
    slab = sum(-(-s // 256) for s in SIZES) * 8 * 8 * 64 * 16                  # ntiles x ksteps x 64 lanes x 16 bytes
    for direct, below in ((1, True), (0, False)):
        ix = pq_index(vdb, X, C, lor, cb, "l2", direct=direct)
        ix.set_nprobe(3)
        ix.search(Q[:70], 10)
        st = ix.stats()
        assert st["scan_dtype"] == (6 if direct else 2) and (st["bytes_workspace"] < slab) == below, (st, slab)
        ix.close()
    two = vdb.IVFFlatIndex(128, 8, "l2", device=[0, 0])
    with pytest.raises(Exception, match="multi-device"):
        two.set_option("ivf_pq_direct", 1)
    two.set_option("ivf_pq_direct", 0)
    two.set_centroids(C)
    two.add(X, id_base=ID0, list_of_row=lor)
    two.set_nprobe(8)
    D, I = two.search(Q[:70], 10)
    Do, Io = oracle.ivf_search(X, C, lor, Q[:70], 10, 8, "l2", id_base=ID0)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    two.close()

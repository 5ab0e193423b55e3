"""Hash-table LSH on the GPU against the NumPy restatement of the contract (tests/lsh_tables_restatement.py) and against the
recorded results of the reference's own LSH class (tests/golden/lsh_tables_*).  Keys, candidates (votes, ids, order) and the ids
of a search are compared for equality; the distances of a search are those of vdb_rerank over the same candidates, bit for bit.
Every candidate test reads the route it took from vdb_stats."""
from __future__ import annotations

import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import admission_cases as ac  # noqa: E402
import lsh_tables_restatement as ref  # noqa: E402
from lsh_tables_cases import case_data, preprocess, published_queries  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
ID_BASE = 1000
PATH_LSHT = 6


def _randn(n, d, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(F32)


def _tables(T, H, d, seed, e2, w=4.0):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((T, H, d)).astype(F32)
    b = rng.uniform(0.0, w, size=(T, H)).astype(F32) if e2 else None
    return p, b


def _index(vdb, X, p, b, w, metric="l2", id_base=ID_BASE):
    idx = vdb.FlatIndex(X.shape[1], metric, 0)
    idx.lsht_set_tables(p, b, w)
    idx.add(X, id_base=id_base)
    return idx


# ---- keys ------------------------------------------------------------------------------------------------------------------
def _special_rows(X):
    X[5] = 0
    X[6] = -0.0
    X[7:30, ::3] = -0.0
    X[30] = np.nan
    X[31, 0] = np.nan
    X[32] = 3e38                                # sums overflow to +-inf: the E2 code saturates
    X[33] = -3e38
    X[34, 0], X[35, 1] = 1e30, -1e30
    return X


@pytest.mark.parametrize("e2,T,H,d", [
    (False, 1, 1, 3), (False, 6, 16, 16), (False, 12, 32, 64), (False, 32, 33, 200), (False, 12, 40, 64), (False, 2, 64, 16),
    (True, 1, 1, 3), (True, 6, 3, 16), (True, 12, 4, 64), (True, 8, 16, 200), (True, 32, 4, 16), (True, 32, 1, 3),
    (True, 6, 5, 16), (True, 14, 9, 64), (True, 9, 13, 16), (True, 18, 7, 16)])
def test_keys_bit_exact(vdb, e2, T, H, d):
    n, w = 1003, 0.75
    X = _special_rows(_randn(n, d, seed=T * 100 + H + d))
    p, b = _tables(T, H, d, seed=H, e2=e2, w=w)
    p[0, 0] = 0                                 # a zero projection: bit set / code floor(b / w) for every finite row
    p[T - 1, H - 1, ::2] = -0.0
    want = ref.keys(X, p, b, w)
    W = ref.words_per_table(H, 1 if e2 else 0)
    idx = _index(vdb, X, p, b, w)
    keys = idx.lsht_keys()
    assert keys.dtype == np.uint32 and keys.shape == (n, T * W)
    assert np.array_equal(keys, want)
    if e2:
        codes = keys.view(np.int32).reshape(n, T, H)
        assert (codes[30] == ref.INT32_MIN).all()
        if T * H >= 8:
            assert ref.INT32_MAX in codes[32] and ref.INT32_MIN in codes[32]
    else:
        assert (keys[30] == 0).all() and (keys[5] == keys[6]).all() and (keys[5, 0] & 1) == 1
    Qs = np.concatenate([X[:48], _randn(16, d, seed=9)])        # the scan at this key width: rows as queries collide everywhere
    want_v, want_i, _ = ref.candidates(ref.keys(Qs, p, b, w), want, T, 20, ID_BASE)
    votes, ids = idx.lsht_candidates(Qs, 20)
    assert np.array_equal(ids, want_i) and np.array_equal(votes, want_v)
    assert idx.stats()["last_fallback_queries"] == 0 and (votes[:5, 0] == T).all()
    got = idx.lsht_get_tables()
    assert (got["num_tables"], got["hash_size"], got["mode"]) == (T, H, 1 if e2 else 0)
    assert got["projections"].tobytes() == p.tobytes()
    assert (got["offsets"].tobytes() == b.tobytes() and got["bucket_width"] == F32(w)) if e2 else got["offsets"] is None
    # two appends equal one add; tables installed behind the rows key the resident rows
    two = vdb.FlatIndex(d, "l2", 0)
    two.lsht_set_tables(p, b, w)
    two.add(X[:400], id_base=7)
    two.add(X[400:], id_base=7)
    assert np.array_equal(two.lsht_keys(), want)
    late = vdb.FlatIndex(d, "l2", 0)
    late.add(X)
    late.lsht_set_tables(p, b, w)
    assert np.array_equal(late.lsht_keys(), want)
    for i in (idx, two, late):
        i.close()


def test_add_device_keys_too(vdb):
    import torch

    X = _randn(5000, 24, seed=3)
    p, b = _tables(6, 3, 24, seed=4, e2=True, w=2.0)
    idx = vdb.FlatIndex(24, "l2", 0)
    idx.lsht_set_tables(p, b, 2.0)
    xd = torch.from_numpy(X).cuda()
    idx.add_device(xd.data_ptr(), 3000, id_base=5)
    idx.add_device(xd[3000:].data_ptr(), 2000, id_base=5)
    torch.cuda.synchronize()
    assert np.array_equal(idx.lsht_keys(), ref.keys(X, p, b, 2.0))
    idx.close()


# ---- candidates and search -------------------------------------------------------------------------------------------------
def _check(idx, X, Q, p, b, w, ncand, k, metric="l2", fallback=False, id_base=ID_BASE, flat=None):
    """candidates and search of `idx` against the restatement; returns (stats after the search, colliding rows per query)"""
    T = p.shape[0]
    rk, qk = ref.keys(X, p, b, w), ref.keys(Q, p, b, w)
    want_v, want_i, count = ref.candidates(qk, rk, T, ncand, id_base)
    votes, ids = idx.lsht_candidates(Q, ncand)
    st = idx.stats()
    assert votes.dtype == np.int32 and ids.dtype == np.int64 and votes.shape == ids.shape == (len(Q), ncand)
    bad = np.flatnonzero((ids != want_i).any(axis=1) | (votes != want_v).any(axis=1))
    assert bad.size == 0, (bad[:5], ids[bad[:1]], want_i[bad[:1]])
    assert st["last_path"] == PATH_LSHT and st["last_path_name"] == "lsh_tables" and st["last_nq"] == len(Q)
    assert st["last_candidates"] == int(np.minimum(count, ncand).sum()) and st["last_rows_scanned"] == 0
    D, I = idx.lsht_search(Q, k, ncand, fallback)
    st2 = idx.stats()
    want_I = ref.search(X, Q, want_i, k, metric, fallback, id_base)
    assert np.array_equal(I, want_I), np.flatnonzero((I != want_I).any(axis=1))[:5]
    D2, I2 = idx.rerank(Q, want_i, k)            # "candidates, then vdb_rerank", bit for bit
    empty = count == 0
    keep = ~empty if fallback else np.ones(len(Q), bool)
    assert D[keep].tobytes() == D2[keep].tobytes() and np.array_equal(I[keep], I2[keep])
    if fallback and empty.any():                # the rows of the empty queries are the flat search's
        Df, If = (flat or idx).search(Q[empty], k)
        assert D[empty].tobytes() == Df.tobytes() and np.array_equal(I[empty], If)
    assert st2["last_rows_scanned"] == (len(X) * int(empty.sum()) if fallback else 0)
    assert st2["last_candidates"] == st["last_candidates"] and st2["last_fallback_queries"] == st["last_fallback_queries"]
    return st2, count


@pytest.mark.parametrize("nq", [1, 255, 257, 1000])
def test_l2_selective_tables_exact_histogram_route(vdb, nq):
    """3 000 x 16, L2 T6 / H3 / w 2: a handful to ~140 colliding rows, some queries below the cap of 30.  The corpus is no larger
    than the sample, so the histogram is exact and every list is filled by the second scan: no query is flagged."""
    X, Q = _randn(3000, 16, seed=11), _randn(nq, 16, seed=12 + nq)
    p, b = _tables(6, 3, 16, seed=13, e2=True, w=2.0)
    idx = _index(vdb, X, p, b, 2.0)
    st, count = _check(idx, X, Q, p, b, 2.0, ncand=30, k=10)
    assert st["last_fallback_queries"] == 0
    if nq >= 255:
        assert (count < 30).any() and (count > 30).any() and count.max() < 400
    st, _ = _check(idx, X, Q, p, b, 2.0, ncand=30, k=40)          # k > ncand pads
    D, I = idx.lsht_search(Q, 40, 30)
    assert (I[:, 30:] == -1).all() and (D[:, 30:] == np.finfo(F32).max).all()
    idx.close()


@pytest.mark.parametrize("fallback", [False, True])
def test_sign_tables_with_empty_queries_and_the_bruteforce_fallback(vdb, fallback):
    """20 000 x 32, sign T8 / H16: 0 to a few dozen colliding rows and queries with none.  fallback = 1 sends exactly those to the
    exhaustive exact scan (last_rows_scanned = ntotal x their number) and their rows equal vdb_search; fallback = 0 pads them."""
    X, Q = _randn(20000, 32, seed=21), _randn(1000, 32, seed=22)
    p, _ = _tables(8, 16, 32, seed=32, e2=False)
    idx = _index(vdb, X, p, None, 0.0, metric="ip")
    st, count = _check(idx, X, Q, p, None, 0.0, ncand=40, k=10, metric="ip", fallback=fallback)
    assert st["last_fallback_queries"] == 0
    assert (count == 0).sum() >= 3 and count.max() <= 200
    D, I = idx.lsht_search(Q, 10, 40, fallback)
    none = count == 0
    if fallback:
        assert (I[none] >= ID_BASE).all()
    else:
        assert (I[none] == -1).all() and (D[none] == -np.finfo(F32).max).all()
    idx.close()


def _routed_corpus():
    """40 000 x 16 (above the 32 768-row sample, so the sampled bound and the first scan run) under T = 2 tables that read
    floor(x[0]) and floor(x[1]): the keys are set by hand.  Query type v in {0, 1, 2} is (v + 0.5, 0.5).  With ncand = 100 the
    list has 2048 entries and the bound wants 131 sample rows:
      v = 0   110 rows collide in both tables, 500 in table 0 only: the bound is class 2, 610 pairs fit the list -> complete
      v = 1   110 in both, 30 000 in table 0 only: the list overflows under the bound, the cut (class 0, 110 rows) fits -> rescan
      v = 2   3 000 duplicates collide in both: the ties at the cut exceed the list -> flagged, exact fallback of the select"""
    n, d = 40000, 16
    rng = np.random.default_rng(31)
    X = rng.standard_normal((n, d)).astype(F32)
    x0, x1 = np.full(n, 9.5, F32), np.full(n, 7.5, F32)
    sizes = [(0.5, 0.5, 110), (0.5, 7.5, 500), (1.5, 0.5, 110), (1.5, 7.5, 30000), (2.5, 0.5, 3000)]
    perm, at = rng.permutation(n), 0
    for a, c, m in sizes:
        x0[perm[at:at + m]], x1[perm[at:at + m]] = a, c
        at += m
    X[:, 0], X[:, 1] = x0, x1
    p = np.zeros((2, 1, d), F32)
    p[0, 0, 0] = p[1, 0, 1] = 1
    b = np.zeros((2, 1), F32)
    return X, p, b


@pytest.mark.parametrize("nq", [3, 257])
def test_sampled_bound_routes_complete_rescan_flagged(vdb, nq):
    X, p, b = _routed_corpus()
    Q = _randn(nq, 16, seed=32)
    Q[:, 0], Q[:, 1] = (np.arange(nq) % 3) + 0.5, 0.5
    idx = _index(vdb, X, p, b, 1.0)
    st, count = _check(idx, X, Q, p, b, 1.0, ncand=100, k=10)
    flagged = int((np.arange(nq) % 3 == 2).sum())
    assert st["last_fallback_queries"] == flagged                # the duplicated rows, and only they
    assert sorted(set(count.tolist())) == [3220, 3720, 33220]       # (table 1 alone collides with 3 220 rows)
    votes, ids = idx.lsht_candidates(Q, 100)
    assert (votes == 2).all()                                    # every candidate collides in both tables
    # the same calls through the exact fallback of the select: identical arrays
    D, I = idx.lsht_search(Q, 10, 100)
    idx.set_option("lsh_force_fallback", 1)
    votes2, ids2 = idx.lsht_candidates(Q, 100)
    assert idx.stats()["last_fallback_queries"] == nq
    D2, I2 = idx.lsht_search(Q, 10, 100)
    assert idx.stats()["last_fallback_queries"] == nq
    assert np.array_equal(votes, votes2) and np.array_equal(ids, ids2) and D.tobytes() == D2.tobytes() and np.array_equal(I, I2)
    idx.set_option("lsh_force_fallback", 0)
    # a cap above every class: all colliding rows of a query, the tail padding (ncand > colliding rows)
    st, _ = _check(idx, X, Q[:6], p, b, 1.0, ncand=4000, k=10)
    assert st["last_fallback_queries"] == 0
    idx.close()


def _wide_key_corpus(n, T, H):
    """n x 16 under T <= 16 E2 tables of H projections, unit bucket width, the keys set by hand: every projection of table t reads
    coordinate t, with offset 0 but for the last one of the table, whose offset is 0.6.  So the values 0.5 and 0.15 share every
    code of a table but the last word, and 9.5 and 5.5 share none with them or each other.  Rows are copies of prototypes:
      P1   7 rows   0.5 everywhere                         P3   40 rows   9.5, table T - 1 at 0.5
      P2  12 rows   0.5, table 0 at 0.15                   P4    5 rows   0.15 everywhere            the rest: 9.5 everywhere
    and the five queries are 0.5 everywhere (P1 in T tables, P2 in T - 1, P3 in one: 59 rows), 0.15 everywhere (P4 in T, P2 in
    one: 17 rows), 5.5 everywhere (no row), 9.5 everywhere (the rest in T, P3 in T - 1: nearly every row), and 0.5 with table 0
    at 0.15 (P2 in T, P1 in T - 1, P3 and P4 in one: 64 rows)."""
    d = 16
    rng = np.random.default_rng(41 + H)
    X = rng.standard_normal((n, d)).astype(F32)
    X[:, :T] = 9.5
    perm = rng.permutation(n)
    X[perm[0:7], :T] = 0.5
    X[perm[7:19], :T] = 0.5
    X[perm[7:19], 0] = 0.15
    X[perm[19:59], T - 1] = 0.5
    X[perm[59:64], :T] = 0.15
    Q = rng.standard_normal((5, d)).astype(F32)
    Q[0, :T], Q[1, :T], Q[2, :T], Q[3, :T], Q[4, :T] = 0.5, 0.15, 5.5, 9.5, 0.5
    Q[4, 0] = 0.15
    p = np.zeros((T, H, d), F32)
    for t in range(T):
        p[t, :, t] = 1
    b = np.zeros((T, H), F32)
    b[:, H - 1] = 0.6
    return X, Q, p, b


def _wide_key_conditions(X, Q, p, b, ncands):
    """what the corpus is built for, on the restatement alone: a query without a colliding row, two or more distinct vote counts
    for every other one, an ncand below and an ncand above the colliding rows of some query"""
    T = p.shape[0]
    votes, _, count = ref.candidates(ref.keys(Q, p, b, 1.0), ref.keys(X, p, b, 1.0), T, len(X), 0)
    assert count.tolist() == [59, 17, 0, len(X) - 24, 64]
    for q in np.flatnonzero(count):
        assert len(set(votes[q, :count[q]].tolist())) >= 2, (q, votes[q, :count[q]])
    assert (count > min(ncands)).any() and (count[count > 0] < max(ncands)).any()


@pytest.mark.parametrize("n", [1000, 33024])
@pytest.mark.parametrize("T,H", [(12, 5), (10, 7), (8, 9), (9, 13)])
def test_candidates_and_search_at_the_wide_key_widths(vdb, n, T, H):
    """E2 keys of 5, 7, 9 and 13 words per table are stored as 6, 8, 12 and 16: the widths the cases above leave out (T = 9 at
    H = 13 is the widest row the scan is compiled for).  N = 1000 takes the exact histogram, N = 33 024 the sampled bound and both
    scans; with and without the brute-force fallback, and once through the exact fallback of the select."""
    X, Q, p, b = _wide_key_corpus(n, T, H)
    _wide_key_conditions(X, Q, p, b, (10, 100))
    idx = _index(vdb, X, p, b, 1.0)
    assert idx.lsht_keys().shape == (n, T * H)                   # E2: one word per projection
    _check(idx, X, Q, p, b, 1.0, ncand=10, k=5)
    st, count = _check(idx, X, Q, p, b, 1.0, ncand=100, k=5, fallback=True)
    assert st["last_rows_scanned"] == n                           # the one query without a colliding row
    votes, ids = idx.lsht_candidates(Q, 100)
    idx.set_option("lsh_force_fallback", 1)
    st, _ = _check(idx, X, Q, p, b, 1.0, ncand=100, k=5, fallback=True)
    assert st["last_fallback_queries"] == len(Q)
    votes2, ids2 = idx.lsht_candidates(Q, 100)
    assert np.array_equal(votes, votes2) and np.array_equal(ids, ids2)
    idx.close()


def test_coarse_tables_most_rows_collide(vdb):
    """40 000 x 16 under the published shape (L2 T12 / H4, a wide bucket): most rows collide with every query and the cap cuts
    deep inside them; candidates and search equal the restatement whichever route a query takes, forced fallback included."""
    X, Q = _randn(40000, 16, seed=41), _randn(255, 16, seed=42)
    p, b = _tables(12, 4, 16, seed=43, e2=True, w=9.0)
    idx = _index(vdb, X, p, b, 9.0)
    st, count = _check(idx, X, Q, p, b, 9.0, ncand=1280, k=20)
    assert count.min() > 1280 and np.median(count) > 20000
    assert st["last_candidates"] == 255 * 1280
    votes, ids = idx.lsht_candidates(Q, 1280)
    idx.set_option("lsh_force_fallback", 1)
    votes2, ids2 = idx.lsht_candidates(Q, 1280)
    assert idx.stats()["last_fallback_queries"] == 255
    assert np.array_equal(votes, votes2) and np.array_equal(ids, ids2)
    idx.close()


def test_ncand_above_ntotal_pads(vdb):
    X, Q = _randn(7, 16, seed=51), _randn(20, 16, seed=52)
    Q[:7] = X                                    # every row collides with its own copy in every table
    p, b = _tables(4, 2, 16, seed=53, e2=True, w=8.0)
    idx = _index(vdb, X, p, b, 8.0)
    st, count = _check(idx, X, Q, p, b, 8.0, ncand=12, k=10)
    votes, ids = idx.lsht_candidates(Q, 12)
    assert (ids[:, 7:] == -1).all() and (votes[:, 7:] == 0).all() and (votes[np.arange(7), 0] == 4).all()
    assert st["last_fallback_queries"] == 0 and count.max() <= 7
    idx.close()


def test_device_forms_on_a_stream(vdb):
    import torch

    n, d, nq, ncand, k = 40000, 16, 300, 200, 10
    X, Q = _randn(n, d, seed=61), _randn(nq, d, seed=62)
    p, _ = _tables(8, 6, d, seed=63, e2=False)
    idx = _index(vdb, X, p, None, 0.0)
    votes, ids = idx.lsht_candidates(Q, ncand)
    qd = torch.from_numpy(Q).cuda()
    vd = torch.zeros((nq, ncand), dtype=torch.int32, device="cuda")
    idd = torch.zeros((nq, ncand), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    idx.lsht_candidates_device(qd.data_ptr(), nq, ncand, vd.data_ptr(), idd.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(vd.cpu().numpy(), votes) and np.array_equal(idd.cpu().numpy(), ids)
    for fallback in (False, True):
        Dd = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        Id = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        idx.lsht_search_device(qd.data_ptr(), nq, k, ncand, fallback, Dd.data_ptr(), Id.data_ptr(), s.cuda_stream)
        s.synchronize()
        D, I = idx.lsht_search(Q, k, ncand, fallback)
        assert Dd.cpu().numpy().tobytes() == D.tobytes() and np.array_equal(Id.cpu().numpy(), I)
    idx.lsht_search_device(qd.data_ptr(), nq, k, ncand, False, Dd.data_ptr(), Id.data_ptr(), 0)      # the null stream
    torch.cuda.synchronize()
    assert np.array_equal(Id.cpu().numpy(), idx.lsht_search(Q, k, ncand)[1])
    idx.close()


def test_timing_stages(vdb):
    X, Q = _randn(40000, 16, seed=71), _randn(64, 16, seed=72)
    p, b = _tables(6, 3, 16, seed=73, e2=True, w=2.0)
    idx = _index(vdb, X, p, b, 2.0)
    idx.set_option("timing", 1)
    idx.lsht_search(Q, 10, 50)
    st = idx.stats()
    assert st["last_scan_ms"] > 0 and st["last_prep_ms"] > 0 and st["last_tail_ms"] > 0
    assert abs(st["last_total_ms"] - (st["last_prep_ms"] + st["last_scan_ms"] + st["last_tail_ms"])) < 0.05 * st["last_total_ms"] + 0.01
    idx.close()


# ---- admission -------------------------------------------------------------------------------------------------------------
NQ, K, NCAND = ac.NQ, ac.K, ac.NCAND
T0, H0 = 4, 3
KIND_WORDS = {"07": "sign-LSH", "08": "k-NN graph", "09": "IVF", "10": "IVF", "11": "SQ8", "12": "SQ8", "13": "IVF-PQ", "14": "IVF-PQ",
              "15": "PQ", "16": "PQ", "17": "multi-device", "18": "multi-device"}
OPTION_WORDS = {"04": "int8_only", "05": "int8_only", "06": "stream_panels"}


def _new_entries(c, P, B):
    from vdbhip._ffi import ptr

    t, hs, mode, w = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_float(-1)
    votes = np.empty((NQ, NCAND), np.int32)
    tv = c.tham.data_ptr()
    return t, [
        ("vdb_lsht_set_tables", (T0, H0, 1, ptr(P), ptr(B), 2.0)),
        ("vdb_lsht_get_tables", (ctypes.byref(t), ctypes.byref(hs), ctypes.byref(mode), None, None, ctypes.byref(w))),
        ("vdb_lsht_get_keys", (ptr(c.words_out),)),
        ("vdb_lsht_candidates", (ptr(c.Q), NQ, NCAND, ptr(votes), ptr(c.I))),
        ("vdb_lsht_candidates_device", (c.tQ.data_ptr(), NQ, NCAND, tv, c.tI.data_ptr(), None)),
        ("vdb_lsht_search", (ptr(c.Q), NQ, K, NCAND, 0, ptr(c.D), ptr(c.I))),
        ("vdb_lsht_search_device", (c.tQ.data_ptr(), NQ, K, NCAND, 1, c.tD.data_ptr(), c.tI.data_ptr(), None)),
    ]


@pytest.mark.parametrize("state", list(ac.STATES))
def test_new_entry_points_on_every_existing_kind(vdb, state):
    """vdb_lsht_set_tables makes a flat handle an LSHT handle (unless an option that drops the float32 rows is set or in effect);
    the compute calls are STATE on a flat handle without tables; every other kind refuses all of them, naming itself."""
    import torch
    from vdbhip import _ffi

    lib = _ffi.load()
    s = ac.STATES[state]
    c = ac.ctx(s.d, s.n, s.byte_valued)
    P, B = _tables(T0, H0, s.d, seed=1, e2=True, w=2.0)
    tag = state[:2]
    flat = tag <= "06"
    h = ac.build(lib, s, c)
    try:
        want = ac.own_search(lib, s, c, h) if s.search else None
        t, entries = _new_entries(c, P, B)
        for name, args in entries:
            lib.vdb_device_count(None)
            rc = getattr(lib, name)(h, *args)
            torch.cuda.synchronize()
            msg = _ffi.last_error()
            if name == "vdb_lsht_get_tables":
                assert rc == _ffi.VDB_OK and t.value == 0, (name, rc, msg)
            elif name == "vdb_lsht_set_tables" and flat and tag not in OPTION_WORDS:
                assert rc == _ffi.VDB_OK, (rc, msg)
                lib.vdb_destroy(h)
                h = None
                h = ac.build(lib, s, c)
                continue
            elif flat:
                code = _ffi.VDB_ERR_UNSUPPORTED if name == "vdb_lsht_set_tables" else _ffi.VDB_ERR_STATE
                assert rc == code and name in msg, (name, rc, msg)
                if name == "vdb_lsht_set_tables":
                    assert OPTION_WORDS[tag] in msg and "hash tables" in msg, msg
            else:
                assert rc == _ffi.VDB_ERR_UNSUPPORTED and name in msg and KIND_WORDS[tag] in msg, (name, rc, msg)
            if want is not None:
                assert ac.own_search(lib, s, c, h) == want, name
    finally:
        if h is not None:
            lib.vdb_destroy(h)


def test_existing_entry_points_on_a_handle_with_tables(vdb, golden_dir):
    """A handle with tables answers what the sign-LSH column of the recorded matrix answers, except that the sign-LSH calls are
    refused on it (it is not that kind); a refused call leaves tables, keys and both searches as they were."""
    import torch
    from vdbhip import _ffi

    lib = _ffi.load()
    want = dict(json.loads((golden_dir / "admission_matrix.json").read_text())["cells"]["07_lsh"])
    for name in want:
        if name.startswith("vdb_lsh_") and name != "vdb_lsh_get_projection":
            want[name] = _ffi.VDB_ERR_UNSUPPORTED
    c = ac.ctx(32, 2000)
    P, B = _tables(T0, H0, 32, seed=1, e2=True, w=2.0)

    def build():
        idx = vdb.FlatIndex(32, "l2", 0)
        idx.lsht_set_tables(P, B, 2.0)
        idx.add(c.X)
        return idx

    def own(idx):
        D, I = idx.lsht_search(c.Q, K, NCAND)
        Df, If = idx.search(c.Q, K)
        return D.tobytes() + I.tobytes() + Df.tobytes() + If.tobytes() + idx.lsht_keys().tobytes()

    idx = build()
    before = own(idx)
    plain = vdb.FlatIndex(32, "l2", 0)
    plain.add(c.X)
    Dp, Ip = plain.search(c.Q, K)
    Df, If = idx.search(c.Q, K)
    assert Dp.tobytes() == Df.tobytes() and np.array_equal(Ip, If)        # the flat search is untouched by the tables
    plain.close()
    got = {}
    for name, fn, args in ac.entries(c):
        lib.vdb_device_count(None)
        rc = getattr(lib, fn)(idx._h, *args)
        torch.cuda.synchronize()
        got[name] = rc
        if rc == _ffi.VDB_OK:
            idx.close()
            idx = build()
            continue
        msg = _ffi.last_error()
        assert msg not in ("", ac.SENTINEL), name
        if rc == _ffi.VDB_ERR_UNSUPPORTED and "set_option" not in name:
            assert "hash tables" in msg, (name, msg)
        idx._sync_ntotal()
        assert own(idx) == before, name
    differ = {e: (got[e], want[e]) for e in got if got[e] != want[e]}
    assert not differ, f"(got, expected): {differ}"
    # the search calls are refused while option "graph" is 1, and come back with it off
    idx.set_option("graph", 1)
    votes, ids = np.empty((NQ, NCAND), np.int32), np.empty((NQ, NCAND), np.int64)
    rc = lib.vdb_lsht_candidates(idx._h, _ffi.ptr(c.Q), NQ, NCAND, _ffi.ptr(votes), _ffi.ptr(ids))
    assert rc == _ffi.VDB_ERR_UNSUPPORTED and "graph" in _ffi.last_error()
    rc = lib.vdb_lsht_search(idx._h, _ffi.ptr(c.Q), NQ, K, NCAND, 0, _ffi.ptr(c.D), _ffi.ptr(c.I))
    assert rc == _ffi.VDB_ERR_UNSUPPORTED and "graph" in _ffi.last_error()
    idx.set_option("graph", 0)
    assert own(idx) == before
    idx.close()


def test_states_and_argument_ranges(vdb):
    from vdbhip import _ffi

    lib = _ffi.load()
    d = 16
    X, Q = _randn(3000, d, seed=81), _randn(9, d, seed=82)
    p, b = _tables(6, 3, d, seed=83, e2=True, w=2.0)
    votes, ids, Dk = np.empty((9, 5), np.int32), np.empty((9, 5), np.int64), np.empty((9, 5), F32)
    idx = vdb.FlatIndex(d, "l2", 0)
    big = np.zeros((33, 64, d), F32)

    def set_tables(T, H, mode, pp=big, bb=big, w=2.0):
        return lib.vdb_lsht_set_tables(idx._h, T, H, mode, _ffi.ptr(pp), _ffi.ptr(bb) if bb is not None else None, w)

    for T, H, mode in ((0, 4, 0), (33, 4, 0), (4, 0, 0), (4, 65, 0), (4, 17, 1), (4, 0, 1), (9, 16, 1), (4, 4, 2), (4, 4, -1)):
        assert set_tables(T, H, mode) == _ffi.VDB_ERR_INVALID, (T, H, mode)
    assert set_tables(4, 4, 1, w=0.0) == _ffi.VDB_ERR_INVALID and set_tables(4, 4, 1, w=-1.0) == _ffi.VDB_ERR_INVALID
    assert set_tables(4, 4, 1, w=float("inf")) == _ffi.VDB_ERR_INVALID and set_tables(4, 4, 1, w=float("nan")) == _ffi.VDB_ERR_INVALID
    assert set_tables(4, 4, 1, bb=None) == _ffi.VDB_ERR_INVALID and set_tables(4, 4, 0, pp=None) == _ffi.VDB_ERR_INVALID
    assert idx.lsht_get_tables() is None                         # every refused call left the handle without tables
    assert set_tables(32, 64, 0, bb=None) == _ffi.VDB_OK         # the largest sign tables; offsets are not read in mode 0
    assert set_tables(8, 16, 1) == _ffi.VDB_OK                   # the largest E2 tables (128 words)
    idx.lsht_set_tables(p, b, 2.0)
    # tables, no rows: STATE
    assert lib.vdb_lsht_candidates(idx._h, _ffi.ptr(Q), 9, 5, _ffi.ptr(votes), _ffi.ptr(ids)) == _ffi.VDB_ERR_STATE
    assert lib.vdb_lsht_search(idx._h, _ffi.ptr(Q), 9, 5, 5, 0, _ffi.ptr(Dk), _ffi.ptr(ids)) == _ffi.VDB_ERR_STATE
    assert lib.vdb_lsht_get_keys(idx._h, _ffi.ptr(np.empty((3000, 18), np.uint32))) == _ffi.VDB_ERR_STATE
    idx.add(X)
    for ncand in (0, -1, 65537):
        assert lib.vdb_lsht_candidates(idx._h, _ffi.ptr(Q), 9, ncand, _ffi.ptr(votes), _ffi.ptr(ids)) == _ffi.VDB_ERR_INVALID
    for k in (0, 2049):
        assert lib.vdb_lsht_search(idx._h, _ffi.ptr(Q), 9, k, 5, 0, _ffi.ptr(Dk), _ffi.ptr(ids)) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_lsht_search(idx._h, _ffi.ptr(Q), 9, 5, 5, 2, _ffi.ptr(Dk), _ffi.ptr(ids)) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_lsht_search(idx._h, _ffi.ptr(Q), -1, 5, 5, 0, _ffi.ptr(Dk), _ffi.ptr(ids)) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_lsht_search(idx._h, None, 9, 5, 5, 0, _ffi.ptr(Dk), _ffi.ptr(ids)) == _ffi.VDB_ERR_INVALID
    _check(idx, X, Q, p, b, 2.0, ncand=5, k=5, id_base=0)
    # the options of kNeedsRows, in both orders
    for opt in ("int8_only", "stream_panels"):
        rc = lib.vdb_set_option(idx._h, opt.encode(), 1.0)
        assert rc == _ffi.VDB_ERR_UNSUPPORTED and opt in _ffi.last_error() and "hash tables" in _ffi.last_error()
        o = vdb.FlatIndex(d, "l2", 0)
        o.set_option(opt, 1)
        rc = lib.vdb_lsht_set_tables(o._h, 6, 3, 1, _ffi.ptr(p), _ffi.ptr(b), 2.0)
        assert rc == _ffi.VDB_ERR_UNSUPPORTED and opt in _ffi.last_error()
        assert o.lsht_get_tables() is None
        o.close()
    # reset keeps the tables, drops the keys; new tables re-key the rows
    idx.reset()
    assert idx.lsht_get_tables()["projections"].tobytes() == p.tobytes()
    assert lib.vdb_lsht_candidates(idx._h, _ffi.ptr(Q), 9, 5, _ffi.ptr(votes), _ffi.ptr(ids)) == _ffi.VDB_ERR_STATE
    idx.add(X[:2000])
    idx.add(X[2000:])
    _check(idx, X, Q, p, b, 2.0, ncand=5, k=5, id_base=0)
    p2, _ = _tables(5, 40, d, seed=84, e2=False)
    idx.lsht_set_tables(p2)
    assert np.array_equal(idx.lsht_keys(), ref.keys(X, p2))
    _check(idx, X, Q, p2, None, 0.0, ncand=5, k=5, id_base=0)
    idx.close()


def test_bytes_resident_grows_by_keys_and_tables_and_returns(vdb):
    d, n, T, H = 16, 6000, 6, 3
    X = _randn(n, d, seed=91)
    p, b = _tables(T, H, d, seed=92, e2=True, w=2.0)
    plain = vdb.FlatIndex(d, "l2", 0)
    plain.add(X)
    base = plain.stats()["bytes_resident"]
    plain.reset()
    base_reset = plain.stats()["bytes_resident"]                  # (the corpus statistics block outlives the rows)
    plain.close()
    idx = vdb.FlatIndex(d, "l2", 0)
    empty = idx.stats()["bytes_resident"]
    idx.lsht_set_tables(p, b, 2.0)
    tables = idx.stats()["bytes_resident"] - empty
    assert tables == p.nbytes + b.nbytes                          # the transposed projections and the offsets, exactly sized
    idx.add(X)
    grown = idx.stats()["bytes_resident"] - base - tables
    key_bytes = n * T * 3 * 4                                     # H = 3 words per table are stored as 3
    assert key_bytes <= grown <= key_bytes + key_bytes // 8 + 64, (grown, key_bytes)      # (+ the growth slack of a device buffer)
    idx.reset()
    assert idx.stats()["bytes_resident"] == base_reset + tables   # keys and rows gone, tables kept
    idx.add(X)
    assert idx.stats()["bytes_resident"] == base + tables + grown
    idx.close()


# ---- the reference's results -----------------------------------------------------------------------------------------------
def _composite(vdb, c, dim):
    return vdb.get_algorithm_instance(
        "Composite", dim, name="lsh", metric=c["metric"],
        indexer={"type": "HipLSHTableIndexer", "metric": c["metric"], "num_tables": c["num_tables"], "hash_size": c["hash_size"],
                 "bucket_width": c["bucket_width"], "seed": c["seed"], "reserve_queries": 0},
        searcher={"type": "HipLSHTableSearcher", "metric": c["metric"], "candidate_multiplier": c["candidate_multiplier"],
                  "max_candidates": c["max_candidates"], "fallback_to_bruteforce": c["fallback_to_bruteforce"]})


def _reference_distances(x, q, ids, metric):
    """LSHSearcher._compute_distances over the recorded ids, float32 NumPy as there"""
    x, q = preprocess(x, q, metric)
    out = np.full(ids.shape, np.inf, F32)
    for i in range(len(q)):
        rows = ids[i][ids[i] >= 0]
        v = x[rows]
        out[i, :rows.size] = (1.0 - v @ q[i]).astype(F32) if metric == "cosine" else np.linalg.norm(v - q[i][None, :], axis=1).astype(F32)
    return out


def test_published_random_lsh_point(vdb, golden_dir):
    """The reference's `lsh` config on its `random` dataset (L2 T12 / H4 / w 20, 64 x 20 = 1280 candidates, top-20, no fallback):
    the ids of all 256 queries equal the reference's, so the recalls are the published ones."""
    from vdbhip import harness
    from vdbhip.metrics import recall_at_k

    doc = json.loads((golden_dir / "lsh_tables_published.json").read_text())
    c = doc["published"]
    recorded = np.load(golden_dir / "lsh_tables_published.npz")["ids"].astype(np.int64)
    train, q = published_queries(golden_dir)
    gt = harness.ground_truth(train, q, k=200, metric="l2")
    algo = _composite(vdb, c, train.shape[1])
    algo.build_index(train)
    dist, ids = algo.batch_search(q, c["topk"])
    assert dist.dtype == np.float32 and ids.dtype == np.int64 and ids.shape == (256, 20)
    assert np.array_equal(ids, recorded)
    r10, r1 = recall_at_k(gt, ids, 10), recall_at_k(gt, ids, 1)
    print(f"recall@10 {r10!r} (published {c['recall@10']!r}), recall@1 {r1!r} (published {c['recall@1']!r})")
    assert abs(r10 - c["recall@10"]) <= 1e-9 and abs(r1 - c["recall@1"]) <= 1e-9
    np.testing.assert_allclose(dist, _reference_distances(train, q, recorded, "l2"), rtol=1e-4, atol=0)
    st = algo.searcher.index.stats()
    assert st["last_path"] == PATH_LSHT and st["last_candidates"] == 256 * 1280 and st["last_rows_scanned"] == 0
    d1, i1 = algo.search(q[3], c["topk"])
    assert np.array_equal(i1, ids[3]) and np.array_equal(d1, dist[3])
    assert algo.get_memory_usage() > 0
    algo.searcher.index.close()


@pytest.mark.parametrize("name", ["l2_t6_h3_w2", "cosine_t8_h16_fallback", "cosine_t8_h16_no_fallback", "cosine_t24_h8"])
def test_recorded_reference_cases(vdb, golden_dir, name):
    doc = json.loads((golden_dir / "lsh_tables_published.json").read_text())
    c = doc["cases"][name]
    recorded = np.load(golden_dir / "lsh_tables_cases.npz")[name].astype(np.int64)
    x, q = case_data(c)
    algo = vdb.get_algorithm_instance(
        "HipLSHTables", c["dim"], name="lsh", metric=c["metric"], num_tables=c["num_tables"], hash_size=c["hash_size"],
        bucket_width=c["bucket_width"], candidate_multiplier=c["candidate_multiplier"], max_candidates=c["max_candidates"],
        fallback_to_bruteforce=c["fallback_to_bruteforce"], seed=c["seed"], reserve_queries=0)
    algo.build_index(x)
    dist, ids = algo.batch_search(q, c["topk"])
    assert np.array_equal(ids, recorded)
    want = _reference_distances(x, q, recorded, c["metric"])
    np.testing.assert_allclose(dist, want, rtol=1e-4, atol=1e-6 if c["metric"] == "cosine" else 0)
    assert np.array_equal(np.isinf(dist), recorded < 0)
    st = algo.index.stats()
    empty = c["queries_without_candidates"]
    assert st["last_rows_scanned"] == (c["n"] * empty if c["fallback_to_bruteforce"] else 0)
    assert st["last_fallback_queries"] == 0
    pair = _composite(vdb, c, c["dim"])
    pair.build_index(x)
    d2, i2 = pair.batch_search(q, c["topk"])
    assert np.array_equal(i2, ids) and d2.tobytes() == dist.tobytes()
    algo.index.close()
    pair.searcher.index.close()

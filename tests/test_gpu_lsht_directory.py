"""Hash-table LSH with option "lsht_directory" = 2 (the bucket lookup of csrc/lsht_dir.hpp in place of the vote scans) against the
NumPy restatement of the contract (tests/lsh_tables_restatement.py) and against option 0 of the same handle: votes, candidate ids,
D and I byte for byte."""
from __future__ import annotations

import numpy as np
import pytest

from tests.test_gpu_lsh_tables import ID_BASE, _index, _randn, _tables, ref
from tests.test_lsht_dir_plan_host import slot_hashes

pytestmark = pytest.mark.gpu

F32 = np.float32


def _compare(idx, X, Q, p, b, w, ncand, k, fallback=False):
    """both options against the restatement and each other; returns (stats after the option-2 search, colliding rows per query)"""
    want_v, want_i, count = ref.candidates(ref.keys(Q, p, b, w), ref.keys(X, p, b, w), p.shape[0], ncand, ID_BASE)
    got = {}
    for opt in (0, 2):
        idx.set_option("lsht_directory", opt)
        votes, ids = idx.lsht_candidates(Q, ncand)
        st = idx.stats()
        assert (st["scan_dtype"] == 9) == (opt == 2) and st["last_candidates"] == int(np.minimum(count, ncand).sum()), (opt, st)
        assert np.array_equal(votes, want_v) and np.array_equal(ids, want_i), (opt, np.flatnonzero((ids != want_i).any(axis=1))[:5])
        D, I = idx.lsht_search(Q, k, ncand, fallback)
        got[opt] = (D, I, idx.stats(), st)
    (D0, I0, st0, c0), (D2, I2, st2, c2) = got[0], got[2]
    assert D0.tobytes() == D2.tobytes() and I0.tobytes() == I2.tobytes()
    keep = (count > 0) | (not fallback)
    Dr, Ir = idx.rerank(Q, want_i, k)                       # "candidates, then vdb_rerank", bit for bit
    assert D2[keep].tobytes() == Dr[keep].tobytes() and I2[keep].tobytes() == Ir[keep].tobytes()
    brute = len(X) * int((count == 0).sum()) if fallback else 0
    assert st0["last_rows_scanned"] == brute and c0["last_rows_scanned"] == 0
    # the lookup walks at least the colliding (row, table) pairs of every query it serves (a flagged one leaves the second pass at once)
    walked = 0 if st2["last_fallback_queries"] else int(want_v.sum())
    assert c2["last_rows_scanned"] >= walked and st2["last_rows_scanned"] >= brute + walked
    assert st0["last_fallback_queries"] == st2["last_fallback_queries"]
    return st2, count


@pytest.mark.parametrize("e2,T,H,n,d,w", [
    (False, 4, 8, 3000, 16, 0.0),        # W = 1, few buckets, each larger than a wave
    (False, 3, 40, 3000, 16, 0.0),       # W = 2, nearly every row a bucket of its own
    (True, 3, 3, 3000, 8, 0.5),          # E2, stored width 3, rows spread over many codes
    (False, 2, 16, 40000, 8, 0.0)])      # above the sample: the MODE 0 lookup runs; different keys share slots
def test_lookup_equals_restatement_and_scan(vdb, e2, T, H, n, d, w):
    X = _randn(n, d, seed=T * 100 + H)
    p, b = _tables(T, H, d, seed=H, e2=e2, w=w)
    rk = ref.keys(X, p, b, w)
    W = ref.words_per_table(H, 1 if e2 else 0)
    Q = np.concatenate([X[:40] + F32(0.01) * _randn(40, d, seed=5), _randn(24, d, seed=6)])
    if n > 32768:
        uniq = np.unique(rk[:, :W], axis=0)
        slots = slot_hashes(uniq) & np.uint32(65535)
        order = np.argsort(slots, kind="stable")
        dup = np.flatnonzero(slots[order][1:] == slots[order][:-1])
        assert dup.size > 0, "no slot of table 0 holds two different keys"
        shared = uniq[order[dup[:4]]]                                     # queries that land in such slots
        rows = [np.flatnonzero((rk[:, :W] == key).all(axis=1))[0] for key in shared]
        Q = np.concatenate([Q, X[rows]])
    idx = _index(vdb, X, p, b, w)
    st, count = _compare(idx, X, Q, p, b, w, ncand=50, k=10)
    assert (count > 0).sum() >= 40 and st["last_fallback_queries"] == 0
    if (T, H) == (4, 8):
        assert np.median(count) > 64
    if H == 40:
        assert np.median(count[:40]) <= 4
    idx.close()


def test_directory_follows_adds_reset_and_the_option(vdb):
    d, w = 16, 2.0
    X, Q = _randn(3000, d, seed=1), _randn(64, d, seed=2)
    p, b = _tables(6, 3, d, seed=3, e2=True, w=w)
    idx = vdb.FlatIndex(d, "l2", 0)
    idx.set_option("lsht_directory", 2)              # before tables and rows: built behind the keys of the add
    idx.lsht_set_tables(p, b, w)
    idx.add(X[:2000], id_base=ID_BASE)
    _compare(idx, X[:2000], Q, p, b, w, ncand=30, k=10)             # (2 -> 0 -> 2 inside)
    held = idx.stats()["bytes_resident"]
    idx.set_option("lsht_directory", 0)
    assert held - idx.stats()["bytes_resident"] == 6 * (2048 + 1 + 2000) * 4        # 0 releases T (S + 1 + N) int32
    idx.set_option("lsht_directory", 2)
    assert idx.stats()["bytes_resident"] == held
    idx.add(X[2000:], id_base=ID_BASE)                               # every add rebuilds it whole
    _compare(idx, X, Q, p, b, w, ncand=30, k=10)
    idx.reset()
    idx.set_option("lsht_directory", 2)
    idx.add(X[500:], id_base=ID_BASE)
    _compare(idx, X[500:], Q, p, b, w, ncand=30, k=10)
    idx.close()


def _route_case(name):
    """(X, Q, p, b, w, ncand, fallback, force)"""
    d = 16
    if name == "giant_bucket":                       # 5000 identical rows + 100 others: the list overflows, ties at the cut
        X = np.concatenate([np.tile(_randn(1, d, seed=7), (5000, 1)), _randn(100, d, seed=8)])
        X = X[np.random.default_rng(9).permutation(len(X))]
        p, b = _tables(4, 3, d, seed=10, e2=True, w=4.0)
        return X, np.concatenate([X[:8], _randn(8, d, seed=11)]), p, b, 4.0, 100, False, 0
    if name == "nan":                                # E2 keys INT32_MIN of a NaN row and a NaN query collide
        X, Q = _randn(3000, d, seed=12), _randn(16, d, seed=13)
        X[17], Q[3] = np.nan, np.nan
        p, b = _tables(4, 3, d, seed=14, e2=True, w=2.0)
        return X, Q, p, b, 2.0, 40, False, 0
    X, Q = _randn(3000, d, seed=15), np.concatenate([_randn(3000, d, seed=15)[:8], _randn(8, d, seed=16)])
    if name == "force_fallback":
        p, b = _tables(4, 8, d, seed=17, e2=False)
        return X, Q, p, None, 0.0, 40, False, 1
    p, b = _tables(3, 40, d, seed=18, e2=False)      # "bruteforce": a random query collides with no row
    return X, Q, p, None, 0.0, 40, True, 0


@pytest.mark.parametrize("name", ["giant_bucket", "force_fallback", "bruteforce", "nan"])
def test_routes_of_the_select(vdb, name):
    X, Q, p, b, w, ncand, fallback, force = _route_case(name)
    idx = _index(vdb, X, p, b, w)
    idx.set_option("lsh_force_fallback", force)
    st, count = _compare(idx, X, Q, p, b, w, ncand=ncand, k=10, fallback=fallback)
    if name == "giant_bucket":
        assert (count >= 5000).sum() >= 5 and st["last_fallback_queries"] >= 5                # flagged: 5000 ties exceed the list
        st, _ = _compare(idx, X, Q, p, b, w, ncand=3000, k=10)                                 # ... and fit it: rescan
        assert st["last_fallback_queries"] == 0
    if name == "force_fallback":
        assert st["last_fallback_queries"] == len(Q)
    if name == "bruteforce":
        assert (count[8:] == 0).all() and (count[:8] > 0).all()
    if name == "nan":
        assert count[3] >= 1 and idx.lsht_candidates(Q[3:4], 1)[1][0, 0] == ID_BASE + 17
    idx.close()

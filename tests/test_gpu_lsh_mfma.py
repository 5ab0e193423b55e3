"""Option "lsh_mfma": the sign-LSH Hamming scans on the int8 matrix instruction (csrc/lsh_mfma.hpp) against the NumPy restatement of
the contract (tests/lsh_restatement.py, exact integer arithmetic) and against the popcount scans of the same handle, bit for bit:
a Hamming distance is an exact int32 dot product, so there is no tolerance anywhere."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import lsh_restatement as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
ID_BASE = 1000


def _corpus(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F32)


def _index(vdb, X, R, metric="l2"):
    idx = vdb.FlatIndex(X.shape[1], metric, 0)
    idx.lsh_set_projection(R)
    idx.add(X, id_base=ID_BASE)
    return idx


def _both(idx, Q, ncand):
    """(ham, ids, stats) with the option at 1, after checking them against the option at 0 and scan_dtype on both sides."""
    idx.set_option("lsh_mfma", 0)
    ham0, ids0 = idx.lsh_candidates(Q, ncand)
    assert idx.stats()["scan_dtype"] != 8
    idx.set_option("lsh_mfma", 1)
    ham1, ids1 = idx.lsh_candidates(Q, ncand)
    st = idx.stats()
    assert st["scan_dtype"] == 8 and st["last_path_name"] == "lsh", st
    assert np.array_equal(ham1, ham0) and np.array_equal(ids1, ids0)
    return ham1, ids1, st


# n = 1000: the corpus is its own sample (MODE 1 only); 33 037: just above the 32 768-row sample (MODE 0, then MODE 1), ragged last row
# tile; 40 000 x 300: two query tiles, the second partial; 300 000 x 32 bits: thousands of rows tie at the cut (list overflow).  32 bits
# run half a K-step, 96 have a padding word, 1024 is the widest; n and nq are no multiples of 16.
CASES = [(1000, nbits, 37, 10) for nbits in (32, 96, 256, 1024)] + [(1000, 256, 1, 1005)] + \
        [(33037, nbits, 5, 10) for nbits in (96, 256, 1024)] + [(40000, 256, 300, 1280), (300000, 32, 37, 10)]


@pytest.mark.parametrize("n,nbits,nq,ncand", CASES)
def test_candidates_bit_exact(vdb, n, nbits, nq, ncand):
    d = 64 if n == 40000 else 16
    X = _corpus(n, d, seed=n + nbits)
    Q = _corpus(nq, d, seed=n + nbits + 1)
    if nq > 2:
        Q[1] = X[n // 2]                        # a query that is a corpus row: distance 0 exists
        Q[2] = 0                                # every bit set
    R = vdb.make_projection(d, nbits, seed=4)
    idx = _index(vdb, X, R)
    ham, ids, _ = _both(idx, Q, ncand)
    rh, ri = ref.candidates(ref.encode(Q, R), ref.encode(X, R), ncand, ID_BASE)
    assert np.array_equal(ham, rh) and np.array_equal(ids, ri)
    idx.close()


def test_cut_inside_a_duplicated_code_and_the_forced_fallback(vdb):
    """One row repeated 5000 times: at 10 candidates the ties overflow the list of the query equal to it (the select's exact
    fallback, unforced); then every query forced there, with the option still on: the same arrays."""
    n, d, nbits, ncand = 40000, 64, 256, 10
    X = _corpus(n, d, seed=11)
    dup = np.random.default_rng(5).choice(n, 5000, replace=False)
    X[dup] = X[dup[0]]
    Q = _corpus(37, d, seed=12)
    Q[0] = X[dup[0]]
    R = vdb.make_projection(d, nbits, seed=6)
    idx = _index(vdb, X, R)
    ham, ids, st = _both(idx, Q, ncand)
    assert st["last_fallback_queries"] >= 1, st
    rh, ri = ref.candidates(ref.encode(Q, R), ref.encode(X, R), ncand, ID_BASE)
    assert np.array_equal(ham, rh) and np.array_equal(ids, ri)
    idx.set_option("lsh_force_fallback", 1)
    ham_f, ids_f = idx.lsh_candidates(Q, ncand)
    st = idx.stats()
    assert st["last_fallback_queries"] == len(Q) and st["scan_dtype"] == 8, st
    assert np.array_equal(ham_f, ham) and np.array_equal(ids_f, ids)
    idx.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_search_equals_the_popcount_search(vdb, metric):
    n, d, ncand, k = 40000, 128, 640, 10
    X = _corpus(n, d, seed=41)
    Q = _corpus(48, d, seed=42)
    idx = _index(vdb, X, vdb.make_projection(d, 256, seed=9), metric)
    D0, I0 = idx.lsh_search(Q, k, ncand)
    idx.set_option("lsh_mfma", 1)
    D1, I1 = idx.lsh_search(Q, k, ncand)
    assert idx.stats()["scan_dtype"] == 8
    assert D1.tobytes() == D0.tobytes() and np.array_equal(I1, I0)
    idx.close()


def test_plugin_pair_with_mfma_scan(vdb):
    n, d, nq, k = 20000, 64, 64, 20
    X = _corpus(n, d, seed=61)
    Q = _corpus(nq, d, seed=62)
    out = []
    for extra in ({}, {"mfma_scan": True}):
        algo = vdb.get_algorithm_instance(
            "Composite", d, name="faiss_lsh", metric="l2",
            indexer=dict({"type": "HipLSHIndexer", "num_bits": 256, "seed": 3, "reserve_queries": 100}, **extra),
            searcher={"type": "HipLSHSearcher", "lsh_candidate_multiplier": 64.0})
        algo.build_index(X)
        out.append(algo.batch_search(Q, k))
        assert (algo.searcher.index.stats()["scan_dtype"] == 8) == bool(extra)
        algo.searcher.index.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and np.array_equal(out[0][1], out[1][1])

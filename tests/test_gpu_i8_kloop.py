"""Option `i8_kloop`: a byte-valued corpus of more than 128 dimensions gets an int8 scan copy in p16 order, and integer query
batches inside a byte window take scan16_i8_kloop_kernel (v_mfma_i32_16x16x64_i8, exact int32 keys).  Same ids and distances
as the oracle and as the same handle on its fp16 K-loop scan (`panel_dtype` = 1)."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WINDOWS = {"u8": (0, 218), "s8": (-128, 90)}
N = 20_001                                   # ragged last span: 20 480 padded rows


def _bytes(n, d, seed, lo=0, hi=218):        # (as tests/test_gpu_int8_only.py)
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.gamma(0.6, 40.0, size=(n, d))) + lo, lo, hi).astype(np.float32)


def _index(vdb, X, metric, on=1):
    ix = vdb.FlatIndex(X.shape[1], metric, 0)
    if on is not None:
        ix.set_option("i8_kloop", on)
    ix.set_option("force_path", 2)           # (these few rows take the MFMA scan at every batch size)
    ix.add(X, id_base=9)
    return ix


def _equal(ix, Q, k, want, dtype):
    D, I = ix.search(Q, k)
    np.testing.assert_array_equal(I, want[1][:len(Q), :k])
    np.testing.assert_array_equal(D, want[0][:len(Q), :k])
    s = ix.stats()
    assert s["last_path_name"] == "mfma_scan" and s["scan_dtype"] == dtype, s


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("window", ["u8", "s8"])
@pytest.mark.parametrize("d", [136, 192, 768])
def test_parity_with_oracle_and_fp16_scan(vdb, oracle, metric, window, d):
    lo, hi = WINDOWS[window]
    X, Q = _bytes(N, d, N + d, lo, hi), _bytes(600, d, 5, lo, hi)
    ix = _index(vdb, X, metric)
    st = ix.stats()
    assert st["has_i8_copy"] == 1 and st["scan_shape"] == 0, st
    want = oracle.knn(X, Q, 10, metric, id_base=9)           # (k = 1 is its first column: ties go by id)
    for nq in (1, 17, 70, 600):
        for k in (1, 10):
            _equal(ix, Q[:nq], k, want, 1)
    Qf, Qw = Q[:70].copy(), Q[:70].copy()
    Qf[3, d - 1] += 0.5                                      # one non-integer value / one value outside both byte windows
    Qw[69, 0] = 300.0
    for Qx in (Qf, Qw):
        _equal(ix, Qx, 10, oracle.knn(X, Qx, 10, metric, id_base=9), 0)
    ix.set_option("panel_dtype", 1)                          # the same handle on the fp16 K-loop scan
    for nq in (1, 600):
        _equal(ix, Q[:nq], 10, want, 0)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("window", ["u8", "s8"])
def test_key_range_at_4096_dimensions(vdb, oracle, metric, window):
    """Rows and queries at the ends of the byte window: where a wrong offset, shift or padding key shows."""
    d, n = 4096, 6000
    lo, top = (0, 255) if window == "u8" else (-128, 127)
    X, Q = _bytes(n, d, 11, *WINDOWS[window]), _bytes(8, d, 12, *WINDOWS[window])
    X[17], X[2999], X[5999], X[4000] = top, lo, lo + 128, top
    Q[0], Q[1] = lo, top
    if window == "s8":
        X[100], Q[2] = -127, -127
    ix = _index(vdb, X, metric)
    assert ix.stats()["has_i8_copy"] == 1
    _equal(ix, Q, 1, oracle.knn(X, Q, 1, metric, id_base=9), 1)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties_and_duplicates_at_768_dimensions(vdb, oracle, metric):
    """Rows one unit in one dimension away from a query's k-th neighbour, and exact duplicates, in different bins and quads: the
    shifted key (D = 768: shift 1) may not separate them, the exact refine must, in the oracle's (distance, id) order."""
    d, k = 768, 10
    X, Q = _bytes(N, d, 21), _bytes(40, d, 22)
    rng = np.random.default_rng(23)
    for qi in range(40):
        base = Q[qi].copy()
        base[rng.integers(d)] += 3                           # the k-th neighbour to be: close to the query
        rows = rng.choice(N, size=12, replace=False)
        for j, r in enumerate(rows):
            X[r] = base
            if j >= 6:                                       # six duplicates, six rows one unit off in one dimension
                X[r, rng.integers(d)] += 1 if j % 2 else -1
    X = np.clip(X, 0, 255)
    ix = _index(vdb, X, metric)
    _equal(ix, Q, k, oracle.knn(X, Q, k, metric, id_base=9), 1)


def test_option_off_builds_nothing(vdb):
    X = _bytes(N, 192, 31)
    never, off = _index(vdb, X, "l2", on=None), _index(vdb, X, "l2", on=0)
    a, b = never.stats(), off.stats()
    assert a["has_i8_copy"] == b["has_i8_copy"] == 0
    assert a["bytes_resident"] == b["bytes_resident"]
    assert _index(vdb, X, "l2").stats()["bytes_resident"] > a["bytes_resident"]

"""Option `ivf_i8_kloop`: an IVF-Flat index over a byte-valued corpus of more than 128 dimensions also gets an int8 copy of its
list-padded panel space, and integer query batches of an unfiltered search on the list-major path take ivf_kloop_i8_scan_kernel
(v_mfma_i32_16x16x64_i8, exact int32 keys; csrc/ivf_kloop_i8.hpp).  Ids and distances must be byte-equal to oracle.ivf_search with
the same centroids and lists, and to the same handle on its fp16 K-loop list scan (`panel_dtype` = 1)."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
WINDOWS = {"u8": (0, 255), "s8": (-128, 127)}
NLIST, ID0 = 24, 1000
# an empty list, one row, one row short of a 256-row span, exactly one, one more, and a list of several spans (one 1024-row span + 126)
SIZES = {0: 0, 1: 1, 2: 255, 3: 256, 4: 257, 5: 1150}


def _lists(n, nlist=NLIST, sizes=SIZES, seed=5):
    rng = np.random.default_rng(seed)
    lor = np.concatenate([np.full(s, l, np.int32) for l, s in sizes.items()])
    lor = np.concatenate([lor, rng.integers(len(sizes), nlist, n - len(lor)).astype(np.int32)])
    rng.shuffle(lor)
    return lor


def _data(n, nq, d, window, nlist=NLIST, seed=0):
    lo, hi = WINDOWS[window]
    rng = np.random.default_rng(1000 * d + seed + (7 if window == "s8" else 0))
    X = rng.integers(lo, hi + 1, (n, d)).astype(F32)
    X[0, 0], X[1, 0], X[2, d - 1], X[3, d - 1] = lo, hi, lo, hi
    return X, rng.uniform(lo, hi, (nlist, d)).astype(F32), rng.integers(lo, hi + 1, (nq, d)).astype(F32)


def _index(vdb, X, C, lor, metric, on=1, **opts):
    ix = vdb.IVFFlatIndex(X.shape[1], len(C), metric, 0)
    ix.set_centroids(C)
    if on is not None:
        ix.set_option("ivf_i8_kloop", on)
    for name, v in dict(opts, ivf_min_batch=1).items():
        ix.set_option(name, v)
    ix.add(X, id_base=ID0, list_of_row=lor)
    return ix


def _equal(got, want, k=None):
    np.testing.assert_array_equal(got[1], want[1][:, :k])
    np.testing.assert_array_equal(got[0], want[0][:, :k])


def _served(ix, dtype, fallbacks=0):
    s = ix.stats()
    assert s["last_path_name"] == "ivf" and s["scan_dtype"] == dtype and s["last_candidates"] > 0, s
    assert fallbacks is None or s["last_fallback_queries"] == fallbacks, s


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("window", ["u8", "s8"])
@pytest.mark.parametrize("d", [136, 192, 768])
def test_parity_with_the_oracle_and_the_fp16_list_scan(vdb, oracle, metric, window, d):
    """136: ragged D, 3 K-steps against a barrier every 2; 768: shift 1.  nprobe 24 = every list: 600 slots on each, two work items;
    nprobe 8 leaves waves of padding slots only.  (24, 10) and (8, 1) are batches the list-major path serves at both span sizes."""
    X, C, Q = _data(6000, 600, d, window)
    lor = _lists(len(X))
    want = {p: oracle.ivf_search(X, C, lor, Q, 10, p, metric, id_base=ID0) for p in (1, 8, 24)}      # (k = 1 is the first column)
    for tps, settings in ((16, ((1, 0), (2, 0), (4, 1))), (64, ((0, 0), (0, 1)))):                    # (ivf_group, ivf_part) after the add
        ix = _index(vdb, X, C, lor, metric, ivf_tps=tps)
        assert ix.stats()["has_i8_copy"] == 1
        for group, part in settings:
            ix.set_option("ivf_group", group)
            ix.set_option("ivf_part", part)
            for nprobe in (1, 8, 24):
                ix.set_nprobe(nprobe)
                for k in (1, 10):
                    _equal(ix.search(Q, k), want[nprobe], k)
                    if (nprobe, k) in ((24, 10), (8, 1)):
                        _served(ix, 1)
        ix.set_option("panel_dtype", 1)                      # the same handle on the fp16 K-loop list scan
        _equal(ix.search(Q, 10), want[24])
        _served(ix, 0)
        ix.set_option("panel_dtype", 0)
        Qf, Qw = Q.copy(), Q.copy()
        Qf[3, d - 1] += 0.5                                  # one non-integer value / one value outside both byte windows
        Qw[599, 0] = 300.0
        for Qx in (Qf, Qw):
            _equal(ix.search(Qx, 10), oracle.ivf_search(X, C, lor, Qx, 10, 24, metric, id_base=ID0))
            _served(ix, 0)
        ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("window", ["u8", "s8"])
def test_key_range_at_4096_dimensions(vdb, oracle, metric, window):
    """Shift 4.  Rows and queries at the ends of the byte window: where a wrong offset, shift or padding key shows."""
    d, n, nlist = 4096, 3000, 4
    lo, top = WINDOWS[window]
    X, C, Q = _data(n, 8, d, window, nlist)
    lor = _lists(n, nlist, {0: 700})
    X[17], X[1499], X[2999], X[2000] = top, lo, lo + 128, top
    Q[0], Q[1] = lo, top
    if window == "s8":
        X[100], Q[2] = -127, -127
    ix = _index(vdb, X, C, lor, metric)
    ix.set_nprobe(nlist)
    assert ix.stats()["has_i8_copy"] == 1
    _equal(ix.search(Q, 1), oracle.ivf_search(X, C, lor, Q, 1, nlist, metric, id_base=ID0))
    _served(ix, 1, fallbacks=None)       # (u8 / ip: the all-zero query scores every row 0 -- every bin ties and the select hands it to the exact scan)
    ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties_and_duplicates_at_768_dimensions(vdb, oracle, metric):
    """Exact duplicates of a query's k-th neighbour and rows one unit away from it, spread over lists, bins and quads: the shifted key
    (shift 1) may not separate them, the exact refine must, in the oracle's (distance, id) order."""
    d, k = 768, 10
    X, C, Q = _data(6000, 40, d, "u8")
    lor = _lists(len(X))                                     # (shuffled: the planted rows below land in many lists and bins)
    rng = np.random.default_rng(23)
    for qi in range(len(Q)):
        base = Q[qi].copy()
        base[rng.integers(d)] += 3                           # the k-th neighbour to be: close to the query
        for j, r in enumerate(rng.choice(len(X), size=12, replace=False)):
            X[r] = base
            if j >= 6:                                       # six duplicates, six rows one unit off in one dimension
                X[r, rng.integers(d)] += 1 if j % 2 else -1
    X = np.clip(X, 0, 255)
    ix = _index(vdb, X, C, lor, metric)
    ix.set_nprobe(NLIST)
    _equal(ix.search(Q, k), oracle.ivf_search(X, C, lor, Q, k, NLIST, metric, id_base=ID0))
    _served(ix, 1)
    ix.close()


def test_lifecycle_appends_and_the_calls_that_never_see_the_copy(vdb, oracle):
    d, metric = 192, "l2"
    X, C, Q = _data(6000, 200, d, "u8")
    lor = _lists(len(X))
    never, off, on = (_index(vdb, X, C, lor, metric, on=v) for v in (None, 0, 1))
    a, b, c = never.stats(), off.stats(), on.stats()
    assert a["has_i8_copy"] == b["has_i8_copy"] == 0 and c["has_i8_copy"] == 1
    assert a["bytes_resident"] == b["bytes_resident"] < c["bytes_resident"]
    # an append of byte-valued rows equals one add
    two = vdb.IVFFlatIndex(d, NLIST, metric, 0)
    two.set_centroids(C)
    two.set_option("ivf_i8_kloop", 1)
    two.set_option("ivf_min_batch", 1)
    two.add(X[:4000], id_base=ID0, list_of_row=lor[:4000])
    two.add(X[4000:], id_base=ID0, list_of_row=lor[4000:])
    assert two.stats()["has_i8_copy"] == 1
    want = oracle.ivf_search(X, C, lor, Q, 10, NLIST, metric, id_base=ID0)
    for ix in (two, on, off):
        ix.set_nprobe(NLIST)
        _equal(ix.search(Q, 10), want)
        _served(ix, 0 if ix is off else 1)
    # filtered and range calls on the option-on handle: the option-off handle's bytes, on the fp16 panels
    allow = np.random.default_rng(3).random(len(X)) < 0.5
    radius = float(np.sort(want[0][:, 9])[100])
    for ix in (on, off):
        ix.set_filter(allow)
    _equal(on.search_filtered(Q, 10), off.search_filtered(Q, 10))
    assert on.stats()["scan_dtype"] == 0 and on.stats()["last_candidates"] > 0
    for x, y in zip(on.range_search(Q, radius), off.range_search(Q, radius)):
        np.testing.assert_array_equal(x, y)
    assert on.stats()["scan_dtype"] == 0
    # an append of a fractional row drops the copy; searches still equal the oracle
    frac = X[:1].copy()
    frac[0, 5] += 0.5
    two.add(frac, id_base=ID0, list_of_row=lor[:1])
    assert two.stats()["has_i8_copy"] == 0
    X1, lor1 = np.concatenate([X, frac]), np.concatenate([lor, lor[:1]])
    _equal(two.search(Q, 10), oracle.ivf_search(X1, C, lor1, Q, 10, NLIST, metric, id_base=ID0))
    _served(two, 0)
    for ix in (never, off, on, two):
        ix.close()

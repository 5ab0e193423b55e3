"""Option `ivf_sq8_kloop`: an IVF-SQ8 index of more than 128 dimensions scans its lists on the matrix cores straight from the 8-bit codes
(csrc/ivf_sq8_kloop.hpp).

Every search is compared bit for bit with oracle.ivf_search over the decoded rows, with the same handle's answer under `force_path` = 1
(the exact list scan) and with a fresh handle built under option 0.  `scan_dtype == 4` says the new kernel served the batch.

Shapes: nlist 8 with lists of 0, 1, 255, 256, 257, 1025 and two of 11 600 rows, filed by hand -- an empty list, a one-row list, both
sides of a 256-row span edge, one row past a 1024-row span, several spans and row parts.  The centroids of the short lists lie far out.
D = 132: one full K-step and a 4-byte tail chunk (D4 = 132); 192: exactly three K-steps; 200: a tail chunk that overlaps the one before
it; 1000: sixteen K-steps.

The (nprobe, k) pairs are those ivf_geometry admits: est_entries = nprobe x 4 x pspans / nlist >= 4 k.
  "ivf_tps" 16: spans of 256 rows, 0 + 1 + 1 + 1 + 2 + 5 + 46 + 46 = 102, 51 entries per probe: k = 1 and 10 at every nprobe, k = 100 at 8
  "ivf_tps" 64: spans of 1024 rows, 0 + 1 + 1 + 1 + 1 + 2 + 12 + 12 = 30, 15 entries per probe: k = 1 at every nprobe, k = 10 from 3 on

The fallback cap of a case is what an IVF-Flat handle over the decoded rows (same centroids, lists, queries, options: the fp16 K-loop
scan, which the parent commit has) counts, recorded in tests/golden/ivf_sq8_kloop_measurements.json, plus nq // 100.  The queries lie
about the two long lists: with a third of them about the 1025-row list (ten nearest rows in four 256-row bins) that reference itself
flagged up to 190 / 600 queries at "ivf_tps" 64, nprobe 3, k = 10 (more than nq // 20), so the inputs were changed, not the cap.
"""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import np_decode

pytestmark = pytest.mark.gpu

F32, ID0 = np.float32, 1000
SIZES = (0, 1, 255, 256, 257, 1025, 11600, 11600)
PAIRS = {16: ((1, 1), (1, 10), (3, 1), (3, 10), (8, 1), (8, 10), (8, 100)), 64: ((1, 1), (3, 1), (3, 10), (8, 1), (8, 10))}   # (nprobe, k)
NQS = (1, 70, 600)
GOLDEN = Path(__file__).parent / "golden" / "ivf_sq8_kloop_measurements.json"
# (metric, d, tps, group, adds): every d at both span sizes; quads and pairs once; one index filled by two adds
CASES = [(m, d, tps, 0, 1) for m in ("l2", "ip") for d in (132, 192, 200, 1000) for tps in (16, 64)] + \
        [("l2", 200, 16, 4, 1), ("ip", 192, 16, 2, 1), ("l2", 132, 16, 0, 2)]


def pairs_of(tps, group, adds):      # the extra cases (another candidate group, two adds) run the two widest pairs
    return PAIRS[tps] if adds == 1 and group == 0 else PAIRS[tps][-2:]


def case_key(metric, d, tps, group, nprobe, k, nq):
    return f"{metric}-d{d}-tps{tps}-g{group}-p{nprobe}-k{k}-q{nq}"


@functools.lru_cache(maxsize=None)
def data(d):
    rng = np.random.default_rng(d)
    lor = rng.permutation(np.repeat(np.arange(8), SIZES)).astype(np.int32)
    C = rng.standard_normal((8, d)).astype(F32)
    C[:5] += F32(6.0) * np.eye(8, d, dtype=F32)[:5]                          # the short lists: rarely a query's nearest
    X = (C[lor] + rng.standard_normal((len(lor), d))).astype(F32)
    Q = (C[rng.integers(6, 8, 600)] + rng.standard_normal((600, d))).astype(F32)   # (about the two long lists: see the module docstring)
    return X, C, lor, Q


def sq8_index(vdb, X, C, lor, metric, kloop, tps=0, group=0, adds=1, ranges=None):
    ix = vdb.IVFSQ8Index(X.shape[1], len(C), metric, 0, direct_kloop=kloop)
    ix.set_centroids(C)
    ix.train_ranges(X) if ranges is None else ix.set_ranges(*ranges)
    ix.set_option("ivf_tps", tps)
    ix.set_option("ivf_group", group)
    for part in np.array_split(np.arange(len(X)), adds):
        ix.add(X[part], id_base=ID0, list_of_row=lor[part])
    return ix


@pytest.mark.parametrize("metric,d,tps,group,adds", CASES)
def test_parity_with_the_oracle_the_exact_scan_and_option_0(vdb, oracle, metric, d, tps, group, adds):
    X, C, lor, Q = data(d)
    ix = sq8_index(vdb, X, C, lor, metric, True, tps, group, adds)
    off = sq8_index(vdb, X, C, lor, metric, None, tps, group, adds)
    np.testing.assert_array_equal(ix.assignment(), lor)
    Xh = np_decode(ix.codes(), C, lor, *ix.ranges())
    FLAT = json.loads(GOLDEN.read_text())["ivf_flat_fallback_queries"]
    for nprobe, k in pairs_of(tps, group, adds):
        Do, Io = oracle.ivf_search(Xh, C, lor, Q, k, nprobe, metric, id_base=ID0)     # (rows of a batch are independent: one reference)
        for nq in NQS:
            ix.set_nprobe(nprobe)
            D, I = ix.search(Q[:nq], k)
            st = ix.stats()
            cap = FLAT[case_key(metric, d, tps, group, nprobe, k, nq)] + nq // 100
            print(case_key(metric, d, tps, group, nprobe, k, nq), "fallback", st["last_fallback_queries"], "cap", cap, "candidates", st["last_candidates"])
            np.testing.assert_array_equal(I, Io[:nq])
            np.testing.assert_array_equal(D, Do[:nq])
            assert st["scan_dtype"] == 4 and st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st
            assert st["last_fallback_queries"] <= cap, (st, cap)
            ix.set_option("force_path", 1)
            De, Ie = ix.search(Q[:nq], k)
            assert ix.stats()["scan_dtype"] != 4
            ix.set_option("force_path", 0)
            off.set_nprobe(nprobe)
            D0, I0 = off.search(Q[:nq], k)
            assert off.stats()["scan_dtype"] != 4
            for Dx, Ix in ((De, Ie), (D0, I0)):
                np.testing.assert_array_equal(I, Ix)
                np.testing.assert_array_equal(D, Dx)
    ix.close()
    off.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_ties_are_ordered_as_the_float64_keys_order_them(vdb, oracle, metric):
    """The twin rows of tests/test_gpu_ivf_sq8_direct.py (equal keys | one code step apart where |q_d| <= 2^-20 ||q||) at D = 192, the
    special dimension in the third K-step: in one bin, across bins, across lists.  No query may be flagged."""
    d, dz, n = 192, 150, 8192
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
    ix = sq8_index(vdb, X, C, lor, metric, True, ranges=(np.full(d, -4.0, F32), np.full(d, 8.0, F32)))
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


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("scale", [1e-15, 1e15])
def test_hostile_ranges_and_an_infinite_query_stay_exact(vdb, oracle, scale, metric):
    X, C, lor, Q = data(192)
    ix = sq8_index(vdb, X, C, lor, metric, True, ranges=(np.full(192, -4.0 * scale, F32), np.full(192, 8.0 * scale, F32)))
    Xh = np_decode(ix.codes(), C, lor, *ix.ranges())
    ix.set_nprobe(8)
    Qi = Q[:70].copy()
    Qi[3, 5] = np.inf
    for q in (Q[:70], Qi):
        D, I = ix.search(q, 10)
        Do, Io = oracle.ivf_search(Xh, C, lor, q, 10, 8, metric, id_base=ID0)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)
    st = ix.stats()
    assert st["scan_dtype"] == 4 and st["last_fallback_queries"] == 70, st     # the infinite query flags its whole batch
    ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_resident_bytes_hold_no_rows_and_no_panels_and_a_multi_device_handle_refuses(vdb, metric):
    """Option 1 adds 4 bytes per list-padded row (the accumulator inits) and three small tables: no float32 rows (4 d bytes per row), no
    fp16 panels (2 d per padded row).  The constant (2 MiB) covers centroids, ranges, offsets, span tables and the coarse index of 8
    lists; `bytes_resident` counts the workspace of the searches as well, which is taken off."""
    X, C, lor, Q = data(192)
    ix = sq8_index(vdb, X, C, lor, metric, True, tps=16)
    ix.set_nprobe(3)
    ix.search(Q[:70], 10)
    st = ix.stats()
    padded = sum(-(-s // 256) for s in SIZES) * 256
    assert st["scan_dtype"] == 4 and st["bytes_resident"] - st["bytes_workspace"] < len(X) * (192 + 8) + 8 * padded + (2 << 20), (st, padded)
    ix.close()
    two = vdb.IVFFlatIndex(192, 8, metric, device=[0, 0])
    with pytest.raises(Exception, match="multi-device"):
        two.set_option("ivf_sq8_kloop", 1)
    two.set_option("ivf_sq8_kloop", 0)
    two.close()

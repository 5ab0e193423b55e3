"""Option `ivf_pq_kloop`: an IVF-PQ index of more than 128 dimensions scans its lists on the matrix cores straight from the product codes
(csrc/ivf_pq_kloop.hpp).

Every search is compared bit for bit with oracle.ivf_search over the decoded rows x^ (tests/ivfpq_restatement.decode on `codes()`), with
the same handle's answer under `force_path` = 1 (the exact list scan) and with a fresh handle built under option 0.  `scan_dtype == 5`
says the new kernel served the batch (on the parent commit it is never 5).

Shapes: nlist 8 with lists of 0, 1, 255, 256, 257, 1025 and two of 11 600 rows, filed by hand -- an empty list, a one-row list, both
sides of a 256-row span edge, one row past a 1024-row span, several spans and row parts.  The centroids of the short lists lie far out
and the queries lie about the two long lists (why: tests/test_gpu_ivf_sq8_kloop.py).  (d, M):
  192 / 24  dsub 8: no padding, three K-steps        192 / 16  dsub 12: P = 16, Kp = 256
  132 / 22  dsub 6: Kp = 176, a K-step tail behind Kp, D4 = 132, code rows that are no whole dwords
  136 /  8  dsub 17: odd, P = 24                     768 / 64  dsub 12: sixteen K-steps
  195 / 65  dsub 3: more than 64 code bytes per row -- the kernels with the 256-byte code pitch and the shallow ring (two cases)
The (nprobe, k) pairs are those ivf_geometry admits there (the table of the SQ8 test).

The fallback cap of a case is what an IVF-Flat handle over x^ (same centroids, lists, queries, options: the fp16 K-loop scan of the
parent commit) counts, recorded in tests/golden/ivf_pq_kloop_measurements.json, plus nq // 100.
"""
from __future__ import annotations

import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))      # (ivfpq_restatement imports its neighbour by its bare name)

from tests import ivfpq_restatement  # noqa: E402

pytestmark = pytest.mark.gpu

F32, ID0 = np.float32, 1000
SIZES = (0, 1, 255, 256, 257, 1025, 11600, 11600)
PAIRS = {16: ((1, 1), (1, 10), (3, 1), (3, 10), (8, 1), (8, 10), (8, 100)), 64: ((1, 1), (3, 1), (3, 10), (8, 1), (8, 10))}   # (nprobe, k)
NQS = (1, 70, 600)
GOLDEN = Path(__file__).parent / "golden" / "ivf_pq_kloop_measurements.json"
# (metric, d, M, tps, group, adds): every (d, M) at both span sizes; quads and pairs once; one index filled by two adds; M = 65
CASES = [(m, d, M, tps, 0, 1) for m in ("l2", "ip") for d, M in ((192, 24), (192, 16), (132, 22), (136, 8), (768, 64)) for tps in (16, 64)] + \
        [("l2", 192, 16, 16, 4, 1), ("ip", 192, 24, 16, 2, 1), ("l2", 132, 22, 16, 0, 2), ("l2", 195, 65, 16, 0, 1), ("ip", 195, 65, 64, 0, 1)]


def pairs_of(M, tps, group, adds):      # the extra cases run the two widest pairs
    return PAIRS[tps] if adds == 1 and group == 0 and M != 65 else PAIRS[tps][-2:]


def case_key(metric, d, M, tps, group, nprobe, k, nq):
    return f"{metric}-d{d}-m{M}-tps{tps}-g{group}-p{nprobe}-k{k}-q{nq}"


@functools.lru_cache(maxsize=None)
def data(d, M):
    rng = np.random.default_rng(1000 * d + M)
    lor = rng.permutation(np.repeat(np.arange(8), SIZES)).astype(np.int32)
    C = rng.standard_normal((8, d)).astype(F32)
    C[:5] += F32(6.0) * np.eye(8, d, dtype=F32)[:5]                          # the short lists: rarely a query's nearest
    X = (C[lor] + rng.standard_normal((len(lor), d))).astype(F32)
    Q = (C[rng.integers(6, 8, 600)] + rng.standard_normal((600, d))).astype(F32)
    cb = rng.standard_normal((M, 256, d // M)).astype(F32)
    return X, C, lor, Q, cb


def pq_index(vdb, X, C, lor, cb, metric, kloop, tps=0, group=0, adds=1):
    ix = vdb.IVFPQIndex(X.shape[1], len(C), cb.shape[0], metric, 0, direct_kloop=kloop)
    ix.set_centroids(C)
    ix.set_codebooks(cb)
    ix.set_option("ivf_tps", tps)
    ix.set_option("ivf_group", group)
    for part in np.array_split(np.arange(len(X)), adds):
        ix.add(X[part], id_base=ID0, list_of_row=lor[part])
    return ix


def check(ix, oracle, Xh, C, lor, Q, k, nprobe, metric):
    ix.set_nprobe(nprobe)
    D, I = ix.search(Q, k)
    st = ix.stats()
    Do, Io = oracle.ivf_search(Xh, C, lor, Q, k, nprobe, metric, id_base=ID0)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    return st


@pytest.mark.parametrize("metric,d,M,tps,group,adds", CASES)
def test_parity_with_the_oracle_the_exact_scan_and_option_0(vdb, oracle, metric, d, M, tps, group, adds):
    X, C, lor, Q, cb = data(d, M)
    ix = pq_index(vdb, X, C, lor, cb, metric, True, tps, group, adds)
    off = pq_index(vdb, X, C, lor, cb, metric, None, tps, group, adds)
    np.testing.assert_array_equal(ix.assignment(), lor)
    Xh = ivfpq_restatement.decode(ix.codes(), C, lor, cb)
    FLAT = json.loads(GOLDEN.read_text())["ivf_flat_fallback_queries"]
    for nprobe, k in pairs_of(M, tps, group, adds):
        Do, Io = oracle.ivf_search(Xh, C, lor, Q, k, nprobe, metric, id_base=ID0)     # (rows of a batch are independent: one reference)
        for nq in NQS:
            ix.set_nprobe(nprobe)
            D, I = ix.search(Q[:nq], k)
            st = ix.stats()
            cap = FLAT[case_key(metric, d, M, tps, group, nprobe, k, nq)] + nq // 100
            print(case_key(metric, d, M, tps, group, nprobe, k, nq), "fallback", st["last_fallback_queries"], "cap", cap, "candidates", st["last_candidates"])
            np.testing.assert_array_equal(I, Io[:nq])
            np.testing.assert_array_equal(D, Do[:nq])
            assert st["scan_dtype"] == 5 and st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st
            assert st["last_fallback_queries"] <= cap, (st, cap)
            ix.set_option("force_path", 1)
            De, Ie = ix.search(Q[:nq], k)
            assert ix.stats()["scan_dtype"] != 5
            ix.set_option("force_path", 0)
            off.set_nprobe(nprobe)
            D0, I0 = off.search(Q[:nq], k)
            assert off.stats()["scan_dtype"] != 5
            for Dx, Ix in ((De, Ie), (D0, I0)):
                np.testing.assert_array_equal(I, Ix)
                np.testing.assert_array_equal(D, Dx)
    ix.close()
    off.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_twin_rows_with_identical_codes_return_in_id_order(vdb, oracle, metric):
    """Twins of six rows of list 2 -- in the same bin, in another bin of the list, and in list 3, whose centroid equals list 2's -- are
    the same float32 rows, so their codes and their keys are equal: every pair must come back in id order, and no query may be flagged."""
    d, M, n = 192, 16, 8192
    rng = np.random.default_rng(5)
    C = rng.standard_normal((4, d)).astype(F32)
    C[3] = C[2]
    lor = np.repeat(np.arange(4), n // 4).astype(np.int32)
    X = (C[lor] + rng.standard_normal((n, d))).astype(F32)
    cb = rng.standard_normal((M, 256, d // M)).astype(F32)
    base = np.array([4200, 4300, 4400, 4500, 4600, 4700])                     # rows of list 2
    twin = np.array([4201, 5000, 6300, 4501, 5100, 6400])                     # same bin | another bin | list 3
    X[twin] = X[base]
    Q = np.repeat(X[base], 4, axis=0) + F32(0.05) * rng.standard_normal((24, d)).astype(F32)
    ix = pq_index(vdb, X, C, lor, cb, metric, True)
    codes = ix.codes()
    assert (codes[base] == codes[twin]).all()
    Xh = ivfpq_restatement.decode(codes, C, lor, cb)
    for nprobe in (2, 4):
        st = check(ix, oracle, Xh, C, lor, Q, 10, nprobe, metric)
        assert st["scan_dtype"] == 5 and st["last_candidates"] > 0 and st["last_fallback_queries"] == 0, st
    ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("scale", [1e-15, 1e15])
def test_hostile_codebooks_and_an_infinite_query_stay_exact(vdb, oracle, scale, metric):
    X, C, lor, Q, cb = data(192, 16)
    cbs = (cb * F32(scale)).astype(F32)
    ix = pq_index(vdb, X, C, lor, cbs, metric, True)
    Xh = ivfpq_restatement.decode(ix.codes(), C, lor, cbs)
    Qi = Q[:70].copy()
    Qi[3, 5] = np.inf
    for q in (Q[:70], Qi):
        st = check(ix, oracle, Xh, C, lor, q, 10, 8, metric)
    assert st["scan_dtype"] == 5 and st["last_fallback_queries"] == 70, st     # the infinite query flags its whole batch
    ix.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_resident_bytes_hold_no_rows_and_no_panels_and_a_multi_device_handle_refuses(vdb, metric):
    """Option 1 adds 4 bytes per list-padded row (the accumulator inits), 8 bytes per span, the fp16 table (M x 256 x P x 2 bytes) and 12
    bytes per dimension: no float32 rows, no fp16 panels.  The constant (2 MiB) covers centroids, codebooks, offsets, span tables and
    the coarse index of 8 lists; `bytes_resident` counts the workspace of the searches as well, which is taken off."""
    X, C, lor, Q, cb = data(192, 16)
    ix = pq_index(vdb, X, C, lor, cb, metric, True, tps=16)
    ix.set_nprobe(3)
    ix.search(Q[:70], 10)
    st = ix.stats()
    padded = sum(-(-s // 256) for s in SIZES) * 256
    bound = len(X) * (16 + 8) + 8 * padded + 16 * 256 * 16 * 2 + (2 << 20)
    assert st["scan_dtype"] == 5 and st["bytes_resident"] - st["bytes_workspace"] < bound, (st, bound)
    ix.close()
    two = vdb.IVFFlatIndex(192, 8, metric, device=[0, 0])
    with pytest.raises(Exception, match="multi-device"):
        two.set_option("ivf_pq_kloop", 1)
    two.set_option("ivf_pq_kloop", 0)
    two.close()

"""The stage ring of the int8 x16 batch loop (scan_i8x16_batch_loop, scan_i8x16.hpp; rules in scan_ring.hpp): three LDS buffers, the
stage after next issued behind the first MFMAs of a stage, tile 0 of the next stage read ahead of the stage barrier, biases by LDS-DMA,
and the bin flush of waves 4 - 7 half a step behind that of waves 0 - 3.  tests/test_gpu_scan_i8_pipelined.py stays the yardstick for
tile, span and chunk positions; this file adds the shapes at which a ring can go wrong.  Byte-valued corpora and integer queries
through `FlatIndex`, ids and float32 distances bit-equal to the CPU oracle:

  * chunks of 1 span (2 stages of 8 tiles: fewer stages than buffers), of 1 and 2 spans (4 stages: the ring wraps once; unequal
    chunks, chunk_rem != 0) and of 2 and 3 spans (6 stages: two wraps); N no multiple of 512 in all three corpora;
  * 1800 of 2048 queries: one wave partly and one wave fully padded -- the padded wave keeps issuing its share and taking barriers;
  * neighbours planted (a copy of the query and a +-1 perturbation of it; positions from `x16_row_in_span`) in the last tile of a stage
    and tile 0 of the next one (read across the barrier), in tile 0 of stage 3 (the first stage that reuses buffer 0; tile 8 of a
    chunk's second span with 8-tile stages, tile 12 of its first with 4-tile stages), and in tile 15 / tile 0 of consecutive spans for
    a query of waves 0 - 3 and one of waves 4 - 7 (the staggered flush), the wave following from the query's index in its tile;
  * l2 and ip, D = 64 and 128, the default index (both scans in one launch) and `int8_only`, `i8_variant` 3, 1 and 2 (8 / 4 column
    blocks per wave with 8-tile stages; 4-tile stages).

`rescan_bins` / `fallback_queries` of every search equal the values of the commit before the ring, recorded once in
tests/golden/scan_i8_ring_stats.json."""
from __future__ import annotations

import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
SPAN = 512
Q_EARLY, Q_LATE = 5, 1000      # query columns of wave 0 and of wave 7, in 1024-query tiles (128 per wave) and in 512-query tiles (64)


def x16_row_in_span(t, rb, m):      # scan_i8x16.hpp
    return (m >> 2) * 128 + t * 8 + rb * 4 + (m & 3)


def _geometry(n, nq, spans_per_chunk, k=K):
    """scan_geometry for the 32-row-tile layout (G = 2): the first span of every chunk, and nspans behind them."""
    G = 2
    nspans = (n + SPAN - 1) // SPAN
    spc_hi = nspans * G // (4 * k)
    spc_lo = (nspans * G + 1023) // 1024
    assert spc_hi >= 1 and spc_hi >= spc_lo
    spc = max(min(spans_per_chunk if spans_per_chunk > 0 else 32 // G, spc_hi), spc_lo)
    if spc < 2 and nspans * G >= 128:
        spc = min(2, spc_hi)
    nchunks = (nspans + spc - 1) // spc
    if nchunks >= 16:
        n8 = (nchunks + 7) // 8 * 8
        if n8 * G <= 1024 and nspans // n8 >= 1:
            nchunks = n8
    cap = 256 // G
    if nq > 512 and spans_per_chunk == 0 and cap < nchunks <= 2 * cap and cap * G >= 4 * k:
        nchunks = cap
    spc, rem = nspans // nchunks, nspans % nchunks
    starts = [c * spc + min(c, rem) for c in range(nchunks + 1)]
    assert starts[-1] == nspans
    return starts


def _bytes(rng, n, d):
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(np.float32)


def _planted(n, nq, starts):
    """[(query, row of the copy, row of the +-1 neighbour)]"""
    sizes = np.diff(starts)
    c = int(np.argmax(sizes))                 # a chunk of the largest size, and its first span s: s + 1 is in the chunk if any chunk has 2
    s = starts[c]
    assert s + 1 < starts[-1] - 1             # (both spans are whole)
    row = lambda span, t, rb, m: span * SPAN + x16_row_in_span(t, rb, m)
    return [
        (0, row(s, 7, 1, 15), row(s, 8, 0, 0)),                    # last tile of a stage / tile 0 of the next, read across the barrier
        (127, row(s + 1, 8, 0, 6), row(s, 12, 1, 9)),              # tile 0 of stage 3: 8-tile stages / 4-tile stages
        (Q_EARLY, row(s, 15, 1, 3), row(s + 1, 0, 0, 12)),         # tile 15 / tile 0 of consecutive spans, a wave that flushes behind step 0
        (Q_LATE, row(s, 15, 0, 10), row(s + 1, 0, 1, 5)),          # ... and one that flushes between the halves of step 1
        (nq - 1, n - 1, row(starts[-1] - 1, 0, 0, 1)),             # the last valid row of the corpus
    ]


_CASES = {}      # data and oracle results, computed once per (corpus, batch, metric) and shared by the index kinds; never modified


def _case(oracle, n, d, nq, spans_per_chunk, metric, count=64):
    key = (n, d, nq, spans_per_chunk, metric)
    if key not in _CASES:
        rng = np.random.default_rng(n + d)
        X, Q = _bytes(rng, n, d), _bytes(rng, nq, d)
        starts = _geometry(n, nq, spans_per_chunk)
        planted = _planted(n, nq, starts)
        rows = [r for _, a, b in planted for r in (a, b)]
        assert len(set(rows)) == len(rows) and max(rows) < n
        for qi, ra, rb in planted:
            X[ra] = Q[qi]
            X[rb] = Q[qi]
            j = int(rng.integers(0, d))
            X[rb, j] += 1.0 if X[rb, j] < 255 else -1.0
        qsel = np.array([qi for qi, _, _ in planted], np.int64)
        rest = np.setdiff1d(np.linspace(0, nq - 1, count, dtype=np.int64), qsel)
        which = np.concatenate([qsel, rest])[:count]
        Do, Io = oracle.knn(X, Q[which], K, metric)
        for qi, ra, rb in planted:          # l2: the planted rows lead their query's list, the copy at distance 0, then the neighbour
            r = int(np.nonzero(which == qi)[0][0])
            assert metric != "l2" or (Io[r, 0] == ra and Io[r, 1] == rb), (qi, ra, rb, Io[r, :3])
        for a in (X, Q, which, Do, Io):
            a.setflags(write=False)
        _CASES[key] = (X, Q, starts, which, Do, Io)
    return _CASES[key]


def _search(idx, Q, stats, key):
    D, I = idx.search(Q, K)
    st = idx.stats()
    # the int8 x16 batch scan served the batch
    assert st["last_path_name"] == "mfma_scan" and st["scan_dtype"] == 1 and st["scan_shape"] == 16, st
    stats[key] = [int(st["last_rescan_bins"]), int(st["last_fallback_queries"])]
    print(f"{key}: rescan_bins, fallback_queries = {stats[key]}")
    return D, I


# n, nq, spans_per_chunk, chunk sizes: every case reaches nchunks x Qpad / 1024 >= 256 workgroups of 1024 queries
SHAPES = {
    32_100: (5120, 1, {1}),           # 63 chunks of one span, 5 query tiles
    127_900: (2048, 2, {1, 2}),       # 250 spans over 128 chunks, chunk_rem = 122
    190_000: (2048, 3, {2, 3}),       # 372 spans over 128 chunks, chunk_rem = 116
}
CASES = [("l2", 128, 32_100), ("ip", 64, 32_100), ("ip", 128, 127_900), ("l2", 64, 127_900), ("l2", 128, 190_000), ("ip", 64, 190_000)]


def run_case(vdb, oracle, metric, d, n, kind):
    """Every search of one case, checked against the oracle -> {key: [rescan_bins, fallback_queries]}"""
    nq, spc, sizes = SHAPES[n]
    X, Q, starts, which, Do, Io = _case(oracle, n, d, nq, spc, metric)
    assert set(np.diff(starts).tolist()) == sizes, set(np.diff(starts).tolist())
    assert (len(starts) - 1) * (nq // 1024) >= 256 and nq % 1024 == 0, "the 1024-query tiles are not reached"
    idx = vdb.FlatIndex(d, metric, 0)
    if kind == "int8_only":
        idx.set_option("int8_only", 1)
    idx.set_option("spans_per_chunk", spc)
    idx.add(X)
    stats, full = {}, {}
    for variant in (3, 1, 2):       # 8-tile stages with 8 and with 4 column blocks per wave; 4-tile stages with 8
        idx.set_option("i8_variant", variant)
        D, I = _search(idx, Q, stats, f"{metric}-{d}-{n}-{kind}-v{variant}-nq{nq}")
        np.testing.assert_array_equal(I[which], Io)
        np.testing.assert_array_equal(D[which], Do)
        full[variant] = (D, I)
    for variant in (1, 2):
        np.testing.assert_array_equal(full[3][1], full[variant][1])
        np.testing.assert_array_equal(full[3][0], full[variant][0])
    # 248 query columns short of the last 1024-query tile (1800 of 2048; 4872 of 5120): its wave 6 holds 8 queries, its wave 7 none
    idx.set_option("i8_variant", 3)
    D, I = _search(idx, Q[: nq - 248], stats, f"{metric}-{d}-{n}-{kind}-v3-nq{nq - 248}")
    np.testing.assert_array_equal(I, full[3][1][: nq - 248])
    np.testing.assert_array_equal(D, full[3][0][: nq - 248])
    idx.close()
    return stats


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "scan_i8_ring_stats.json").read_text())["recorded"]


@pytest.mark.parametrize("kind", ["default", "int8_only"])
@pytest.mark.parametrize("metric,d,n", CASES)
def test_ring_scan(vdb, oracle, recorded, metric, d, n, kind):
    stats = run_case(vdb, oracle, metric, d, n, kind)
    assert len(stats) == 4
    for key, got in stats.items():
        assert key in recorded, f"{key} is not recorded in tests/golden/scan_i8_ring_stats.json"
        assert got == recorded[key], (key, got, recorded[key])

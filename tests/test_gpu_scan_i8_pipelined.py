"""The software-pipelined batch loop of the int8 x16 scan (scan_i8x16_batch_loop, scan_i8x16.hpp): a step issues the MFMAs of tile t
and retires tile t-1 in their gaps, so the select of a tile, the flush of a bin and the drain after the last stage all happen one tile
later than the arithmetic.  Byte-valued corpora and integer queries through `FlatIndex`, ids and float32 distances bit-equal to the CPU
oracle, at the shapes where a deferred select can go wrong:

  * chunks of 1 span (the drain comes right after the first bin), of 2 spans, unequal chunks (chunk_rem != 0), N not a multiple of 512;
  * a query count that leaves one wave partly and one wave fully padded (1800 of 2048);
  * neighbours planted (distance 0 and a +-1 perturbation) in tile 0 and tile 15 of a span, in the first and the last span of a chunk,
    in the last stage of the last chunk and in the last valid row of the corpus -- positions derived from `x16_row_in_span`;
  * l2 and ip, D = 64 (one 64-dim k-step) and 128 (two), the default index (both scans in one launch) and an `int8_only` index (the
    int8 scan as its own kernel), `i8_variant` 3 and 1 (8 and 4 column blocks per wave; 1024- and 512-query tiles), and the default
    geometry with 1100 queries (512-query tiles).

The geometry of `scan_geometry` (search_flat.inc) is restated below to place the planted rows and to FAIL, not skip, when a case would
not reach the 1024-query tiles (nchunks x Qpad / 1024 >= 256).  One shape of the issue cannot be produced through `FlatIndex`: a last
chunk cut by `nspans` -- chunk_span0 deals exactly nspans spans over the chunks, so the kernel's clamp never acts for a flat index.

`rescan_bins` / `fallback_queries` of every case equal the values of the build before the loop was pipelined, recorded once in
tests/golden/scan_i8_pipelined_stats.json."""
from __future__ import annotations

import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
SPAN = 512


def x16_row_in_span(t, rb, m):      # scan_i8x16.hpp
    return (m >> 2) * 128 + t * 8 + rb * 4 + (m & 3)


def _geometry(n, nq, spans_per_chunk, k=K):
    """scan_geometry for the 32-row-tile layout (G = 2): (nspans, [first span of chunk c ...] + [nspans])."""
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
    return nspans, starts


def _bytes(rng, n, d):
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(np.float32)


def _planted_rows(n, starts):
    """(row of the copy, row of the +-1 neighbour) per planted query: each at a tile / span position named in the module docstring."""
    nchunks = len(starts) - 1
    mid = nchunks // 2
    two = next(c for c in range(nchunks) if starts[c + 1] - starts[c] >= 2) if max(np.diff(starts)) >= 2 else mid
    last_span = starts[-1] - 1
    pos = [
        (starts[mid] * SPAN + x16_row_in_span(0, 0, 0), starts[mid] * SPAN + x16_row_in_span(15, 1, 15)),          # tile 0 / tile 15, first span of a chunk
        ((starts[two + 1] - 1) * SPAN + x16_row_in_span(15, 0, 5), (starts[two + 1] - 1) * SPAN + x16_row_in_span(0, 1, 10)),   # last span of a chunk
        (starts[two] * SPAN + x16_row_in_span(15, 1, 3), starts[two] * SPAN + x16_row_in_span(7, 0, 12)),             # tile 15 of a first span, end of a stage
        (starts[-2] * SPAN + x16_row_in_span(0, 1, 6), starts[-2] * SPAN + x16_row_in_span(8, 0, 9)),                # last chunk: first tile, first tile of a stage
        (n - 1, last_span * SPAN + x16_row_in_span(0, 0, 1)),                                                       # the last valid row of the corpus
    ]
    # the last stage (tiles 8..15) of the last chunk, as far as the corpus reaches into it
    tail = [r for t in range(8, 16) for rb in (0, 1) for m in range(16) if (r := last_span * SPAN + x16_row_in_span(t, rb, m)) < n - 1]
    if len(tail) >= 2:
        pos.append((tail[-1], tail[0]))
    return [(a, b) for a, b in pos if a < n and b < n and a != b]


_CASES = {}      # data and oracle results, computed once per (corpus, batch, metric) and shared by the index kinds; never modified


def _case(oracle, n, d, nq, spans_per_chunk, metric, count):
    key = (n, d, nq, spans_per_chunk, metric)
    if key not in _CASES:
        X, Q, starts, qsel = _make_case(n, d, nq, spans_per_chunk, seed=n + d)
        which = _sample(nq, qsel, count)
        Do, Io = oracle.knn(X, Q[which], K, metric)
        for a in (X, Q, which, Do, Io):
            a.setflags(write=False)
        _CASES[key] = (X, Q, starts, which, Do, Io)
    return _CASES[key]


def _make_case(n, d, nq, spans_per_chunk, seed):
    rng = np.random.default_rng(seed)
    X, Q = _bytes(rng, n, d), _bytes(rng, nq, d)
    nspans, starts = _geometry(n, nq, spans_per_chunk)
    planted = _planted_rows(n, starts)
    rows = [r for pair in planted for r in pair]
    assert len(set(rows)) == len(rows)
    # the planted queries: spread over the batch -- first and last wave of a workgroup, both halves, the last valid query
    qsel = [0, 127, 128, nq // 2 + 5, nq - 129, nq - 1][: len(planted)]
    for qi, (ra, rb) in zip(qsel, planted):
        X[ra] = Q[qi]
        X[rb] = Q[qi]
        j = int(rng.integers(0, d))
        X[rb, j] += 1.0 if X[rb, j] < 255 else -1.0
    return X, Q, starts, qsel


def _sample(nq, qsel, count):
    """The planted queries first, then evenly spaced ones (count == nq: every query)."""
    rest = np.setdiff1d(np.linspace(0, nq - 1, count, dtype=np.int64), np.array(qsel))
    return np.concatenate([np.array(qsel, np.int64), rest])[:count]


def _index(vdb, X, metric, kind, **opts):
    idx = vdb.FlatIndex(X.shape[1], metric, 0)
    if kind == "int8_only":
        idx.set_option("int8_only", 1)
    for name, value in opts.items():
        idx.set_option(name, value)
    idx.add(X)
    return idx


def _search(idx, Q, recorded, key):
    D, I = idx.search(Q, K)
    st = idx.stats()
    # the int8 x16 batch scan served the batch
    assert st["last_path_name"] == "mfma_scan" and st["scan_dtype"] == 1 and st["scan_shape"] == 16, st
    got = [int(st["last_rescan_bins"]), int(st["last_fallback_queries"])]
    print(f"{key}: rescan_bins, fallback_queries = {got}")
    _compare(recorded, key, got)
    return D, I


def _compare(recorded, key, got):
    assert key in recorded, f"{key} is not recorded in tests/golden/scan_i8_pipelined_stats.json"
    assert got == recorded[key], (key, got, recorded[key])


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "scan_i8_pipelined_stats.json").read_text())["recorded"]


# 127 900 rows: 250 spans dealt over 128 chunks of 1 and 2 spans (chunk_rem = 122), N no multiple of 512, the last span half empty;
# 131 072 rows: 256 spans, 128 equal chunks of 2.  Both reach 128 x 2048 / 1024 = 256 workgroups of 1024 queries.
@pytest.mark.parametrize("kind", ["default", "int8_only"])
@pytest.mark.parametrize("metric,d,n", [("l2", 128, 127_900), ("ip", 128, 131_072), ("l2", 64, 131_072), ("ip", 64, 127_900)])
def test_pipelined_scan_1024_query_tiles(vdb, oracle, recorded, metric, d, n, kind):
    nq = 2048
    X, Q, starts, which, Do, Io = _case(oracle, n, d, nq, 2, metric, 64)
    sizes = set(np.diff(starts).tolist())
    assert sizes == ({1, 2} if n == 127_900 else {2}), sizes
    assert (len(starts) - 1) * (nq // 1024) >= 256, "the 1024-query tiles are not reached"
    idx = _index(vdb, X, metric, kind, spans_per_chunk=2)
    full = {}
    for variant in (3, 1):          # 8 column blocks per wave and 1024-query tiles; 4 and 512
        idx.set_option("i8_variant", variant)
        D, I = _search(idx, Q, recorded, f"{metric}-{d}-{n}-{kind}-v{variant}-nq{nq}")
        np.testing.assert_array_equal(I[which], Io)
        np.testing.assert_array_equal(D[which], Do)
        full[variant] = (D, I)
    np.testing.assert_array_equal(full[3][1], full[1][1])
    np.testing.assert_array_equal(full[3][0], full[1][0])
    # 1800 of 2048 query columns: the wave of columns 1792.. holds 8 queries, the wave of columns 1920.. none
    idx.set_option("i8_variant", 3)
    D, I = _search(idx, Q[:1800], recorded, f"{metric}-{d}-{n}-{kind}-v3-nq1800")
    np.testing.assert_array_equal(I, full[3][1][:1800])
    np.testing.assert_array_equal(D, full[3][0][:1800])
    idx.close()


@pytest.mark.parametrize("kind", ["default", "int8_only"])
@pytest.mark.parametrize("metric,d", [("l2", 128), ("ip", 64)])
def test_pipelined_scan_default_geometry_512_query_tiles(vdb, oracle, recorded, metric, d, kind):
    """Default options, 1100 queries (Qpad 1536 is no multiple of 1024): 512-query tiles, 4 column blocks per wave; 137 spans over 24
    chunks of 5 and 6; every query against the oracle."""
    n, nq = 70_001, 1100
    X, Q, starts, which, Do, Io = _case(oracle, n, d, nq, 0, metric, nq)
    assert set(np.diff(starts).tolist()) == {5, 6} and len(which) == nq
    idx = _index(vdb, X, metric, kind)
    D, I = _search(idx, Q, recorded, f"{metric}-{d}-{n}-{kind}-default-nq{nq}")
    np.testing.assert_array_equal(I[which], Io)
    np.testing.assert_array_equal(D[which], Do)
    idx.close()

"""Census of the flat PQ<M> index: every decoded row is a query, through every launch branch of the panel pass.

The refine re-scores candidates exactly from the codes, so a wrong panel -- one tile of a slab made from the wrong rows, one k-step
slice gathering from the neighbouring sub-space's table, a code >= 128 read as signed -- never shows in a returned distance: it only
keeps the damaged rows from becoming candidates, and parity on a random corpus sees the few per cent of rows that are somebody's
neighbour.  Here the codebooks and codes are injected (tests/census_coded.py) so that every decoded row x^ is its own strict nearest
neighbour and a planted twin (partner masks of census.MASKS over the 2048-row blocks) its strict second; every row is a query:

  * plain census, k = 1, natural order; twin census, k = 2, stride order -- on ONE index (every coded corpus carries its twins);
  * ids of all N queries against the Gram reference over x^, distances too on the integer kind, the 64-row sample bit-equal to
    oracle.knn over x^; no tolerance anywhere;
  * after every call: `last_path_name`, `scan_dtype` (2 = fp16 panels made from codes, what vdb_stats reports for a PQ handle on the
    MFMA scan; 0 on the exact kernels), `scan_shape` and, on the scan, `last_fallback_queries` 0;
  * before anything runs, from the restated launch_pq_panels / scan_in_slabs / scan geometry: the case reaches the branch it names.

Rows as in the flat census: 17 409 / 17 508 (D <= 128: 35 spans, the last holding 1 / 100 rows) and 18 433 / 18 443 (D > 128: 19 spans,
the last holding 1 / 11), `spans_per_chunk` 2 and `force_path` 2: chunks of one and of two spans, and a tail run that ends at N M.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import census
from tests import census_coded as cc
from tests.test_gpu_census_flat import census_run, check

pytestmark = pytest.mark.gpu

SCAN_OPTS = {"force_path": 2, "spans_per_chunk": 2}
# what each shape of cc.PQ_SHAPES is there for: (layout p16, gather width W, dword staging, table form, grid y, steps of the last slice)
BRANCH = {
    (64, 8): (False, 8, True, "lds", 1, 2), (128, 32): (False, 4, True, "lds", 1, 4), (100, 50): (False, 2, False, "lds", 1, 4),
    (50, 50): (False, 1, False, "lds", 1, 2), (128, 128): (False, 1, True, "cache", 1, 4), (384, 64): (True, 2, True, "sliced", 4, 3),
    (384, 96): (True, 4, True, "sliced", 3, 4), (200, 25): (True, 8, False, "sliced", 2, 4), (240, 16): (True, 1, True, "cache", 1, 8),
    (320, 40): (True, 8, True, "sliced", 3, 2)}


def _reaches(d, M, n, nq):
    """The restated launch choices of this shape: the panel branch it names, chunks of one and of two spans, a partly filled last span."""
    L = cc.pq_panel_launch(d, M)
    assert (L["p16"], L["W"], L["vec"], L["table"], L["gy"], L["last"]) == BRANCH[(d, M)], L
    assert L["pad8"] == (d in (50, 100)) and L["partial"] == (d in (50, 100, 200, 240))
    g = census.scan_geometry(n, d, 2, nq, 2)
    assert g.ok and g.chunk_sizes() == {1, 2} and n % census.span_rows(d) in (1, 11, 100)
    assert (g.nspans, g.nchunks, g.rem) == ((19, 10, 9) if d > 128 else (35, 24, 11))
    return g


def _index(vdb, c, metric, opts):
    idx = vdb.PQIndex(c.d, c.M, metric, 0)
    for name, value in opts.items():
        idx.set_option(name, value)
    idx.set_codebooks(c.cb)
    idx.add_codes(c.codes)
    return idx


def run_case(vdb, oracle, c, metric, opts, nq, expect):
    """Both censuses on one index built from the injected codebooks and codes."""
    c.ref("twin", metric, 2)                   # (the reference first: it asserts, on the CPU, that x^ is a census corpus)
    n = c.n
    idx = _index(vdb, c, metric, opts)
    stride = census.stride_order(n, 4099 if n % 4099 else 4093)
    for which, k, order in (("plain", 1, np.arange(n)), ("twin", 2, stride)):
        D, I = census_run(idx, c.X, nq, k, order, expect)
        check(oracle, c, which, metric, k, D, I)
    idx.close()


def _scan(d):
    return {"last_path_name": "mfma_scan", "scan_dtype": 2, "last_fallback_queries": 0, "scan_shape": 16 if d <= 128 else 0,
            "has_i8_copy": 0}


def _metric(i):
    return ("l2", "ip")[i % 2]


@pytest.mark.parametrize("nq", [40, 700])
@pytest.mark.parametrize("d,M,construction,kind,n", cc.PQ_SHAPES, ids=lambda v: str(v))
def test_panel_pass(vdb, oracle, d, M, construction, kind, n, nq):
    """pq_panels_kernel<W, LDS> in every branch of launch_pq_panels (BRANCH), one slab (the default `pq_slab_chunks`), serving-shaped
    (40 queries, one wave) and batch-shaped (700) scans behind it."""
    g = _reaches(d, M, n, nq)
    assert cc.slab_cut(g, d) == [(0, g.nchunks, 0, g.nspans)]
    c = cc.case(construction, kind, n, d, M)
    run_case(vdb, oracle, c, _metric(d // 2 + M + nq // 40), SCAN_OPTS, nq, _scan(d))


@pytest.mark.parametrize("d,M,construction,kind,n", [cc.PQ_SHAPES[0], cc.PQ_SHAPES[7]], ids=lambda v: str(v))
def test_panel_pass_256_queries(vdb, oracle, d, M, construction, kind, n):
    """256 queries per call (four waves of the serving shape) on an x16 and a p16 shape."""
    _reaches(d, M, n, 256)
    assert census.nw_small(256) == 4
    run_case(vdb, oracle, cc.case(construction, kind, n, d, M), _metric(M), SCAN_OPTS, 256, _scan(d))


@pytest.mark.parametrize("d,M,construction,kind,n", cc.PQ_SHAPES, ids=lambda v: str(v))
def test_add_encodes_the_decoded_rows_to_the_injected_codes(vdb, d, M, construction, kind, n):
    """vdb_pq_add over x^ gives back the injected codes: every used entry is the unique nearest entry of its own sub-vector."""
    c = cc.case(construction, kind, n, d, M)
    idx = vdb.PQIndex(d, M, "l2", 0)
    idx.set_codebooks(c.cb)
    idx.add(c.X)
    np.testing.assert_array_equal(idx.codes(), c.codes)
    idx.close()


X16_SLABS, P16_SLABS = cc.PQ_SHAPES[2] + (700,), cc.PQ_SHAPES[10] + (40,)


@pytest.mark.parametrize("d,M,construction,kind,n,nq,chunks", [X16_SLABS + (1,), X16_SLABS + (3,), X16_SLABS + (5,), P16_SLABS + (1,),
                                                               P16_SLABS + (3,)], ids=lambda v: str(v))
def test_slabs(vdb, oracle, d, M, construction, kind, n, nq, chunks):
    """scan_in_slabs with `pq_slab_chunks` 1, 3 and 5 (the default, one slab: test_panel_pass): `tile0`, `ntiles` and the rebased
    `panels` differ per slab.  D = 128 (24 chunks, the first 11 of two spans): slabs begin behind two-span and behind one-span chunks,
    3 chunks give slabs of 6, 5 and 3 spans, 5 chunks a short last slab of four chunks.  D = 320 (10 chunks, the first 9 of two spans): 3
    chunks leave a last slab of ONE one-span chunk, the partly filled last span."""
    g = _reaches(d, M, n, nq)
    cut = cc.slab_cut(g, d, chunks)
    assert len(cut) == -(-g.nchunks // chunks) > 1 and sum(s[1] for s in cut) == g.nchunks and sum(s[3] for s in cut) == g.nspans
    assert {g.starts[c0] - g.starts[c0 - 1] for c0, _, _, _ in cut[1:]} == ({1, 2} if d <= 128 else {2})
    assert len({s[3] for s in cut}) > 1                    # slabs of different numbers of spans
    if (d, chunks) in ((128, 5), (320, 3)):
        assert cut[-1][1] < chunks                         # the last slab is short
    run_case(vdb, oracle, cc.case(construction, kind, n, d, M), _metric(chunks), dict(SCAN_OPTS, pq_slab_chunks=chunks), nq, _scan(d))


@pytest.mark.parametrize("nq,blocked", [(40, False), (1024, True)])
@pytest.mark.parametrize("d,M,construction,kind,n", [cc.PQ_SHAPES[3], cc.PQ_SHAPES[8]], ids=lambda v: str(v))
def test_exact_kernels_on_the_codes(vdb, oracle, d, M, construction, kind, n, nq, blocked):
    """`pq_scan_min_batch` above the batch: the exhaustive float64 kernels read x^ through pq_key (refine.hpp), one wave per query
    (40 queries) and query-blocked (1024 queries: 256 groups x 8 splits)."""
    assert census.exact_blocked(nq, n, 2) == blocked and census.exact_blocked(nq, n, 1) == blocked
    run_case(vdb, oracle, cc.case(construction, kind, n, d, M), _metric(nq), {"pq_scan_min_batch": 100_000}, nq,
             {"last_path_name": "exact_scan", "scan_dtype": 0})

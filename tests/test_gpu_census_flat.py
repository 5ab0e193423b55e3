"""Census of the flat search: every row of a corpus is a query, through every launch shape of search_flat.inc.

A census corpus (tests/census.py) makes every row the strict nearest neighbour of exactly one query -- itself -- and a partner row its
second, so a scan that loses, or wrongly returns, the rows of ONE tile, stage, span, chunk or slab position fails for exactly those rows;
a random corpus only checks the rows that land in some query's top-k.  Every case runs

  * the plain census: k = 1 on the plain corpus, queries in natural order;
  * the twin census: k = 2 on the mixed-twin corpus (the seven partner masks 4 .. 1024 dealt over its 2048-row blocks: other quad,
    neighbouring group, other tile / 128-row block of the same 256-row bin -- the bin's second minimum and the exact re-scan --, the
    other bin of the span, the next span), queries in a stride order so that a row meets another query column than its own offset.

Asserted per case: ids of ALL N queries equal the exact Gram-matrix reference; distances of all N queries on the integer kinds; the
whole (D, I) of a fixed 64-query sample bit-equal to the CPU oracle; after EVERY call the statistics that prove the path (path name,
scan_dtype, scan_shape, has_i8_copy, fallback count); and, before anything runs, the restated geometry's preconditions for the shape
the case names (it fails, never skips, when the shape is not reached).  Calls always carry `nq` queries: the last one wraps around.

Shapes of N (D <= 128, 512-row spans): 17 409 rows = 35 spans, the last holding ONE row; 17 508 rows = 35 spans, the last holding 100.
With `spans_per_chunk` = 2 the 35 spans are dealt over 24 chunks: 11 of two spans (chunk_rem = 11) and 13 of one.  D > 128 (1024-row
spans): 18 433 / 18 443 rows = 19 spans, the last holding 1 / 11 rows, ten chunks of 2 and 1 spans (chunk_rem = 9).  `force_path` = 2
lets these corpora reach the scan below 32 768 rows.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import census

pytestmark = pytest.mark.gpu

N1, N100 = 17_409, 17_508          # D <= 128
K1, K11 = 18_433, 18_443           # D > 128
NWIDE = 26_625                     # 53 one-span chunks x 5 tiles of 1024 queries = 265 >= 256 workgroups
NI8 = 33_803                       # above the int8_only threshold: 67 spans, the last holding 11 rows

SCAN = {"last_path_name": "mfma_scan", "last_fallback_queries": 0}
F16 = dict(SCAN, scan_dtype=0)
# Direct bins serve large k; the default work list (2 k + 32 candidates) can overflow there, which sends a query to the exact fallback
# and would hide what the direct-bin select did.  `list_cap` 4096 holds every level-1 bin of these corpora, so the candidate list cannot
# overflow.  The re-scan list cannot be sized: it holds max(16, k / 2 + 8) bins, and select_kernel takes its threshold from the two
# smallest minima of every lane, which may lie above the k-th smallest minimum and admit more than k bins; on these corpora, where all
# rows but two are nearly equidistant from a query, the second minimum of an admitted bin is often below the threshold too.  Measured:
# at most 1 query of a 700-query call falls back, in a few calls of a census.  Required: no more than 1 % of any call, so that the
# direct-bin select answers at least 99 % of the queries at every position.
DIRECT = dict(F16, last_fallback_queries=lambda nq: range(nq // 100 + 1))
DIRECT_OPTS = {"force_path": 2, "spans_per_chunk": 2, "list_cap": 4096}
I8 = dict(SCAN, scan_dtype=1, has_i8_copy=1)


def _index(vdb, rows, metric, opts, device=0):
    idx = vdb.FlatIndex(rows.shape[1], metric, device)
    for name, value in opts.items():          # (before the add: the layout options take effect there)
        idx.set_option(name, value)
    idx.add(rows)
    return idx


def census_run(idx, C, nq, k, order, expect, queries=None):
    """Query with every row of C (or the row-aligned `queries`) in calls of exactly `nq` rows; (D, I) stacked in row order.  After every
    call the statistics must equal `expect` (a value may be a callable of the call's query count)."""
    n = len(C)
    Q = C if queries is None else queries
    D = np.full((n, k), np.nan, np.float32)
    I = np.full((n, k), -7, np.int64)
    for b0 in range(0, n, nq):
        sel = order[np.arange(b0, b0 + nq) % n]
        d, i = idx.search(Q[sel], k)
        st = idx.stats()
        for key, want in expect.items():
            want = want(nq) if callable(want) else want
            assert st[key] in want if isinstance(want, range) else st[key] == want, (key, st[key], want, b0)
        D[sel], I[sel] = d, i
    assert (I != -7).all()
    return D, I


def check(oracle, c, which, metric, k, D, I, kref=None):
    """ids (and, integer kinds, distances) of all rows against the Gram reference in the first `kref` columns; the 64-row sample
    bit-equal to the oracle in all k columns."""
    kref = min(k if kref is None else kref, c.kmax(which))
    Dr, Ir = c.ref(which, metric, kref)
    np.testing.assert_array_equal(I[:, 0], Ir[:, 0])
    if c.exact:
        np.testing.assert_array_equal(I[:, :kref], Ir)
        np.testing.assert_array_equal(D[:, :kref], Dr)
    elif kref > 1:          # (gauss: the second neighbour is certain for the rows that have a twin)
        has = c.partner(which) >= 0
        np.testing.assert_array_equal(I[has, 1], Ir[has, 1])
    s = census.sample_rows(c.n)
    rows = c.rows(which)
    Do, Io = oracle.knn(rows, rows[s], k, metric)
    np.testing.assert_array_equal(I[s], Io)
    np.testing.assert_array_equal(D[s], Do)


def twin_of(rot):
    """The twin corpus whose deal of the masks over the 2048-row blocks is rotated by rot % 3 blocks.  At 17 409 rows the masks 64 and 128
    (same bin, other tile / 128-row block) lie in two-span chunks at rotation 0, and at 1 and 2 in the one-span chunks and the partly
    filled last span; the cases of a family take the three rotations in turn."""
    return ("twin", "twin1", "twin2")[rot % 3]


def run_case(vdb, oracle, c, metric, opts, nq, expect, rot=0, device=0, twin_only=False):
    """Both censuses of one case on indexes built with `opts`."""
    n = c.n
    stride = census.stride_order(n, 4099 if n % 4099 else 4093)
    for which, k, order in (("plain", 1, np.arange(n)), (twin_of(rot), 2, stride)):
        if twin_only and which == "plain":
            continue
        idx = _index(vdb, c.rows(which), metric, opts, device)
        D, I = census_run(idx, c.rows(which), nq, k, order, expect)
        idx.close()
        check(oracle, c, which, metric, k, D, I)


def _metric(i):
    return ("l2", "ip")[i % 2]


def _std(n, d, k, nq, spc=2, **want):
    """The standard geometry at this shape, with the properties the case relies on."""
    g = census.scan_geometry(n, d, k, nq, spc)
    assert g.ok and n % census.span_rows(d) != 0
    for key, value in want.items():
        got = {"sizes": g.chunk_sizes(), "rem": g.rem, "nchunks": g.nchunks}[key]
        assert got == value, (key, got, value)
    return g


# ---- layout x16, fp16 ---------------------------------------------------------------------------------------------------------
X16_F16_SERVING = [(kind, d, n, nq) for (kind, d, n) in (("wide", 64, N1), ("gauss", 128, N100)) for nq in (40, 64, 128, 256)] + \
                  [("gauss", 64, N100, 40), ("wide", 128, N1, 256)]


@pytest.mark.parametrize("i,kind,d,n,nq", [(i,) + t for i, t in enumerate(X16_F16_SERVING)], ids=lambda v: str(v))
def test_x16_fp16_serving(vdb, oracle, i, kind, d, n, nq):
    """scan_x16_kernel<KS2, NW, 4, 1|2>, NW = 1 (40: partly filled, 64), 2 (128), 4 (256) waves of 64 queries."""
    assert census.nw_small(nq) == {40: 1, 64: 1, 128: 2, 256: 4}[nq]
    _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    run_case(vdb, oracle, census.case(kind, n, d), _metric(i), {"force_path": 2, "spans_per_chunk": 2}, nq,
             dict(F16, scan_shape=16, has_i8_copy=0, corpus_fp16_exact=int(kind == "wide")), rot=i)


@pytest.mark.parametrize("i,kind,d,n,st", [(0, "wide", 64, N1, 4), (1, "wide", 64, N1, 8), (2, "gauss", 128, N100, 4),
                                           (3, "gauss", 128, N100, 8)])
def test_x16_fp16_batch(vdb, oracle, i, kind, d, n, st):
    """scan_x16_kernel<KS2, 8, ST, 2>, 512-query tiles, 4- and 8-tile stages; 700 queries: the wave of columns 640.. of the second
    tile holds 60 queries, the waves behind it none."""
    nq = 700
    assert census.nw_small(nq) == 8 and not census.wide_tiles(24, nq)
    _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    run_case(vdb, oracle, census.case(kind, n, d), _metric(i), {"force_path": 2, "spans_per_chunk": 2, "f16_stage_tiles": st}, nq,
             dict(F16, scan_shape=16, has_i8_copy=0), rot=i + 1)


@pytest.mark.parametrize("i,opts,wide", [(0, {"f16_stage_tiles": 8}, True), (1, {"f16_stage_tiles": 4}, True),
                                         (2, {"f16_wide": 1}, False)], ids=["stage8", "stage4", "control-512"])
def test_x16_fp16_wide_tiles(vdb, oracle, i, opts, wide):
    """scan_x16_kernel<2, 8, ST, 2, 256, 8, 8>: 1024-query tiles at D <= 64 (53 one-span chunks x 5 tiles >= 256 workgroups), and
    the same batch on 512-query tiles (`f16_wide` = 1) as the control."""
    nq = 5120
    g = census.scan_geometry(NWIDE, 64, 2, nq, 1)
    assert g.ok and g.chunk_sizes() == {1} and g.nchunks == 53 and census.wide_tiles(g.nchunks, nq) and NWIDE % 512 == 1
    run_case(vdb, oracle, census.case("wide", NWIDE, 64), _metric(i), dict({"force_path": 2, "spans_per_chunk": 1}, **opts), nq,
             dict(F16, scan_shape=16, has_i8_copy=0))


@pytest.mark.parametrize("i,kind,d,n,k,rows", [(0, "wide", 64, N1, 20, 128), (1, "gauss", 128, N100, 40, 64),
                                               (2, "wide", 64, N1, 40, 64), (3, "gauss", 128, N100, 20, 128)])
def test_x16_fp16_direct_bins(vdb, oracle, i, kind, d, n, k, rows):
    """scan_x16_kernel<KS2, 8, 4, 2, 128 | 64, 4> and the direct-bin select: k large enough that the standard geometry declines.  The
    nearest neighbour (twin census: the two nearest) of ALL rows, all k columns of the sample."""
    nq = 700
    g = census.geometry(n, d, k, nq, 2)
    assert not census.scan_geometry(n, d, k, nq, 2).ok and g.ok and g.direct_rows == rows
    c = census.case(kind, n, d)
    stride = census.stride_order(n, 4099)
    metric = _metric(i)
    for which, order, kref in (("plain", np.arange(n), 1), ("twin", stride, 2)):
        idx = _index(vdb, c.rows(which), metric, DIRECT_OPTS)
        D, I = census_run(idx, c.rows(which), nq, k, order, dict(DIRECT, scan_shape=16))
        idx.close()
        check(oracle, c, which, metric, k, D, I, kref)


# ---- layout x16, int8 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("ring", [2, 4, 8])
@pytest.mark.parametrize("nq", [40, 128, 256])
def test_x16_int8_serving(vdb, oracle, nq, ring, nt):
    """scan_i8x16_kernel<KS2, 4, 4, NW, ring, nt>: 1, 2 and 4 waves x `i8_ring` 2, 4, 8 x `i8_nt` 0 (non-temporal loads) and 1."""
    i = (nq // 40) + ring + nt
    d, n = ((64, N100), (128, N1))[i % 2]
    _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    run_case(vdb, oracle, census.case("bytes", n, d), _metric(i // 2),
             {"force_path": 2, "spans_per_chunk": 2, "i8_ring": ring, "i8_nt": nt}, nq, dict(I8, scan_shape=16), rot=i)


def _wide_i8(variant, x16, group=8):
    """The 26 625-row byte-valued corpus with one-span chunks and 5120 queries per call: 53 chunks x 5 tiles of 1024 queries cover the
    chip, so the launch keeps the form `i8_variant` names.  Returns (geometry, form)."""
    nq = 5120
    g = census.scan_geometry(NWIDE, 64, 2, nq, 1)
    assert g.ok and g.nchunks == 53 and g.chunk_sizes() == {1} and census.wide_tiles(g.nchunks, nq) and NWIDE % 512 == 1
    return g, census.i8_batch_form(variant, g.nchunks, nq, x16, group)


@pytest.mark.parametrize("variant", [0, 1])
def test_x16_int8_batch(vdb, oracle, variant):
    """scan_i8x16_kernel<KS2, 4, 4> and <KS2, 8, 4> as their own launch (`scan_pair` = 0): 512-query tiles, 4- and 8-tile stages, 700
    queries, chunks of one and of two spans."""
    nq = 700
    d, n = ((64, N100), (128, N1))[variant % 2]
    g = _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    assert census.i8_batch_form(variant, g.nchunks, nq, True) == (512, (4, 8)[variant], 8, 0)
    run_case(vdb, oracle, census.case("bytes", n, d), _metric(variant),
             {"force_path": 2, "spans_per_chunk": 2, "i8_variant": variant, "scan_pair": 0}, nq, dict(I8, scan_shape=16), rot=variant + 1)


@pytest.mark.parametrize("variant", [2, 3])
def test_x16_int8_batch_1024_query_tiles(vdb, oracle, variant):
    """scan_i8x16_kernel<1, 4, 8> and <1, 8, 8> as their own launch: 1024-query tiles (8 column blocks per wave), 4- and 8-tile
    stages."""
    g, form = _wide_i8(variant, True)
    assert form == (1024, (4, 8)[variant - 2], 8, 0)
    run_case(vdb, oracle, census.case("bytes", NWIDE, 64), _metric(variant),
             {"force_path": 2, "spans_per_chunk": 1, "i8_variant": variant, "scan_pair": 0}, 5120, dict(I8, scan_shape=16), rot=variant)


def frac_queries(c, which):
    """The rows of the corpus + 0.25 on the coordinate that holds the multiset's largest value (never one of the swapped pair): not
    integer, so the fp16 scan serves them.  The ids are those of the rows themselves.  Margin, with j that coordinate and z a row that
    is neither the query's row x nor its twin y (x_j = y_j): L2 |q - z|^2 = |x - z|^2 + 1/16 - (x_j - z_j) / 2 >= d3 - 127.5 against
    |q - y|^2 = 2 + 1/16, so d3 > 130 suffices; IP q.z = x.z + z_j / 4 <= G3 + 63.75 against q.y = x.x - 1 + x_j / 4 >= x.x - 1, so
    G3 < x.x - 65 suffices (values are 0..255); d3 / G3: the third neighbour of the exact reference."""
    rows = c.rows(which)
    assert c.kind == "bytes" and c.ms.max() not in c.pair
    D3 = c.ref(which, "l2", 3)[0][:, 2]
    G3 = c.ref(which, "ip", 3)[0][:, 2]
    assert (D3 > 130).all() and (G3 < c.n2 - 65).all()
    Q = rows.copy()
    Q[np.arange(c.n), np.argmax(rows, axis=1)] += 0.25
    return Q


def run_frac_case(vdb, oracle, c, metric, opts, nq, expect, rot=0):
    """Twin census with fractional queries: ids of all rows from the integer reference (margin: frac_queries), the sample against the
    oracle."""
    which = twin_of(rot)
    Q, T = frac_queries(c, which), c.rows(which)
    idx = _index(vdb, T, metric, opts)
    D, I = census_run(idx, T, nq, 2, census.stride_order(c.n, 4099), expect, queries=Q)
    idx.close()
    Ir, has = c.ref(which, metric, 2)[1], c.partner(which) >= 0       # (a row without a twin: its second neighbour has no margin)
    np.testing.assert_array_equal(I[:, 0], Ir[:, 0])
    np.testing.assert_array_equal(I[has, 1], Ir[has, 1])
    s = census.sample_rows(c.n)
    Do, Io = oracle.knn(T, Q[s], 2, metric)
    np.testing.assert_array_equal(I[s], Io)
    np.testing.assert_array_equal(D[s], Do)


@pytest.mark.parametrize("nq", [40, 128, 256, 700])
@pytest.mark.parametrize("d,n", [(64, N100), (128, N1)])
def test_x16_paired_kernel(vdb, oracle, d, n, nq):
    """scan_pair_x16_kernel at default options (`i8_ks` 2 at D = 64, 4 at D = 128): integer queries run its int8 body, the same rows
    + 0.25 on one coordinate its fp16 body; serving shapes (1, 2, 4 waves) and the batch shape."""
    _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    c = census.case("bytes", n, d)
    metric = _metric(d // 64 + nq // 40)
    opts = {"force_path": 2, "spans_per_chunk": 2}
    assert nq <= 256 or census.i8_batch_form(3, 24, nq, True) == (512, 8, 8, 0)      # (batch shape here: the 512-query form of the pair)
    run_case(vdb, oracle, c, metric, opts, nq, dict(I8, scan_shape=16), rot=nq // 40)
    run_frac_case(vdb, oracle, c, metric, opts, nq, dict(F16, scan_shape=16, has_i8_copy=1), rot=nq // 40)


def test_x16_paired_kernel_1024_query_tiles(vdb, oracle):
    """scan_pair_x16_kernel<false, 8, 8, 8, 8, 2, 0>: the batch form of the paired kernel with 1024-query tiles in its int8 body
    (default `i8_variant` 3 on a grid that covers the chip); fractional queries run its fp16 body on 512-query tiles."""
    g, form = _wide_i8(3, True)
    assert form == (1024, 8, 8, 0)
    c = census.case("bytes", NWIDE, 64)
    opts = {"force_path": 2, "spans_per_chunk": 1}
    run_case(vdb, oracle, c, "l2", opts, 5120, dict(I8, scan_shape=16), rot=1)
    run_frac_case(vdb, oracle, c, "l2", opts, 5120, dict(F16, scan_shape=16, has_i8_copy=1), rot=1)


@pytest.mark.parametrize("i,opts,nq,frac", [
    (0, {}, 700, False), (1, {}, 256, False),
    (2, {"int8_slab_chunks": 1}, 700, True), (3, {}, 700, True), (4, {"int8_slab_chunks": 3}, 128, True),
    (5, {"int8_block_rows": 5000}, 700, False)],
    ids=["int-batch", "int-serving", "frac-slab1", "frac-slab-default", "frac-slab3-serving", "block-rows-5000"])
def test_int8_only(vdb, oracle, i, opts, nq, frac):
    """An `int8_only` index (33 803 rows, above its 32 768-row threshold; `spans_per_chunk` 2: 40 chunks, 27 of two spans): integer queries on the int8
    scan; fractional queries on fp16 slabs made from the int8 panels (convert_slab_from_i8_kernel + scan_in_slabs) with 1, 3 and the
    default 8 chunks per slab, so that slab boundaries fall inside the corpus; `int8_block_rows` 5000 = seven ingestion blocks."""
    d = 64
    g = census.scan_geometry(NI8, d, 2, nq, 2)
    assert g.ok and g.nchunks == 40 and g.chunk_sizes() == {1, 2} and g.rem == 27 and NI8 > 32_768 and NI8 % 512 == 11
    slab = opts.get("int8_slab_chunks", 8)
    assert g.nchunks % slab != 0 or slab == 1 or slab == 8          # (3: the last slab is partial; 8: five whole slabs)
    c = census.case("bytes", NI8, d)
    metric = _metric(i)
    opts = dict({"int8_only": 1, "spans_per_chunk": 2}, **opts)
    if frac:
        run_frac_case(vdb, oracle, c, metric, opts, nq, dict(F16, scan_shape=16, has_i8_copy=2))
    else:
        run_case(vdb, oracle, c, metric, opts, nq, dict(I8, scan_shape=16, has_i8_copy=2))


# ---- flat_shape = 32: the 32x32 kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [8, 4])
@pytest.mark.parametrize("nq", [40, 128, 256, 700])
@pytest.mark.parametrize("kind,d,n", [("wide", 64, N1), ("gauss", 128, N100)])
def test_shape32_fp16(vdb, oracle, kind, d, n, nq, group):
    """scan_kernel<KSTEPS, NW, 4, 1|2, 16, false, octs>: 1, 2, 4 and 8 waves, octs (`f16_group` 8) and quads (4)."""
    _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    i = d // 64 + nq // 40 + group // 4
    run_case(vdb, oracle, census.case(kind, n, d), _metric(i),
             {"force_path": 2, "spans_per_chunk": 2, "flat_shape": 32, "f16_group": group}, nq, dict(F16, scan_shape=32, has_i8_copy=0),
             rot=i)


@pytest.mark.parametrize("i,kind,d,n,k,rows", [(0, "gauss", 64, N100, 20, 128), (1, "wide", 128, N1, 40, 64)])
def test_shape32_fp16_direct_bins(vdb, oracle, i, kind, d, n, k, rows):
    """scan_kernel<KSTEPS, 8, 4, 2, 8 | 4>: direct bins of 128 and of 64 rows."""
    nq = 700
    g = census.geometry(n, d, k, nq, 2)
    assert not census.scan_geometry(n, d, k, nq, 2).ok and g.direct_rows == rows
    c = census.case(kind, n, d)
    metric = _metric(i)
    for which, order, kref in (("plain", np.arange(n), 1), ("twin", census.stride_order(n, 4099), 2)):
        idx = _index(vdb, c.rows(which), metric, dict(DIRECT_OPTS, flat_shape=32))
        D, I = census_run(idx, c.rows(which), nq, k, order, dict(DIRECT, scan_shape=32))
        idx.close()
        check(oracle, c, which, metric, k, D, I, kref)


@pytest.mark.parametrize("group", [8, 4])
@pytest.mark.parametrize("variant", [0, 1])
def test_shape32_int8_batch(vdb, oracle, variant, group):
    """scan_i8_kernel<KS, 4 | 8, 2, 8, 16, false, G>: 512-query tiles, 4- and 8-tile stages, `i8_group` 8 and 4; 700 queries, chunks of
    one and of two spans.  (Every other variant folds onto these two at this size: test_shape32_int8_batch_forms.)"""
    nq = 700
    d, n = ((64, N100), (128, N1))[(variant + group // 4) % 2]
    g = _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    assert census.i8_batch_form(variant, g.nchunks, nq, False, group) == (512, (4, 8)[variant], 8, 0)
    run_case(vdb, oracle, census.case("bytes", n, d), _metric(variant),
             {"force_path": 2, "spans_per_chunk": 2, "flat_shape": 32, "i8_variant": variant, "i8_group": group}, nq,
             dict(I8, scan_shape=32), rot=variant + group)


SHAPE32_FORMS = {0: (512, 4, 8, 0), 1: (512, 8, 8, 0), 2: (1024, 4, 8, 0), 3: (1024, 8, 8, 0), 4: (512, 8, 16, 0), 5: (512, 16, 16, 0),
                 6: (1024, 8, 8, 1), 7: (1024, 8, 8, 2)}


@pytest.mark.parametrize("group", [8, 4])
@pytest.mark.parametrize("variant", range(8))
def test_shape32_int8_batch_forms(vdb, oracle, variant, group):
    """scan_i8_kernel in every batch form `i8_variant` names: 512- and 1024-query tiles with 4- and 8-tile stages (0 - 3), sixteen
    waves with 8- and 16-tile stages (4, 5), a pacing barrier per one and per two tiles (6, 7; with `i8_group` 4 these are variant
    3).  (query tile, tiles per stage, waves, pacing) from the restated rule."""
    g, form = _wide_i8(variant, False, group)
    assert form == (SHAPE32_FORMS[variant] if group == 8 or variant < 6 else SHAPE32_FORMS[3])
    run_case(vdb, oracle, census.case("bytes", NWIDE, 64), _metric(variant + group // 4),
             {"force_path": 2, "spans_per_chunk": 1, "flat_shape": 32, "i8_variant": variant, "i8_group": group}, 5120,
             dict(I8, scan_shape=32), rot=variant)


@pytest.mark.parametrize("ring", [2, 4, 8])
@pytest.mark.parametrize("nq", [40, 128, 256])
def test_shape32_int8_serving(vdb, oracle, nq, ring):
    """scan_i8_kernel<KS, 4, 2, NW, 16, false, G, 0, ring>: the serving rings of the 32x32 int8 scan; `i8_group` alternates."""
    i = nq // 40 + ring
    d, n = ((64, N100), (128, N1))[i % 2]
    _std(n, d, 2, nq, sizes={1, 2}, rem=11, nchunks=24)
    run_case(vdb, oracle, census.case("bytes", n, d), _metric(i // 2),
             {"force_path": 2, "spans_per_chunk": 2, "flat_shape": 32, "i8_ring": ring, "i8_group": (8, 4)[(i // 2) % 2]}, nq,
             dict(I8, scan_shape=32), rot=i)


# ---- D > 128: the K-loop scan ---------------------------------------------------------------------------------------------------
KLOOP = [("wide", 192, K11), ("gauss", 136, K1), ("wide", 384, K11)]


@pytest.mark.parametrize("nq", [16, 40, 700])
@pytest.mark.parametrize("kind,d,n", KLOOP)
def test_kloop(vdb, oracle, kind, d, n, nq):
    """scan16_kloop_kernel<3, 8, 2> (16 queries: the LDS-resident query block), <2, 8, 1> (40) and <2> (700) at D = 136, 192 (three
    64-dim K-steps) and 384."""
    g = census.scan_geometry(n, d, 2, nq, 2)
    assert g.ok and g.nspans == 19 and g.chunk_sizes() == {1, 2} and g.rem == 9 and n % 1024 in (1, 11)
    run_case(vdb, oracle, census.case(kind, n, d), _metric(d // 8 + nq), {"force_path": 2, "spans_per_chunk": 2}, nq,
             dict(F16, scan_shape=0, has_i8_copy=0), rot=(16, 40, 700).index(nq))


@pytest.mark.parametrize("qgroup", [0, 1])
def test_kloop_query_groups(vdb, oracle, qgroup):
    """2600 queries = six 512-query tiles (the last holding 40 queries): at the default four tiles per group the block order has
    two empty slots; `kloop_qgroup` = 1 has none."""
    nq = 2600
    assert census.qpad(nq) // 512 == 6
    g = census.scan_geometry(K11, 192, 2, nq, 2)
    assert g.ok and g.chunk_sizes() == {1, 2}
    run_case(vdb, oracle, census.case("wide", K11, 192), _metric(qgroup), {"force_path": 2, "spans_per_chunk": 2, "kloop_qgroup": qgroup},
             nq, dict(F16, scan_shape=0, has_i8_copy=0))


@pytest.mark.parametrize("i,kind,d,n,k,rows", [(0, "wide", 192, K11, 20, 128), (1, "gauss", 136, K1, 40, 64)])
def test_kloop_direct_bins(vdb, oracle, i, kind, d, n, k, rows):
    """scan16_kloop_kernel<2, 4> and <2, 2>: direct bins of 128 and of 64 rows."""
    nq = 700
    g = census.geometry(n, d, k, nq, 2)
    assert not census.scan_geometry(n, d, k, nq, 2).ok and g.direct_rows == rows
    c = census.case(kind, n, d)
    metric = _metric(i)
    for which, order, kref in (("plain", np.arange(n), 1), ("twin", census.stride_order(n, 4099), 2)):
        idx = _index(vdb, c.rows(which), metric, DIRECT_OPTS)
        D, I = census_run(idx, c.rows(which), nq, k, order, dict(DIRECT, scan_shape=0))
        idx.close()
        check(oracle, c, which, metric, k, D, I, kref)


@pytest.mark.parametrize("nq", [40, 700])
def test_kloop_streamed_panels(vdb, oracle, nq):
    """`stream_panels` = 1 with `stream_slab_rows` 8192: chunks of at most two spans, so four chunks per slab -- ten chunks in three
    slabs, the last one partial (convert_slab16_kernel + scan_in_slabs)."""
    g = census.scan_geometry(K11, 192, 2, nq, 2)
    slab_chunks = max(1, 8192 // ((g.spc + 1) * 1024))
    assert g.ok and g.nchunks == 10 and slab_chunks == 4 and -(-g.nchunks // slab_chunks) == 3 and g.nchunks % slab_chunks != 0
    run_case(vdb, oracle, census.case("wide", K11, 192), _metric(nq // 40),
             {"force_path": 2, "spans_per_chunk": 2, "stream_panels": 1, "stream_slab_rows": 8192}, nq, dict(F16, scan_shape=0, has_i8_copy=0))


# ---- the other paths ----------------------------------------------------------------------------------------------------------
def test_dense_path(vdb, oracle):
    """The dense small-corpus path: 9001 rows (<= 15 360), 64 queries per call (64 x 9001 pairs are too few for the scan)."""
    n, nq = 9001, 64
    assert n <= 15_360 and nq >= 64 and nq * n < 4.0e6
    run_case(vdb, oracle, census.case("wide", n, 64), "l2", {}, nq, dict(last_path_name="mfma_scan", scan_shape=32, last_fallback_queries=0))


@pytest.mark.parametrize("force,nq,blocked", [(1, 1024, True), (3, 1024, False), (1, 40, False)],
                         ids=["blocked", "per-wave", "per-wave-small-batch"])
def test_exhaustive_kernels(vdb, oracle, force, nq, blocked):
    """`force_path` 1: the exhaustive float64 kernels -- query-blocked (groups of four queries, launch_refine_full_blocked) once
    there are 1024 (group, split) units: 1024 queries on 9001 rows give 256 groups x 4 splits; 40 queries do not, and `force_path` 3
    never blocks: one wave per query (launch_refine_full)."""
    assert census.exact_blocked(nq, 9001, 1, force) == blocked
    run_case(vdb, oracle, census.case("wide", 9001, 64), _metric(force), {"force_path": force}, nq, dict(last_path_name="exact_scan"))


def test_split_fallback(vdb, oracle):
    """`list_cap` = 1 at k = 17, the largest k the standard geometry admits here: seventeen superbins lie below the threshold, so the
    work list of every query overflows and every query takes the exhaustive fallback of the tail kernel, split four ways (max_split =
    N / 4096) and merged on the device.  (At k = 1 a census query has ONE candidate, its own row, and nothing overflows.)  Plain
    corpus, natural and stride order: `last_fallback_queries` == nq after every call.  On the twin corpus a bin that holds a row and
    its twin is re-scanned, not listed, and one query in some calls is left with a single listed candidate (measured: 255 of 256 in
    one call of 69), so there the count is only required to reach 95 % of the call.  The three nearest of all rows, all seventeen of
    the sample."""
    nq, k, n = 256, 17, N1
    assert n // 4096 == 4 and census.scan_geometry(n, 64, k, nq, 2).ok and not census.scan_geometry(n, 64, k + 1, nq, 2).ok
    c = census.case("wide", n, 64)
    opts = {"force_path": 2, "spans_per_chunk": 2, "list_cap": 1}
    every = dict(last_path_name="mfma_scan", scan_shape=16, last_fallback_queries=lambda q: q)
    most = dict(every, last_fallback_queries=lambda q: range(q - q // 20, q + 1))
    for which, order, expect in (("plain", np.arange(n), every), ("plain", census.stride_order(n, 4099), every),
                                 ("twin", census.stride_order(n, 4099), most)):
        idx = _index(vdb, c.rows(which), "ip", opts)
        D, I = census_run(idx, c.rows(which), nq, k, order, expect)
        idx.close()
        check(oracle, c, which, "ip", k, D, I)


NSHARD = 46_100                    # three shards of 15 366 / 15 367 rows: each above the 15 360 rows that layout x16 needs


@pytest.mark.parametrize("shards", [2, 3])
def test_shards(vdb, oracle, shards):
    """A two- and a three-shard handle on one GPU, every shard on the remote-shard path (`multi_stage_all`), every shard in layout
    x16 (`scan_shape` is the first shard's; all are built alike).  One corpus of 46 100 rows, the smallest that keeps three shards
    in that layout; its reference is the costliest of the file, so these two cases run the twin census only."""
    assert NSHARD // 3 > 15_360
    run_case(vdb, oracle, census.case("bytes", NSHARD, 64), _metric(shards), {"force_path": 2, "multi_stage_all": 1}, 700,
             dict(last_path_name="mfma_scan", scan_dtype=1, scan_shape=16, last_fallback_queries=0, has_i8_copy=1), rot=shards,
             device=[0] * shards, twin_only=True)

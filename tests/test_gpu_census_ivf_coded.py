"""Census of the coded IVF indexes: every decoded row of an IVF<nlist>,PQ<M> and an IVF<nlist>,SQ8 index is a query.

Both codecs make the fp16 panels of their lists per search from the codes (ivf_pq_panels_kernel, ivf_sq8_panels_kernel) and re-score
candidates exactly through the row accessors of refine.hpp, so a wrong panel -- the centroid of another tile, a k-step slice reading the
wrong sub-space, the last valid row of a span dropped -- changes no returned distance, only which rows become candidates.  As in
tests/test_gpu_census_ivf.py: 20 011 rows in 64 lists, among them an empty list, lists of 1, 255, 256 and 257 rows and one of about 1900,
twins inside the lists at position masks 4, 64 and 256, 8 probes, k = 2; the reference is oracle.ivf_search over the decoded rows x^ for
EVERY row, ids and distances bit for bit.

IVF-PQ   injected centroids, codebooks, codes and lists (tests/census_coded.py: ivfpq_corpus); x^ = ivfpq_restatement.decode.  Shapes
         for every branch of ivf_pq_panels, asserted from its restatement: the table whole in LDS (grid y = 1), in k-step slices (grid
         y = 4), byte staging with D % 16 != 0, and read through the cache (M = 2 at D = 128; that corpus runs under L2 only: with two
         sub-spaces the residual cannot keep one of them at zero, so the norms of c_l + residual differ).
IVF-SQ8  the census corpora ("bytes" at D = 64, "gauss" at D = 128) under centroids close to one another and injected ranges whose
         quantisation step (1, and 5 / 255 < census.GAUSS_GAP) keeps a twin apart from its row; lists and twins as in the IVF-Flat
         census; x^ = the NumPy decode of idx.codes().

Asserted on the CPU, from the reference alone, before any GPU call: the x^ are pairwise distinct, at least 0.8 of the queries have
themselves as first neighbour and at least 0.8 of the paired rows their planted twin as second.  After every call: `last_path_name`
"ivf", `last_candidates` > 0 and `scan_dtype` 2 where the list scan over panels serves, `last_candidates` == 0 where the exact list scan
answers (through ivfpq_key / sq8_key).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import census
from tests import census_coded as cc
from tests.helpers import np_decode, np_encode
from tests.test_gpu_census_ivf import LIST_MASKS, NLIST, NPROBE, K, N, adjust, list_twins

pytestmark = pytest.mark.gpu

F32 = np.float32
assert (N, NLIST, LIST_MASKS) == (cc.IVF_N, cc.IVF_NLIST, cc.LIST_MASKS)


class Built:
    """One coded corpus in one index, the decoded rows (the queries) and the oracle's answer for every row; never modified."""

    def finish(self, oracle, partner):
        """The conditions of the census, from the reference alone; then the index may be built."""
        assert len(np.unique(self.xh, axis=0)) == N
        self.want = oracle.ivf_search(self.xh, self.C, self.lor, self.xh, K, NPROBE, self.metric)
        has = partner >= 0
        assert has.sum() > N // 2
        assert (self.want[1][:, 0] == np.arange(N)).mean() >= 0.8
        assert (self.want[1][has, 1] == partner[has]).mean() >= 0.8
        for a in (self.xh, self.C, self.lor) + tuple(self.want):
            a.setflags(write=False)

    def census(self, nq, lists_serve=True):
        D = np.full((N, K), np.nan, np.float32)
        I = np.full((N, K), -7, np.int64)
        for b0 in range(0, N, nq):
            sel = np.arange(b0, b0 + nq) % N
            d, i = self.idx.search(self.xh[sel], K)
            st = self.idx.stats()
            assert st["last_path_name"] == "ivf", st
            assert (st["last_candidates"] > 0) == lists_serve, (b0, st)
            assert st["scan_dtype"] == (2 if lists_serve else 0), (b0, st)
            D[sel], I[sel] = d, i
        np.testing.assert_array_equal(I, self.want[1])
        np.testing.assert_array_equal(D, self.want[0])


class BuiltPQ(Built):
    def __init__(self, vdb, oracle, d, M, construction, kind, metric):
        self.metric = metric
        self.C, cb, codes, self.lor, partner, self.xh = cc.ivfpq_corpus(d, M, construction, kind)
        self.finish(oracle, partner)
        idx = vdb.IVFPQIndex(d, NLIST, M, metric, 0)
        idx.set_centroids(self.C)
        idx.set_codebooks(cb)
        idx.add_codes(codes, self.lor)
        np.testing.assert_array_equal(idx.assignment(), self.lor)
        np.testing.assert_array_equal(idx.codes(), codes)
        idx.set_nprobe(NPROBE)
        self.idx = idx


def sq8_inputs(kind, d):
    """(rows, pair, centroids, vmin, vdiff).  The centroids lie close to one another and the ranges are injected, so that one code step
    is 1 (bytes: residuals in -127.5 .. 127.5) or 5 / 255 (gauss: residuals in -2.5 .. 2.5), below the 1 / census.GAUSS_GAP that
    separates a twin from its row; values beyond the range clamp (a few per cent of the coordinates)."""
    X = census.corpus(kind, N, d, seed=5)
    _, pair = census.multiset(kind, d, 5)
    if kind == "bytes":
        C = (128 + np.rint((X[:NLIST] - 128) / 16)).astype(F32)
        vmin, vdiff = np.full(d, -127.5, F32), np.full(d, 255, F32)
    else:
        C = (X[:NLIST] / 4).astype(F32)
        vmin, vdiff = np.full(d, -2.5, F32), np.full(d, 5, F32)
        assert vdiff[0] / 255 < census.GAUSS_GAP
    return X, pair, C, vmin, vdiff


class BuiltSQ8(Built):
    def __init__(self, vdb, oracle, kind, d, metric):
        self.metric = metric
        X, pair, self.C, vmin, vdiff = sq8_inputs(kind, d)
        self.lor = adjust(oracle.ivf_assign(self.C, X, metric))
        T = list_twins(X, self.lor, pair)
        codes = np_encode(T, self.C, self.lor, vmin, vdiff)
        self.xh = np.ascontiguousarray(np_decode(codes, self.C, self.lor, vmin, vdiff), F32)
        self.finish(oracle, cc.list_partner(self.lor, LIST_MASKS, NLIST))
        idx = vdb.IVFSQ8Index(d, NLIST, metric, 0)
        idx.set_centroids(self.C)
        idx.set_ranges(vmin, vdiff)
        idx.add(T, list_of_row=self.lor)
        np.testing.assert_array_equal(idx.assignment(), self.lor)
        got = idx.codes()
        np.testing.assert_array_equal(got, codes)
        np.testing.assert_array_equal(np_decode(got, self.C, self.lor, vmin, vdiff).astype(F32), self.xh)
        idx.set_nprobe(NPROBE)
        self.idx = idx


@pytest.fixture(scope="module")
def built(vdb, oracle):
    cache = {}

    def get(codec, *key):
        if (codec,) + key not in cache:
            cache[(codec,) + key] = (BuiltPQ if codec == "pq" else BuiltSQ8)(vdb, oracle, *key)
        return cache[(codec,) + key]

    yield get
    for b in cache.values():
        b.idx.close()


PQ = [("pq", d, M, construction, kind, metric) for d, M, construction, kind, metrics in cc.IVFPQ_SHAPES for metric in metrics]
SQ8 = [("sq8", "bytes", 64, "ip"), ("sq8", "gauss", 128, "l2")]
# the branch of ivf_pq_panels every IVF-PQ shape names: (table in LDS, grid y, dword staging, D % 16 != 0)
BRANCH = {(48, 12): (True, 1, True, False), (128, 64): (True, 4, True, False), (100, 25): (True, 4, False, True),
          (128, 2): (False, 1, False, False)}


def _get(built, key):
    if key[0] == "pq":
        L = cc.ivfpq_panel_launch(key[1], key[2])
        assert (L["lds"], L["gy"], L["vec"], L["pad16"]) == BRANCH[key[1:3]], L
    return built(*key)


def _options(idx, **opts):
    for name, value in opts.items():
        idx.set_option(name, value)


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("nq", [40, 700])
@pytest.mark.parametrize("key", PQ + SQ8 + [("sq8", "bytes", 128, "l2"), ("sq8", "gauss", 64, "ip")], ids=_ids)
def test_list_scan_default_options(built, key, nq):
    """Default launch shapes, batches of 40 and of 700 queries."""
    b = _get(built, key)
    _options(b.idx, ivf_nw=0, ivf_bt=0, ivf_part=0, ivf_min_batch=1)
    b.census(nq)


@pytest.mark.parametrize("bt", [4, 16])
@pytest.mark.parametrize("nw", [2, 4, 8])
@pytest.mark.parametrize("key", PQ[1::2] + SQ8, ids=_ids)
def test_list_scan_waves_and_bins(built, key, nw, bt):
    """`ivf_nw` 2 / 4 / 8 waves x `ivf_bt` 4 / 16 tiles per bin over the panels made from the codes."""
    b = _get(built, key)
    _options(b.idx, ivf_nw=nw, ivf_bt=bt, ivf_part=0, ivf_min_batch=1)
    b.census(700)
    _options(b.idx, ivf_nw=0, ivf_bt=0)


@pytest.mark.parametrize("part,bt", [(4, 0), (1, 4), (4, 4)])
@pytest.mark.parametrize("key", PQ[0::2] + SQ8, ids=_ids)
def test_list_scan_parts(built, key, part, bt):
    """`ivf_part`: the long list (1900 rows, 8 spans) is cut into row parts in every case."""
    b = _get(built, key)
    assert np.bincount(b.lor)[1] > 4 * 256
    _options(b.idx, ivf_nw=0, ivf_bt=bt, ivf_part=part, ivf_min_batch=1)
    b.census(700)
    _options(b.idx, ivf_part=0, ivf_bt=0)


@pytest.mark.parametrize("key", PQ + SQ8, ids=_ids)
def test_exact_list_scan(built, key):
    """`ivf_min_batch` above the batch: the exact list scan answers through ivfpq_key / sq8_key (no candidates)."""
    b = _get(built, key)
    _options(b.idx, ivf_nw=0, ivf_bt=0, ivf_part=0, ivf_min_batch=100_000)
    b.census(700, lists_serve=False)
    _options(b.idx, ivf_min_batch=1)

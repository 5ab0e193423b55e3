"""Census of the IVF-Flat list scans: every row of a corpus is a query, through every row of the list scans' launch tables.

The corpora are those of tests/census.py (every row its own strict nearest neighbour), 20 011 rows in 64 lists under injected centroids
(the first 64 rows).  The assignment of a first add is then adjusted (vdb_ivf_add_assigned) so that the lists include an empty list, a
one-row list, lists of 255, 256 and 257 rows (one 256-row bin, exactly full, one row over) and one list of about 1900 rows that
`ivf_part` cuts; and inside every list the row at position j ^ mask becomes the twin of the row at position j (masks 4, 64 and 256,
dealt over the lists: other quad, other tile, the next 256-row span of the list), so that the second neighbour of a query sits at a
chosen position of the SAME list.  A query finds its own list among its 8 probes unless the adjustment moved it: either way the
reference, `oracle.ivf_search` over the same centroids and assignment, for EVERY query, says what must come back -- ids and distances
of all rows, bit for bit.  `last_path_name == "ivf"` after every call, and `last_candidates > 0` (the list-major MFMA scan served)
wherever that scan is meant to serve.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import census

pytestmark = pytest.mark.gpu

N, NLIST, NPROBE, K = 20_011, 64, 8, 2
LIST_MASKS = (4, 64, 256)


def adjust(lor):
    """The assignment with the list sizes the census wants: list 0 empty, list 2 one row, lists 4 / 5 / 6 of 255 / 256 / 257 rows, list
    1 long (it takes what the others give up and the whole of lists 8 .. 11)."""
    lor = lor.copy()
    keep = {0: 0, 2: 1, 4: 255, 5: 256, 6: 257}
    for l, size in keep.items():
        members = np.flatnonzero(lor == l)
        assert len(members) >= size, (l, len(members))
        lor[members[size:]] = 1
    for l in (8, 9, 10, 11):
        lor[lor == l] = 1
    sizes = np.bincount(lor, minlength=NLIST)
    assert [sizes[l] for l in keep] == list(keep.values()) and sizes[1] > 1500 and (sizes[8:12] == 0).all()
    return lor


def list_twins(X, lor, pair):
    """Inside every list, the row at position j ^ mask (list order = id order) becomes the twin of the row at position j."""
    T = X.copy()
    paired = 0
    for l in range(NLIST):
        members = np.flatnonzero(lor == l)
        j = np.arange(len(members))
        p = j ^ LIST_MASKS[l % 3]
        lo = j[(p > j) & (p < len(members))]
        if len(lo):
            T[members[p[lo]]] = census._swap_pair(X, members[lo], pair)
            paired += 2 * len(lo)
    assert len(np.unique(T, axis=0)) == len(T) and paired > len(T) // 2
    return T


def frac(T):
    """The rows + 0.25 on the coordinate holding the largest value: not integer, so the fp16 list scan serves a byte-valued index."""
    Q = T.copy()
    Q[np.arange(len(T)), np.argmax(T, axis=1)] += 0.25
    return Q


class Built:
    """One corpus in one index, its queries and the oracle's answer for every row; shared by the cases, never modified."""

    def __init__(self, vdb, oracle, kind, d, metric, opts=()):
        X = census.corpus(kind, N, d, seed=5)
        _, pair = census.multiset(kind, d, 5)
        self.C = X[:NLIST].copy()
        self.metric = metric
        idx = vdb.IVFFlatIndex(d, NLIST, metric, 0)
        for name, value in opts:
            idx.set_option(name, value)
        idx.set_centroids(self.C)
        idx.add(X)
        self.lor = adjust(idx.assignment())
        self.T = list_twins(X, self.lor, pair)
        idx.reset()
        idx.add(self.T, list_of_row=self.lor)
        np.testing.assert_array_equal(idx.assignment(), self.lor)
        idx.set_nprobe(NPROBE)
        self.idx = idx
        self.queries = {"rows": self.T}
        if kind == "bytes":
            assert idx.stats()["has_i8_copy"] == 1
            self.queries["frac"] = frac(self.T)
        else:
            assert idx.stats()["has_i8_copy"] == 0
        self.want = {name: oracle.ivf_search(self.T, self.C, self.lor, q, K, NPROBE, metric) for name, q in self.queries.items()}
        # the census is about a row that finds itself: all but the rows the adjustment moved out of their probes do
        found = self.want["rows"][1][:, 0] == np.arange(N)
        assert found.mean() > 0.8
        for a in (self.T, self.lor, self.C) + tuple(self.queries.values()) + tuple(x for w in self.want.values() for x in w):
            a.setflags(write=False)

    def census(self, nq, lists_serve=True, which=None):
        for name, Q in self.queries.items():
            if which and name != which:
                continue
            D = np.full((N, K), np.nan, np.float32)
            I = np.full((N, K), -7, np.int64)
            for b0 in range(0, N, nq):
                sel = np.arange(b0, b0 + nq) % N
                d, i = self.idx.search(Q[sel], K)
                st = self.idx.stats()
                assert st["last_path_name"] == "ivf", st
                assert (st["last_candidates"] > 0) == lists_serve, (name, b0, st)
                if lists_serve:     # (the int8 list scan serves integer queries on byte-valued rows only)
                    assert st["scan_dtype"] == (1 if name == "rows" and "frac" in self.queries else 0), (name, b0, st)
                D[sel], I[sel] = d, i
            np.testing.assert_array_equal(I, self.want[name][1], err_msg=name)
            np.testing.assert_array_equal(D, self.want[name][0], err_msg=name)


@pytest.fixture(scope="module")
def built(vdb, oracle):
    cache = {}

    def get(kind, d, metric, opts=()):
        key = (kind, d, metric, tuple(opts))
        if key not in cache:
            cache[key] = Built(vdb, oracle, kind, d, metric, opts)
        return cache[key]

    yield get
    for b in cache.values():
        b.idx.close()


SHAPES = [("gauss", 64, "l2"), ("wide", 128, "ip"), ("bytes", 64, "ip"), ("bytes", 128, "l2")]


def _options(idx, **opts):
    for name, value in opts.items():
        idx.set_option(name, value)


@pytest.mark.parametrize("nq", [40, 700])
@pytest.mark.parametrize("kind,d,metric", SHAPES)
def test_list_scan_default_options(built, kind, d, metric, nq):
    """Default launch shapes, batches of 40 and of 700 queries; byte-valued rows: integer queries on the int8 list scan, fractional
    ones on the fp16 list scan."""
    b = built(kind, d, metric)
    _options(b.idx, ivf_nw=0, ivf_bt=0, i8_ring=0, ivf_i8_group=4, ivf_part=0, ivf_min_batch=1)
    b.census(nq)


@pytest.mark.parametrize("bt", [4, 16])
@pytest.mark.parametrize("nw", [2, 4, 8])
@pytest.mark.parametrize("kind,d,metric", SHAPES)
def test_list_scan_waves_and_bins(built, kind, d, metric, nw, bt):
    """`ivf_nw` 2 / 4 / 8 waves x `ivf_bt` 4 / 16 tiles per bin (64- / 128-row bins): the fp16 list scan, and on byte-valued rows the
    int8 one.  k = 2 wants 8 bins per query; 8 probes give them at either bin size."""
    b = built(kind, d, metric)
    _options(b.idx, ivf_nw=nw, ivf_bt=bt, i8_ring=0, ivf_i8_group=4, ivf_part=0, ivf_min_batch=1)
    b.census(700)
    _options(b.idx, ivf_nw=0, ivf_bt=0)


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("ring", [2, 4, 8])
@pytest.mark.parametrize("d,metric", [(64, "ip"), (128, "l2")])
def test_int8_list_scan_rings_and_groups(built, d, metric, ring, group):
    """The int8 list scan: `i8_ring` 2 / 4 / 8 x `ivf_i8_group` 4 / 8 (integer queries only)."""
    b = built("bytes", d, metric)
    _options(b.idx, ivf_nw=0, ivf_bt=0, i8_ring=ring, ivf_i8_group=group, ivf_part=0, ivf_min_batch=1)
    b.census(700, which="rows")
    _options(b.idx, i8_ring=0, ivf_i8_group=4)


@pytest.mark.parametrize("part,bt", [(4, 0), (1, 4), (4, 4)])
@pytest.mark.parametrize("kind,d,metric", SHAPES)
def test_list_scan_parts(built, kind, d, metric, part, bt):
    """`ivf_part`: row parts of the 256-row spans of a list, rounded up by ivf_part_spans to the unit the bins of a lane's run allow
    (4 / bins per span half).  At the default bin size that unit is 4 spans, so `ivf_part` 1 would be the same launch as 4 and is
    not a case; with `ivf_bt` 4 the unit is smaller and 1 and 4 differ.  The long list (about 1900 rows, 8 spans) is cut in every
    case; D = 200, where the unit is one span: test_kloop_list_scan_parts."""
    b = built(kind, d, metric)
    assert np.bincount(b.lor)[1] > 4 * 256
    _options(b.idx, ivf_nw=0, ivf_bt=bt, i8_ring=0, ivf_i8_group=4, ivf_part=part, ivf_min_batch=1)
    b.census(700)
    _options(b.idx, ivf_part=0, ivf_bt=0)


@pytest.mark.parametrize("part", [1, 4])
def test_kloop_list_scan_parts(built, part):
    """D = 200, `ivf_tps` 16: `ivf_part` 1 and 4 spans with a unit of one span -- the finest cut of the long list, and of the 257-row
    list."""
    b = built("gauss", 200, "l2", (("ivf_tps", 16),))
    _options(b.idx, ivf_tile=0, ivf_group=0, ivf_part=part, ivf_min_batch=1)
    b.census(700)
    _options(b.idx, ivf_part=0)


@pytest.mark.parametrize("kind,d,metric", SHAPES)
def test_exact_list_scan(built, kind, d, metric):
    """`ivf_min_batch` above the batch: the exact list scan answers (no candidates)."""
    b = built(kind, d, metric)
    _options(b.idx, ivf_nw=0, ivf_bt=0, i8_ring=0, ivf_i8_group=4, ivf_part=0, ivf_min_batch=100_000)
    b.census(700, lists_serve=False)
    _options(b.idx, ivf_min_batch=1)


@pytest.mark.parametrize("group", [1, 2, 4])
@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("tps", [16, 64])
def test_kloop_list_scan(built, tps, tile, group):
    """D = 200 (the K-loop list scan): `ivf_tps` 16 / 64 tiles per panel span (set before the add) x `ivf_tile` 1 / 2 x `ivf_group`
    1 / 2 / 4."""
    b = built("gauss" if tps == 16 else "wide", 200, "l2" if tps == 16 else "ip", (("ivf_tps", tps),))
    _options(b.idx, ivf_tile=tile, ivf_group=group, ivf_part=0, ivf_min_batch=1)
    b.census(700)
    b.census(40) if (tile, group) == (1, 1) else None
    _options(b.idx, ivf_tile=0, ivf_group=0)

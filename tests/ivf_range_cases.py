"""Shapes, radii and the reference of the range search on IVF-Flat indexes (vdb_ivf_range_search), shared by
tests/test_ivf_range_host.py and tests/test_gpu_ivf_range.py.

Reference: the oracle's IVF search with K = the rows of the nprobe longest lists -- ivf_search(X, C, lor, Q, K, nprobe, metric) returns
every row of a query's probed lists -- cut to the entries with I >= 0 whose float32 D passes the radius, put in (list, id) order.
The coarse choice, the canonical keys and the returned D are vdb_ivf_search's, so this is the contract restated.

Shapes are tests/ivf_filter_cases.SHAPES: the smallest at which each launch family of the list scans still runs.  The near-tie cases
carry tests/range_cases.py's construction (clusters of near-copies that the radius cuts through) over to an index of four lists, and
`emulated_miss` restates (scan score, packed minimum, threshold, marks) so that the host can show what eps = 0 would lose.  NumPy only."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import guard_cases as gc
from tests import ivf_filter_cases as ic
from tests import range_cases as rc

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
SHAPES = ic.SHAPES
ID_BASES = ic.ID_BASES


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def probed_rows_bound(lor, nlist: int, nprobe: int) -> int:
    """rows of the nprobe longest lists: no query probes more"""
    return int(np.sort(np.bincount(lor, minlength=nlist))[::-1][:nprobe].sum())


def full_lists(ivf_search, X, C, lor, Q, nprobe: int, metric: str):
    """(D, I) of the oracle with K = probed_rows_bound: every probed row of every query, nearest first, padded with I = -1"""
    K = max(1, probed_rows_bound(lor, len(C), nprobe))
    d, i = ivf_search(X, C, lor, Q, K, nprobe, metric)
    d, i = np.ascontiguousarray(d, F32), np.ascontiguousarray(i, np.int64)
    d.flags.writeable = False
    i.flags.writeable = False
    return d, i


def cut(full, lor, radius, metric: str, id_base: int = 0):
    """(lims, D, I) of the contract from full_lists' (D, I): entries with I >= 0 whose float32 D passes, in (list, id) order"""
    d, i = full
    r = F32(radius)
    with np.errstate(invalid="ignore"):
        keep = (i >= 0) & ((d < r) if metric == "l2" else (d > r))
    n = len(lor)
    key = np.where(keep, lor[np.maximum(i, 0)].astype(np.int64) * n + i, np.int64(n) * (int(lor.max()) + 2))
    order = np.argsort(key, axis=1, kind="stable")
    cnt = keep.sum(axis=1)
    lims = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    lead = np.arange(d.shape[1])[None, :] < cnt[:, None]
    return lims, np.take_along_axis(d, order, axis=1)[lead], (np.take_along_axis(i, order, axis=1)[lead] + id_base).astype(np.int64)


def radii(full, metric: str):
    """name -> radius: the medians over the queries of the 10th and 100th D, the special values, and a returned D itself"""
    d, _ = full
    last = d.shape[1] - 1                      # (tiny host shapes probe fewer than 100 rows)
    return {"median10": float(np.median(d[:, min(9, last)])), "median100": float(np.median(d[:, min(99, last)])), "zero": 0.0,
            "-inf": float("-inf"), "+inf": float("inf"), "flt_max": FLT_MAX, "a-returned-D": float(d[0, min(5, last)])}


MEDIANS = ("median10", "median100")


def brute_reference(pair_keys, X, C, lor, Q, nprobe: int, metric: str, radius, id_base: int = 0):
    """The definition stated directly: per query the nprobe nearest lists (float64, ties to the lower list), the oracle's pair_keys
    over the rows of those lists in (list, id) order, the float32 comparison."""
    perm, offsets = ic.list_order(lor)
    lims, D, I = [0], [], []
    r = F32(radius)
    for q in range(len(Q)):
        lists = np.sort(ic.nearest_lists(C, Q[q], metric, nprobe))
        rows = np.concatenate([perm[offsets[l]:offsets[l + 1]] for l in lists]).astype(np.int64)
        keys = pair_keys(X, Q[q:q + 1], rows[None, :], metric)[0]
        with np.errstate(over="ignore", invalid="ignore"):
            d = (keys if metric == "l2" else -keys).astype(F32)
            hit = d < r if metric == "l2" else d > r
        D.append(d[hit])
        I.append(rows[hit] + id_base)
        lims.append(lims[-1] + int(hit.sum()))
    return np.asarray(lims, np.int64), np.concatenate(D).astype(F32), np.concatenate(I).astype(np.int64)


# ---- near ties: the radius cuts through clusters of near-copies inside the lists ------------------------------------------------------
NEAR_TIE_CASES = rc.CASES
NEAR_TIE_NPROBE = 2


@lru_cache(maxsize=None)
def near_tie(c):
    """(X, C, Q, radius): range_cases.make(c) under the four centroids of guard_cases.ivf_centroids"""
    X, Q, radius = rc.make(c)
    C = gc.ivf_centroids(c.d)
    C.flags.writeable = False
    return X, C, Q, radius


def scan_layout(n: int, d: int, nlist: int, nprobe: int, k: int = 1):
    """(bin_rows, group_rows, nm) of the list scan ivf_geometry (csrc/ivf_plan.hpp) picks at default options"""
    if d > 128:
        tps = 64 if n / nlist > 2048.0 else 16
        return tps * 4, (4 if tps == 64 else 1), 5
    avg_pspans = n / nlist / 256.0            # (a lower bound of pspans / nlist: enough for the comparison below at these sizes)
    bt = 8 if nprobe * 256.0 / 128.0 * avg_pspans >= 8.0 * k else 4
    return bt * 16, 4, 3


def packed(scores: np.ndarray, quad: np.ndarray) -> np.ndarray:
    """pack_score (csrc/scan.hpp): the low six mantissa bits of a score replaced by its quad number.  Monotone in the score for a given
    quad, so "some row of the quad passes" is "the packed quad minimum passes"."""
    b = np.ascontiguousarray(scores, F32).view(np.uint32)
    return ((b & np.uint32(0xFFFFFFC0)) | quad.astype(np.uint32)[None, :]).view(F32)


def emulated_marks(X, lor, Q, radius, metric: str, eps, bin_rows: int, group_rows: int, nm: int):
    """(nq, n) bool in INSERTION order: the rows the mark kernel would mark from emulated scan scores -- a quad (group_rows
    consecutive list rows) whose packed minimum passes, or the whole bin when nm or more of its quads pass"""
    perm, offsets = ic.list_order(lor)
    s = gc.emulated_scores(X, Q, metric)[:, perm]                   # list order
    thr = rc.emulated_threshold(X, Q, radius, metric, eps)[:, None]
    pos = np.arange(len(lor)) - offsets[lor[perm]]
    passes = packed(s, (pos % bin_rows) // group_rows) <= thr
    quad_start = np.flatnonzero(pos % group_rows == 0)
    bin_start_q = np.flatnonzero(pos[quad_start] % bin_rows == 0)  # index into the quads
    quad_pass = np.add.reduceat(passes, quad_start, axis=1) > 0
    whole = np.add.reduceat(quad_pass.astype(np.int32), bin_start_q, axis=1) >= nm
    quad_of_row = np.cumsum(pos % group_rows == 0) - 1
    bin_of_quad = np.cumsum(pos[quad_start] % bin_rows == 0) - 1
    marked = quad_pass[:, quad_of_row] | whole[:, bin_of_quad[quad_of_row]]
    out = np.zeros_like(marked)
    out[:, perm] = marked
    return out


def emulated_miss(X, C, lor, Q, radius, metric: str, keys, eps, nprobe: int = NEAR_TIE_NPROBE):
    """(share of the queries with a true result among their probed rows that the emulated marks leave out, mean true results)
    keys: canonical float64 keys (nq, n)"""
    n, d = X.shape
    bin_rows, group_rows, nm = scan_layout(n, d, len(C), nprobe)
    probed = gc.probed_mask(C, lor, Q, metric, nprobe)
    dist = (keys if metric == "l2" else -keys).astype(F32)
    truth = ((dist < F32(radius)) if metric == "l2" else (dist > F32(radius))) & probed
    marked = emulated_marks(X, lor, Q, radius, metric, eps, bin_rows, group_rows, nm)
    return float((truth & ~marked).any(axis=1).mean()), float(truth.sum(axis=1).mean())


# ---- the packing allowance on its own: exact integer scores of magnitude 2^18 and more ---------------------------------------------------
# A byte-valued corpus and an integer batch: sx = sq = 1, the fp16 products and the float32 sums are exact, and query_eps_body leaves
# eps = 1.02 pack_err and nothing else (int_exact).  The scan scores ||x||^2 - 2 q.x are integers near -||q||^2, about -1.4e6 (D = 64)
# and -2.8e6 (D = 128): a float32 there has 3 / 2 fractional bits, so the six bits a kept minimum gives up for its quad number are worth
# up to 7.9 / 15.75 -- and for a negative score a LOW quad number moves the packed value UP.  Every query is a base row moved by +-1 in
# PACK_SHIFT coordinates; replica j of the base row differs from it by +-1 in j other coordinates, so the query sees its cluster at the
# squared distances PACK_SHIFT + 0 .. 10, and the radius PACK_SHIFT + 5.5 cuts between two adjacent integers: six true results at
# 0.5, 1.5, .. 5.5 below it.  Sixteen lists keep the replicas of a row (nb ids apart) in different 128-row bins.
PACK_SHIFT, PACK_NLIST, PACK_NPROBE = 12, 16, 4


@dataclass(frozen=True)
class PackCase:
    nb: int
    d: int
    nq: int
    metric: str = "l2"

    @property
    def id(self):
        return f"pack-nb{self.nb}-d{self.d}-nq{self.nq}-{self.metric}"


PACK_CASES = (PackCase(1800, 128, 256), PackCase(1800, 64, 256))


@lru_cache(maxsize=None)
def pack_case(c: PackCase):
    """(X (11 nb, d), C, Q (nq, d), radius): integers in 2 .. 253 moved by +-1, read-only"""
    rng = np.random.default_rng([67, c.nb, c.d, c.nq])
    B = rng.integers(2, 254, size=(c.nb, c.d)).astype(np.int64)
    reps = np.repeat(B[None], rc.REPLICAS, axis=0)
    cols = np.argsort(rng.random((c.nb, c.d)), axis=1)          # per base row: a random order of the coordinates
    sign = rng.choice([-1, 1], size=(c.nb, c.d))
    base = np.arange(c.nb)
    for j in range(1, rc.REPLICAS):                             # replica j: +-1 in the coordinates cols[:, PACK_SHIFT .. PACK_SHIFT + j)
        for t in range(j):
            col = cols[:, PACK_SHIFT + t]
            reps[j, base, col] += sign[base, col]
    X = reps.reshape(rc.REPLICAS * c.nb, c.d).astype(F32)
    pick = rng.choice(c.nb, c.nq, replace=False)
    Q = B[pick].copy()
    for t in range(PACK_SHIFT):                                 # the query: +-1 in the first PACK_SHIFT coordinates of that order
        col = cols[pick, t]
        Q[np.arange(c.nq), col] += sign[pick, col]
    Q = Q.astype(F32)
    C = X[:PACK_NLIST].copy()
    for a in (X, C, Q):
        a.flags.writeable = False
    return X, C, Q, F32(PACK_SHIFT + 5.5)


def pack_only_eps(X, Q, metric):
    """(nq,) 1.02 pack_err of query_eps_body in scan units, for a batch whose other terms are zero (cs = 1)"""
    n2 = (X.astype(np.float64) ** 2).sum(axis=1).astype(F32).max()
    Xn = float(F32(np.sqrt(n2, dtype=F32) * F32(1.0000002)))
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(axis=1))
    mag = Xn * Xn + 2.0 * qn * Xn if metric == "l2" else qn * Xn
    return 1.02 * 2.0 ** -17 * mag


# ---- more bins than the mark kernel lists: its own fallback --------------------------------------------------------------------------------
# 32 long lists of 66 spans and 32 short ones: the average query meets 32 * 2 * 33.5 = 2144 entries, which ivf_geometry admits
# (<= 0.7 * 4096), but a query whose 32 probed lists are the long ones meets 32 * 2 * 68 = 4352 > max_entries = 4096 (two runs of 66
# bins, each padded to 68: ivf_bins_of_list) and must take the kernel's fill, counted there and not by range_thr_kernel.
OVERFLOW_NLIST, OVERFLOW_NPROBE, OVERFLOW_LONG, OVERFLOW_SHORT, OVERFLOW_MAX_ENTRIES = 64, 32, 16700, 100, 4096


def overflow_entries(length: int) -> int:
    """entries a probed list of `length` rows gives a query on the 32-row-tile scans with 128-row bins (ivf_bins_of_list, run_groups 2)"""
    spans = -(-length // 256)
    return 2 * ((spans + 3) & ~3)


@lru_cache(maxsize=None)
def overflow():
    """(X, C, lor, Q, flagged): d = 16; the first 8 queries sit among the centroids of the long lists, the other 8 among the short ones'"""
    rng = np.random.default_rng(71)
    d, half = 16, OVERFLOW_NLIST // 2
    centre = np.zeros((2, d))
    centre[1, 0] = 40.0
    C = (np.repeat(centre, half, axis=0) + rng.standard_normal((OVERFLOW_NLIST, d))).astype(F32)
    lor = np.repeat(np.arange(OVERFLOW_NLIST), [OVERFLOW_LONG] * half + [OVERFLOW_SHORT] * half).astype(np.int32)
    lor = lor[rng.permutation(len(lor))]
    X = (C[lor] + rng.standard_normal((len(lor), d))).astype(F32)
    Q = (np.repeat(centre, 8, axis=0) + rng.standard_normal((16, d))).astype(F32)
    lengths = np.bincount(lor, minlength=OVERFLOW_NLIST)
    flagged = np.array([sum(overflow_entries(int(lengths[l])) for l in ic.nearest_lists(C, q, "l2", OVERFLOW_NPROBE)) > OVERFLOW_MAX_ENTRIES
                        for q in Q])
    for a in (X, C, lor, Q, flagged):
        a.flags.writeable = False
    return X, C, lor, Q, flagged


# ---- census: one small index with lists of every awkward length ------------------------------------------------------------------------
CENSUS_LENGTHS = (0, 1, 31, 32, 33, 256, 300, 47)          # (256: a list that ends exactly at a span boundary)


@lru_cache(maxsize=None)
def census(d: int):
    """(X, C, lor): sum(CENSUS_LENGTHS) Gaussian rows filed by hand, interleaved so that list order is not insertion order"""
    rng = np.random.default_rng([61, d])
    lor = rng.permutation(np.repeat(np.arange(len(CENSUS_LENGTHS)), CENSUS_LENGTHS)).astype(np.int32)
    X = rng.standard_normal((len(lor), d)).astype(F32)
    C = rng.standard_normal((len(CENSUS_LENGTHS), d)).astype(F32)
    for a in (X, C, lor):
        a.flags.writeable = False
    return X, C, lor

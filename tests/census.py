"""Census corpora: every row is provably the nearest neighbour of exactly one query (itself) and a chosen partner is its second.

A random corpus only verifies the rows that land in some query's top-k; a census queries with EVERY row, so a scan that loses the rows of
one tile, stage, span or chunk position fails for exactly those rows.  This module holds no GPU code: the corpora, an exact reference
over the Gram matrix, and a restatement of the scan geometry of csrc/scan_plan.hpp with which a test asserts the launch shape it names.

Corpora.  Every row is a random permutation of one fixed multiset of D values, so all rows have the same norm and row r is its own
strict nearest neighbour under L2 (distance 0) and under IP (Cauchy-Schwarz: x.y < |x||y| = x.x for y != x of equal norm).  Kinds:
  bytes  multiset from 0..255: the index keeps an int8 copy, integer queries take the int8 scans
  wide   integers in -200..200 with a value below -128 and one above 127: no int8 copy, exact in fp16 (the fp16 scans with eps = 0)
  gauss  float32 Gaussian values pushed at least `GAUSS_GAP` apart: the fp16 scans with eps > 0 and real scales

Twins.  `twins(X, mask)` makes row r ^ mask a copy of row r with two coordinates swapped whose values differ by 1 (integer kinds) or by
the smallest gap of the multiset (gauss).  Two rows of one multiset differ in at least two coordinates, each by at least the smallest
gap g, so |x - y|^2 >= 2 g^2 with equality only for such a swap: the twin is the second neighbour under both metrics (L2 2 g^2,
IP x.x - g^2), strictly unless another row happens to be the same swap, which the exact reference would show as a tie.
`twins_mixed` deals the seven masks over the 2048-row blocks of one corpus (every mask is below 2048, so pairs stay inside a block);
`rot` rotates the deal, so that over the cases of a family every mask meets other spans and chunks (Case: "twin", "twin1", "twin2").
"""
from __future__ import annotations

import numpy as np

KINDS = ("bytes", "wide", "gauss")
MASKS = (4, 8, 64, 128, 256, 512, 1024)     # other quad | neighbouring group | other tile / 128-row block of a bin (2) | other bin | next span (2)
GAUSS_GAP = 0.02
MIXED_BLOCK = 2048


# ---- corpora ------------------------------------------------------------------------------------------------------------------
def multiset(kind, d, seed):
    """The D values every row of the corpus permutes (float32), and the pair (a, b = a + gap) a twin swaps."""
    rng = np.random.default_rng([seed, d, KINDS.index(kind)])
    if kind == "bytes":
        ms = rng.integers(0, 256, size=d).astype(np.float32)
        ms[0], ms[1] = 100.0, 101.0
        ms[2:][np.isin(ms[2:], (100.0, 101.0))] += 2.0
    elif kind == "wide":
        ms = rng.integers(-200, 201, size=d).astype(np.float32)
        ms[0], ms[1], ms[2], ms[3] = -37.0, -36.0, -150.0, 190.0
        ms[4:][np.isin(ms[4:], (-37.0, -36.0))] += 2.0
    elif kind == "gauss":
        ms = np.sort(rng.standard_normal(d)).astype(np.float32)
        for i in range(1, d):       # at least GAUSS_GAP apart: the reference's ids are certain (gram_topk asserts the margin)
            ms[i] = max(ms[i], np.float32(ms[i - 1] + np.float32(GAUSS_GAP * (1.25 + 0.5 * rng.random()))))
        ms[d // 2] = np.float32(ms[d // 2 - 1] + np.float32(GAUSS_GAP))      # the one smallest gap
        for i in range(d // 2 + 1, d):
            ms[i] = max(ms[i], np.float32(ms[i - 1] + np.float32(GAUSS_GAP * 1.25)))
    else:
        raise AssertionError(kind)
    if kind == "gauss":
        a, b = ms[d // 2 - 1], ms[d // 2]
        gaps = np.diff(np.sort(ms))
        assert gaps.min() > 0 and np.argmin(gaps) == d // 2 - 1 and (np.delete(gaps, d // 2 - 1) > gaps.min()).all()
    else:
        a, b = ms[0], ms[1]
        assert b - a == 1.0
        if kind == "wide":
            assert ms.min() < -128 and ms.max() > 127 and np.abs(ms).max() <= 200
    assert (ms == a).sum() == 1 and (ms == b).sum() == 1     # the swapped pair is unambiguous in every row
    return ms, (np.float32(a), np.float32(b))


def corpus(kind, n, d, seed=0):
    """(n, d) float32, rows pairwise distinct permutations of multiset(kind, d, seed)."""
    ms, _ = multiset(kind, d, seed)
    rng = np.random.default_rng([seed, n, d, 7 + KINDS.index(kind)])
    X = rng.permuted(np.broadcast_to(ms, (n, d)), axis=1).astype(np.float32)
    assert len(np.unique(X, axis=0)) == n, "census rows must be pairwise distinct"
    return X


def partner(n, mask):
    """r ^ mask per row (an involution); -1 where the partner would lie past the corpus: that row stays single."""
    r = np.arange(n, dtype=np.int64)
    p = r ^ np.asarray(mask, np.int64)
    return np.where(p < n, p, -1)


def _swap_pair(X, rows, pair):
    """Copies of X[rows] with the coordinates holding pair[0] and pair[1] swapped."""
    Y = X[rows].copy()
    ia, ib = np.argmax(Y == pair[0], axis=1), np.argmax(Y == pair[1], axis=1)
    j = np.arange(len(rows))
    assert (Y[j, ia] == pair[0]).all() and (Y[j, ib] == pair[1]).all()
    Y[j, ia], Y[j, ib] = pair[1], pair[0]
    return Y


def twins(X, mask, pair):
    """(T, partner): T[r ^ mask] = X[r] with the pair swapped for every r with the mask bits clear and r ^ mask < N; `mask` is one
    mask or one per row (equal for both rows of a pair)."""
    n = len(X)
    p = partner(n, mask)
    lo = np.flatnonzero((p > np.arange(n)))
    assert (p[p[lo]] == lo).all()
    T = X.copy()
    T[p[lo]] = _swap_pair(X, lo, pair)
    assert len(np.unique(T, axis=0)) == n
    return T, p


def mixed_masks(n, rot=0):
    """Mask per row: 2048-row block j takes MASKS[(j + rot) % 7]."""
    return np.asarray(MASKS, np.int64)[(np.arange(n) // MIXED_BLOCK + rot) % len(MASKS)]


def twins_mixed(X, pair, rot=0):
    return twins(X, mixed_masks(len(X), rot), pair)


# ---- exact reference over the Gram matrix ---------------------------------------------------------------------------------------
def is_integer_kind(X):
    return bool((X == np.rint(X)).all())


def gram_topk(X, rows, k, metric, block=512, margin_rows=None):
    """Top-k of the queries X[rows] against X in the flat conventions (squared L2 ascending / inner product descending, float32
    distances, int64 ids), ordered by (value, id), every tie at the k-th place resolved towards the smaller id.

    Integer corpora: float32 sgemm is exact (every partial sum is an integer below 2**24, asserted), the distances are exact integers.
    Other corpora: float64; only the ids are meant to be used, and they are certain because the k-th and (k+1)-th keys are asserted to
    lie more than 1e-6 |x|^2 apart (`margin_rows`: a mask over `rows` of the queries this is asserted for -- a row without a twin has
    two random rows as its second and third neighbour, and its second id is not used)."""
    X = np.ascontiguousarray(X, np.float32)
    rows = np.asarray(rows, np.int64)
    n, d = X.shape
    k = int(k)
    assert 1 <= k <= n
    exact = is_integer_kind(X)
    if exact:
        assert float(np.abs(X).max()) ** 2 * d < 2 ** 24, "float32 Gram matrix would not be exact"
        W = X
        n2 = (X.astype(np.int64) ** 2).sum(axis=1)
    else:
        W = X.astype(np.float64)
        n2 = (W * W).sum(axis=1)
    D = np.empty((len(rows), k), np.float32)
    I = np.empty((len(rows), k), np.int64)
    for b0 in range(0, len(rows), block):
        rb = rows[b0:b0 + block]
        G = W[rb] @ W.T             # (integer kinds: float32 and exact; the L2 keys can pass 2**24, so they are formed in float64)
        key = (n2[rb][:, None] + n2[None, :] - 2 * G.astype(np.float64)) if metric == "l2" else -G
        if k < n:
            part = np.argpartition(key, k - 1, axis=1)[:, :k]
            kth = np.take_along_axis(key, part, axis=1).max(axis=1)
            cnt = (key <= kth[:, None]).sum(axis=1)
        else:
            part, cnt = np.broadcast_to(np.arange(n), (len(rb), n)), np.full(len(rb), n)
        if not exact and k < n:
            nxt = np.where(key > kth[:, None], key, np.inf).min(axis=1)
            sure = nxt - kth > 1e-6 * n2[rb]
            if margin_rows is not None:
                sure |= ~np.asarray(margin_rows, bool)[b0:b0 + block]
            assert sure.all(), "float64 reference: the k-th neighbour is not certain"
        for i in range(len(rb)):
            cand = part[i] if cnt[i] == k else np.flatnonzero(key[i] <= kth[i])     # every entry <= the k-th value
            cand = np.sort(cand)
            cand = cand[np.argsort(key[i, cand], kind="stable")][:k]                # (value, id)
            I[b0 + i] = cand
            kv = key[i, cand]
            D[b0 + i] = (kv if metric == "l2" else -kv).astype(np.float32)
    return D, I


# ---- restated geometry of the flat scan (csrc/scan_plan.hpp; held against the C++ itself by test_scan_plan_host.py) ------------------
BIN_ROWS = 256


def span_rows(d):
    return 1024 if d > 128 else 512


def bins_per_span(d):
    return 4 if d > 128 else 2


def nw_small(nq, small_batch=1):
    """Waves per workgroup of the serving shapes (8 = the batch shape)."""
    return 8 if not small_batch else 1 if nq <= 64 else 2 if nq <= 128 else 4 if nq <= 256 else 8


def qpad(nq):
    return (nq + 511) // 512 * 512


class Geometry:
    """What scan_geometry / scan_geometry_direct give: ok, nspans, spc (spans of the short chunks), rem (chunks one span longer),
    nchunks, starts (first span of every chunk, then nspans), direct_rows (0: standard geometry)."""

    def __init__(self, ok, nspans=0, spc=0, rem=0, nchunks=0, direct_rows=0):
        self.ok, self.nspans, self.spc, self.rem, self.nchunks, self.direct_rows = ok, nspans, spc, rem, nchunks, direct_rows
        self.starts = [c * spc + min(c, rem) for c in range(nchunks + 1)] if ok else []
        if ok:
            assert self.starts[-1] == nspans

    def chunk_sizes(self):
        return set(np.diff(self.starts).tolist())


def scan_geometry(n, d, k, nq, spans_per_chunk=0, small_batch=1):
    """scan_geometry(): G = 2 bins per 512-row span for D <= 128, G = 4 per 1024-row span above."""
    G, S = bins_per_span(d), span_rows(d)
    nspans = (n + S - 1) // S
    bad = Geometry(False, nspans)
    if nspans * G < 16:
        return bad
    spc_hi = nspans * G // (4 * k)
    spc_lo = (nspans * G + 1023) // 1024
    if spc_hi < 1 or spc_hi < spc_lo:
        return bad
    want = 32 // G
    if nq <= 512 and small_batch:
        want = max(1, min(want, nspans // 512))
    spc = max(min(spans_per_chunk if spans_per_chunk > 0 else want, spc_hi), spc_lo)
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
    spc = nspans // nchunks
    rem = nspans - spc * nchunks
    if spc < 1:
        return bad
    vpl = 1
    while vpl * 64 < G * nchunks:
        vpl *= 2
    if vpl > 16:
        return bad
    return Geometry(True, nspans, spc, rem, nchunks)


def scan_geometry_direct(n, d, k):
    """scan_geometry_direct() for the kernels that have the finer bins (the flat x16 / 32x32 scans, the K-loop scan)."""
    G, S = bins_per_span(d), span_rows(d)
    nspans = (n + S - 1) // S
    if nspans * G < 16:
        return Geometry(False, nspans)
    for rows in (128, 64):
        nb = nspans * G * (BIN_ROWS // rows)
        if 4 * k <= nb <= 2048:
            nchunks = (nspans * G + 31) // 32
            if nchunks >= 16:
                nchunks = (nchunks + 7) // 8 * 8
            nchunks = max(1, min(nchunks, nspans))
            spc = nspans // nchunks
            return Geometry(True, nspans, spc, nspans - spc * nchunks, nchunks, rows)
    return Geometry(False, nspans)


def geometry(n, d, k, nq, spans_per_chunk=0, small_batch=1):
    """The geometry a search takes: the standard one, else direct bins."""
    g = scan_geometry(n, d, k, nq, spans_per_chunk, small_batch)
    return g if g.ok else scan_geometry_direct(n, d, k)


def wide_tiles(nchunks, nq):
    """1024-query workgroup tiles (fp16 x16 at D <= 64, the int8 batch scans): Qpad a multiple of 1024 and >= 256 workgroups."""
    Q = qpad(nq)
    return Q % 1024 == 0 and nchunks * (Q // 1024) >= 256


def stride_order(n, s):
    """r = (j s) mod n, s coprime to n: a row meets another query column than its own offset."""
    assert np.gcd(n, s) == 1
    return (np.arange(n, dtype=np.int64) * s) % n


# ---- cached references of a census case --------------------------------------------------------------------------------------
class Case:
    """One corpus kind at one shape: the plain corpus X, the mixed-twin corpora ("twin", "twin1", "twin2": the deal of the masks rotated
    by 0, 1, 2 blocks; made on first use), and for each the exact top-3 of every row (ids and inner products from one Gram pass; equal
    norms make the L2 order the same and the L2 distance 2 (|x|^2 - G)).  Never modified."""

    def __init__(self, kind, n, d, seed=0):
        self.kind, self.n, self.d = kind, n, d
        self.ms, self.pair = multiset(kind, d, seed)
        self.X = corpus(kind, n, d, seed)
        self.X.setflags(write=False)
        self.exact = kind != "gauss"
        self.n2 = float((self.ms.astype(np.float64) ** 2).sum())
        self._ref, self._twin = {}, {}

    def _twins(self, which):
        if which not in self._twin:
            T, p = twins_mixed(self.X, self.pair, int(which[4:] or 0))
            T.setflags(write=False)
            p.setflags(write=False)
            self._twin[which] = (T, p)
        return self._twin[which]

    def rows(self, which):
        return self.X if which == "plain" else self._twins(which)[0]

    def partner(self, which):
        """Partner row of every row of a twin corpus, -1 for a row that stays single."""
        return self._twins(which)[1]

    def kmax(self, which):
        """Columns of the reference: 3 for the integer kinds; gauss: as many as are certain -- the row itself, and its twin."""
        return 3 if self.exact else 1 if which == "plain" else 2

    def ref(self, which, metric, k):
        """(D, I) of every row against the corpus `which`, k <= kmax.  D is exact for the integer kinds only; on gauss column 1 is
        certain for the rows that have a partner."""
        assert k <= self.kmax(which)
        if which not in self._ref:
            margin = None if which == "plain" else self.partner(which) >= 0
            G, I = gram_topk(self.rows(which), np.arange(self.n), self.kmax(which), "ip", margin_rows=margin)
            G.setflags(write=False)
            I.setflags(write=False)
            self._ref[which] = (G, I)
        G, I = self._ref[which]
        D = G if metric == "ip" else (2.0 * (self.n2 - G.astype(np.float64))).astype(np.float32)
        return D[:, :k], I[:, :k]


_CASES = {}


def case(kind, n, d, seed=0):
    key = (kind, n, d, seed)
    if key not in _CASES:
        _CASES[key] = Case(kind, n, d, seed)
    return _CASES[key]


def sample_rows(n, count=64):
    """A fixed sample of query rows: the first, the last, evenly spaced ones."""
    return np.unique(np.linspace(0, n - 1, count).astype(np.int64))


# ---- restated launch rules outside the scan geometry ---------------------------------------------------------------------------
def exact_blocked(nq, n, k, force_path=1):
    """search_exact(): the query-blocked exhaustive kernel (groups of 4 queries) serves when k <= 128, nq >= 8, `force_path` is not 3
    and there are at least 1024 (group, split) units; otherwise one wave per query."""
    kpl = 1
    while kpl * 64 < k:
        kpl *= 2
    if kpl > 2 or nq < 8 or force_path == 3:
        return False
    g4 = (nq + 3) // 4
    s4 = min((4096 + g4 - 1) // g4, max(1, n // 2048))
    return g4 * s4 >= 1024


def i8_batch_form(variant, nchunks, nq, x16, group=8):
    """scan_i8(): what `i8_variant` becomes for a batch-shaped launch (nq > 256): (query tile, tiles per stage, waves, pacing).
    Without 1024-query tiles that cover the chip (`wide_tiles`) every variant folds onto its low bit."""
    wide = wide_tiles(nchunks, nq)
    if x16:
        v = 3 if variant in (4, 5) else variant & 3
        if not wide:
            v &= 1
        return (1024 if v >= 2 else 512, 8 if v & 1 else 4, 8, 0)
    pace = {6: 1, 7: 2}.get(variant, 0)
    v = 3 if pace else variant
    if not wide:
        v &= 1
    if pace and not (v == 3 and group == 8):
        pace = 0
    return {0: (512, 4, 8), 1: (512, 8, 8), 2: (1024, 4, 8), 3: (1024, 8, 8), 4: (512, 8, 16), 5: (512, 16, 16)}[v] + (pace,)

"""Census corpora for the coded indexes (flat PQ<M>, IVF<nlist>,PQ<M>): codebooks and codes chosen so that the DECODED rows x^ are a
census corpus in the sense of tests/census.py -- every row its own strict nearest neighbour, a planted twin its strict second -- and a
restatement of the launch choices of the panel passes (launch_pq_panels in pq.inc, ivf_pq_panels in ivf_pq.inc, the slab cut of
scan_in_slabs in search_flat.inc) with which a test asserts the branch it names.  No GPU code.

Two constructions; both return (codebooks (M, 256, dsub) float32, codes (n, M) uint8, x^ (n, D) float32, partner (n,) int64).

slots    (M >= 8, any dsub)  M distinct sub-vectors S; row r holds S[perm_r[m]] in sub-space m, perm_r a permutation of 0..M-1, the
         perms pairwise distinct.  All rows have the norm of S, so a row is its own strict nearest neighbour under L2 and IP.  One
         pair (S[0], S[1]) has the uniquely smallest distance g of S; the twin of a row swaps the slots holding S[0] and S[1]: distance
         2 g^2.  Any other row differs in at least two slots, each by at least g, and not in exactly those two by exactly g each, so it
         is strictly farther.  The M used codes of sub-space m sit at scattered positions of 0..255 (0 and 255 among them), another
         choice per sub-space; the unused entries are decoys, far from every S[i].
entries  (dsub >= 6, any M)  the 256 entries of sub-space m are distinct permutations of one multiset of dsub values (norms equal
         whatever the codes), in pairs that differ by the swap of the two values a, a + gap of the multiset, every other two values
         being farther apart.  The twin changes ONE sub-space's code to the paired entry: distance 2 gap^2.  Every pair of twins (and
         every single row) has its own vector of entry PAIRS over the sub-spaces, so any other row differs somewhere by a permutation
         that is no such swap, which is strictly farther.  Every code 0..255 of every sub-space is in use.

Kinds: "int" -- small integers, exact in fp16 (the scans run with eps = 0) and in a float32 Gram matrix; "gauss" -- float32 with the gap
discipline of census.multiset("gauss"): the swapped pair is census.GAUSS_GAP apart, every other pair at least 1.25 times that.

`pin0` (the IVF-PQ corpora): sub-space 0 decodes to all zeros for every row -- a handful of all-zero entries at scattered codes, used in
turn -- and the permutation runs over sub-spaces 1 .. M-1 only.  With centroids of equal norm supported on the dims of sub-space 0
(`circle_centroids`) the decoded rows c_l + residual keep equal norms, and a row's own centroid is its nearest under L2 and IP.
"""
from __future__ import annotations

import itertools
import sys
from pathlib import Path

import numpy as np

from tests import census

sys.path.insert(0, str(Path(__file__).resolve().parent))

import ivfpq_restatement  # noqa: E402

F32 = np.float32
KINDS = ("int", "gauss")


# ---- pieces ---------------------------------------------------------------------------------------------------------------------
def _int_values(count, rng):
    """`count` distinct integers: 0 and 1 (the pair), every other one even and at least 2 away from both."""
    pool = np.array([v for v in range(-(count + 6), count + 8, 2) if v not in (0, 2)])
    return np.concatenate([[0, 1], rng.choice(pool, count - 2, replace=False)]).astype(F32)


def _gauss_values(count, seed):
    """`count` float32 values from census.multiset("gauss"), the pair (a, a + GAUSS_GAP) first."""
    ms, (a, b) = census.multiset("gauss", count, seed)
    rest = ms[(ms != a) & (ms != b)]
    return np.concatenate([[a, b], rest]).astype(F32)


def _positions(count, rng, need=(0, 255)):
    """`count` distinct codes of 0..255 in random order, 0 and 255 among them (and, from three codes on, one >= 128 besides 255)."""
    need = list(need[:count])
    if count >= 3:
        need.append(int(rng.integers(128, 255)))
    rest = np.setdiff1d(np.arange(256), need)
    pos = np.concatenate([need, rng.choice(rest, count - len(need), replace=False)]).astype(np.int64)
    return rng.permutation(pos)


def _pair_classes(width, count, rng):
    """`count` distinct permutations of 0..width-1 in which 0 stands before 1: one representative of `count` classes {p, p with 0 and 1
    swapped}.  Small widths are enumerated (8! / 2 = 20 160 classes), larger ones drawn and made unique."""
    if width <= 8:
        every = np.array([p for p in itertools.permutations(range(width)) if p.index(0) < p.index(1)], np.int16)
        assert count <= len(every), (width, count, len(every))
        return every[rng.choice(len(every), count, replace=False)]
    got = np.empty((0, width), np.int16)
    while len(got) < count:
        p = rng.permuted(np.broadcast_to(np.arange(width, dtype=np.int16), (count - len(got) + 16, width)), axis=1)
        got = np.unique(np.concatenate([got, _canonical(p)]), axis=0)
    return got[rng.permutation(len(got))[:count]]


def _swap01(p):
    """The permutations with the values 0 and 1 exchanged."""
    q = p.copy()
    q[p == 0], q[p == 1] = 1, 0
    return q


def _canonical(p):
    back = np.argmax(p == 0, axis=1) > np.argmax(p == 1, axis=1)
    q = p.copy()
    q[back] = _swap01(p[back])
    return q


def _check_partner(p):
    n = len(p)
    has = p >= 0
    assert (p[has] != np.flatnonzero(has)).all() and (p[p[has]] == np.flatnonzero(has)).all(), "partner must be an involution"
    return np.flatnonzero(has & (p > np.arange(n))), np.flatnonzero(~has)


# ---- slots ----------------------------------------------------------------------------------------------------------------------
def slot_vectors(kind, count, dsub, seed):
    """S (count, dsub): distinct sub-vectors; S[0], S[1] the uniquely nearest pair (they differ in the first coordinate only, by 1 /
    GAUSS_GAP; every other two differ there by at least 2 / 1.25 GAUSS_GAP)."""
    rng = np.random.default_rng([seed, count, dsub, 11 + KINDS.index(kind)])
    S = np.empty((count, dsub), F32)
    if kind == "int":
        S[:, 0] = _int_values(count, rng)
        S[:, 1:] = rng.integers(-30, 31, size=(count, dsub - 1))
    else:       # (the other coordinates are kept small: the margin gram_topk asserts is relative to |x|^2)
        S[:, 0] = _gauss_values(count, seed)
        S[:, 1:] = (0.3 * rng.standard_normal((count, dsub - 1))).astype(F32)
    S[1, 1:] = S[0, 1:]
    return S


def _decoys(kind, count, dsub, S, rng):
    """Entries no row uses: at least 40 (int) / 8 (gauss) beyond every S[i] in the first coordinate, pairwise distinct."""
    far = float(np.abs(S[:, 0]).max())
    D = np.empty((count, dsub), F32)
    if kind == "int":
        D[:, 0] = (far + 40 + rng.permutation(count)) * rng.choice([-1, 1], count)
        D[:, 1:] = rng.integers(-30, 31, size=(count, dsub - 1))
    else:
        D[:, 0] = ((far + 8.25 + 0.05 * rng.permutation(count)) * rng.choice([-1, 1], count)).astype(F32)
        D[:, 1:] = (0.3 * rng.standard_normal((count, dsub - 1))).astype(F32)
    return D


def slots(kind, d, M, partner, seed=0, pin0=False):
    n = len(partner)
    assert d % M == 0 and M >= 8 and kind in KINDS
    dsub = d // M
    rng = np.random.default_rng([seed, d, M, n, 21 + KINDS.index(kind)])
    lo, single = _check_partner(np.asarray(partner, np.int64))
    m0 = 1 if pin0 else 0                      # sub-spaces m0 .. M-1 carry the permutation
    W = M - m0
    S = slot_vectors(kind, W, dsub, seed)
    cls = _pair_classes(W, len(lo) + len(single), rng)
    flip = rng.random(len(cls)) < 0.5          # which member of its class the lower row of a pair (or a single row) takes
    first = np.where(flip[:, None], _swap01(cls), cls)
    perms = np.empty((n, W), np.int16)
    perms[lo], perms[partner[lo]] = first[:len(lo)], _swap01(first[:len(lo)])
    perms[single] = first[len(lo):]
    cb = np.empty((M, 256, dsub), F32)
    codes = np.empty((n, M), np.uint8)
    for m in range(m0, M):
        pos = _positions(W, rng)               # S[i] sits at code pos[i] of sub-space m
        cb[m] = _decoys(kind, 256, dsub, S, rng)
        cb[m, pos] = S
        codes[:, m] = pos[perms[:, m - m0]]
    xh = S[perms].reshape(n, W * dsub)
    if pin0:
        zeros = _positions(5, rng)
        cb[0] = _decoys(kind, 256, dsub, S, rng)
        cb[0, zeros] = 0
        codes[:, 0] = zeros[rng.integers(0, len(zeros), n)]
        xh = np.concatenate([np.zeros((n, dsub), F32), xh], axis=1)
    return cb, codes, np.ascontiguousarray(xh, F32), np.asarray(partner, np.int64)


# ---- entries --------------------------------------------------------------------------------------------------------------------
def entries(kind, d, M, partner, seed=0):
    n = len(partner)
    assert d % M == 0 and d // M >= 6 and kind in KINDS
    dsub = d // M
    rng = np.random.default_rng([seed, d, M, n, 31 + KINDS.index(kind)])
    partner = np.asarray(partner, np.int64)
    lo, _ = _check_partner(partner)
    cb = np.empty((M, 256, dsub), F32)
    code_of = np.empty((M, 128, 2), np.int64)  # the two codes of class i of sub-space m
    for m in range(M):
        vals = _int_values(dsub, rng) if kind == "int" else _gauss_values(dsub, seed * 1000 + m)
        cls = _pair_classes(dsub, 128, rng)
        code_of[m] = rng.permutation(256).reshape(128, 2)
        cb[m, code_of[m, :, 0]] = vals[cls]
        cb[m, code_of[m, :, 1]] = vals[_swap01(cls)]
    # A row is (class, member) per sub-space.  Rows one paired entry apart share their classes, so every pair of twins, and every
    # single row, gets a class vector ("cell") of its own: no two rows are equal, and a row's only neighbour at one paired entry is
    # its twin.  M <= 2: the cells are drawn without replacement (128^2 cells for 12 344 pairs and singles of the IVF corpus); above,
    # every class in turn, shuffled, and equal cells drawn again.
    single = _check_partner(partner)[1]
    count = len(lo) + len(single)
    if M <= 2:
        flat = rng.choice(128 ** M, count, replace=False)
        cell = np.stack([(flat // 128 ** m) % 128 for m in range(M)], axis=1)
    else:
        cell = np.stack([rng.permutation(np.resize(np.arange(128), count)) for _ in range(M)], axis=1)
        for _ in range(100):
            _, inv, cnt = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
            dup = np.flatnonzero(cnt[inv.reshape(-1)] > 1)
            if not len(dup):
                break
            cell[dup] = rng.integers(0, 128, size=(len(dup), M))
        else:
            raise AssertionError("could not draw distinct cells")
    member = np.stack([rng.permutation(np.resize(np.arange(2), count)) for _ in range(M)], axis=1)
    cols = np.arange(M)
    codes = np.empty((n, M), np.int64)
    codes[np.concatenate([lo, single])] = code_of[cols, cell, member]
    which = rng.integers(0, M, size=len(lo))   # the sub-space a pair differs in
    member[np.arange(len(lo)), which] ^= 1
    codes[partner[lo]] = code_of[cols, cell[:len(lo)], member[:len(lo)]]
    assert len(np.unique(codes, axis=0)) == n
    codes = codes.astype(np.uint8)
    xh = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)
    return cb, codes, np.ascontiguousarray(xh, F32), partner


def build(construction, kind, d, M, partner, seed=0, pin0=False):
    if construction == "slots":
        return slots(kind, d, M, partner, seed, pin0)
    assert construction == "entries" and not pin0
    return entries(kind, d, M, partner, seed)


def flat_partner(n, rot=0):
    """The partner of every row of a flat corpus: the masks of census.MASKS dealt over its 2048-row blocks."""
    return census.partner(n, census.mixed_masks(n, rot))


def list_partner(lor, masks, nlist):
    """Inside every list (list order = id order) the row at position j ^ mask is the partner of the row at position j; the mask of list
    l is masks[l % len(masks)]."""
    p = np.full(len(lor), -1, np.int64)
    for l in range(nlist):
        members = np.flatnonzero(lor == l)
        j = np.arange(len(members))
        q = j ^ masks[l % len(masks)]
        ok = q < len(members)
        p[members[j[ok]]] = members[q[ok]]
    return p


def circle_centroids(kind, nlist, d, dsub):
    """`nlist` centroids of equal norm, supported on the first two dims (inside sub-space 0, dsub >= 2): the integer points of the
    circle a^2 + b^2 = 27 625 = 5^3 13 17 (there are exactly 64), scaled to radius 4 for the float kind."""
    assert dsub >= 2 and nlist <= 64
    r2 = 27625
    pts = [(a, b) for a in range(-167, 168) for b in range(-167, 168) if a * a + b * b == r2]
    assert len(pts) == 64
    C = np.zeros((nlist, d), F32)
    C[:, :2] = np.array(pts[:nlist], F32)
    if kind == "gauss":
        C *= F32(4.0 / np.sqrt(r2))
    return C


# ---- a flat PQ census case: corpora and exact references, cached ------------------------------------------------------------------
class CodedCase:
    """Same surface as census.Case ("plain" and "twin" are ONE corpus here: every corpus carries its twins), so that the helpers of
    the flat census serve: rows(which), partner(which), kmax(which), ref(which, metric, k), .n, .d, .exact."""

    def __init__(self, construction, kind, n, d, M, seed=0):
        self.construction, self.kind, self.n, self.d, self.M = construction, kind, n, d, M
        self.cb, self.codes, self.X, self.p = build(construction, kind, d, M, flat_partner(n), seed)
        for a in (self.cb, self.codes, self.X, self.p):
            a.setflags(write=False)
        self.exact = kind == "int"
        self.n2 = float((self.X[0].astype(np.float64) ** 2).sum())
        self._ref = None

    def rows(self, which):
        return self.X

    def partner(self, which):
        return self.p

    def kmax(self, which):
        return 2

    def ref(self, which, metric, k):
        assert k <= 2
        if self._ref is None:
            G, I = census.gram_topk(self.X, np.arange(self.n), 2, "ip", margin_rows=self.p >= 0)
            has = self.p >= 0                  # a census corpus: every row its own first neighbour, the planted twin its second
            assert (I[:, 0] == np.arange(self.n)).all() and (I[has, 1] == self.p[has]).all()
            G.setflags(write=False)
            I.setflags(write=False)
            self._ref = (G, I)
        G, I = self._ref
        D = G if metric == "ip" else (2.0 * (self.n2 - G.astype(np.float64))).astype(np.float32)
        return D[:, :k], I[:, :k]


_CASES = {}


def case(construction, kind, n, d, M, seed=0):
    key = (construction, kind, n, d, M, seed)
    if key not in _CASES:
        _CASES[key] = CodedCase(*key)
    return _CASES[key]


# ---- restated launch choices ------------------------------------------------------------------------------------------------------
PQ_LDS_BUDGET = 80 * 1024          # kPqLdsBudget (pq.inc)
PQ_TAB_SKEW = 8                    # kPqTabSkew (pq.hpp), halves
PQ_SLAB_ROWS = 524_288             # kPqSlabRows (scan_plan.hpp)
IVFPQ_LDS_BUDGET = 64 * 1024       # kIvfPqLdsBudget (ivf_pq.inc)
IVFPQ_CENT_FLOATS = 128            # kIvfPqCentFloats (ivf_pq.hpp)


def flat_ksteps(d):
    """vdb_create: 16-dim k-steps of the register-resident scans (D <= 128), four per 64 dims of the K-loop scan above."""
    return 4 if d <= 64 else 8 if d <= 128 else (d + 63) // 64 * 4


def _code_pitch(M):
    pitch = (M + 3) & ~3
    return pitch + 4 if (pitch // 4) % 2 == 0 else pitch


def pq_panel_launch(d, M):
    """What launch_pq_panels chooses: p16 (layout of D > 128), W (halves per gather), vec (dword staging), table ("lds": whole in LDS,
    "sliced": k-step slices over blockIdx.y, "cache": read through the cache), ks32 (32-dim steps), slice_ks, gy, last (steps of the
    last slice), partial (the last 32-dim step that holds a dim holds fewer than 32), pad8 (D % 8 != 0)."""
    dsub = d // M
    p16 = flat_ksteps(d) > 8
    ks32 = flat_ksteps(d) // 2
    stage = 4 * (((16 if p16 else 32) * _code_pitch(M) + 15) & ~15)
    unit = next(dsub // g for g in (32, 16, 8, 4, 2, 1) if dsub % g == 0)
    table, slice_ks = "cache", ks32
    if stage + 512 * d + M * PQ_TAB_SKEW * 2 <= PQ_LDS_BUDGET:
        table = "lds"
    else:
        unit_bytes = unit * 32 * 512 + (unit * 32 // dsub) * PQ_TAB_SKEW * 2
        units = (PQ_LDS_BUDGET - stage) // unit_bytes
        if units >= 1 and p16:
            table, slice_ks = "sliced", units * unit
    gy = -(-ks32 // slice_ks)
    return dict(p16=p16, W=8 if dsub % 8 == 0 else 4 if dsub % 4 == 0 else 2 if dsub % 2 == 0 else 1, vec=M % 4 == 0, table=table,
                ks32=ks32, slice_ks=slice_ks, gy=gy, last=ks32 - (gy - 1) * slice_ks, partial=d % 32 != 0, pad8=d % 8 != 0)


def ivfpq_panel_launch(d, M):
    """What ivf_pq_panels chooses (D <= 128): lds, slice_ks (16-dim k-steps per blockIdx.y slice, halved from ksteps until the float32
    codebooks of the widest slice fit), gy, vec."""
    assert d <= 128
    dsub, ksteps = d // M, flat_ksteps(d)
    fixed = 4 * (((32 * _code_pitch(M) + 15) & ~15) + IVFPQ_CENT_FLOATS * 4)
    lds, slice_ks, s = False, ksteps, ksteps
    while s >= 1 and not lds:
        worst = 0
        for ks_lo in range(0, ksteps, s):
            d_lo, d_hi = min(ks_lo * 16, d), min(d, (ks_lo + s) * 16)
            worst = max(worst, ((d_hi + dsub - 1) // dsub - d_lo // dsub) * 256 * dsub)
        if fixed + worst * 4 <= IVFPQ_LDS_BUDGET:
            lds, slice_ks = True, s
        s //= 2
    return dict(lds=lds, slice_ks=slice_ks, gy=-(-ksteps // slice_ks), vec=M % 4 == 0, pad16=d % 16 != 0)


def slab_cut(g, d, pq_slab_chunks=0):
    """scan_in_slabs for a PQ index under the geometry g (census.Geometry): [(first chunk, chunks, first span, spans)] per slab."""
    chunk_rows = (g.spc + 1) * census.span_rows(d)
    per = pq_slab_chunks if pq_slab_chunks > 0 else max(1, PQ_SLAB_ROWS // chunk_rows)
    per = max(1, min(per, g.nchunks))
    out = []
    for c0 in range(0, g.nchunks, per):
        c1 = min(g.nchunks, c0 + per)
        out.append((c0, c1 - c0, g.starts[c0], min(g.nspans, g.starts[c1]) - g.starts[c0]))
    return out


# ---- the shapes of the GPU cases (tests/test_gpu_census_pq.py, tests/test_gpu_census_ivf_coded.py) --------------------------------
# flat PQ: (D, M, construction, kind, rows): 17 409 / 17 508 rows = 35 spans of 512, the last holding 1 / 100 rows; D > 128:
# 18 433 / 18 443 rows = 19 spans of 1024, the last holding 1 / 11
PQ_SHAPES = [
    (64, 8, "slots", "int", 17_409), (64, 8, "entries", "gauss", 17_508), (128, 32, "slots", "gauss", 17_508),
    (100, 50, "slots", "int", 17_409), (50, 50, "slots", "gauss", 17_508), (128, 128, "slots", "int", 17_409),
    (384, 64, "entries", "int", 18_443), (384, 96, "slots", "gauss", 18_433), (200, 25, "entries", "int", 18_433),
    (240, 16, "slots", "gauss", 18_443), (320, 40, "slots", "int", 18_443)]
# IVF-PQ: (D, M, construction, kind, metrics)
IVFPQ_SHAPES = [(48, 12, "slots", "int", ("l2", "ip")), (128, 64, "slots", "gauss", ("l2", "ip")),
                (100, 25, "slots", "int", ("l2", "ip")), (128, 2, "entries", "int", ("l2",))]
IVF_N, IVF_NLIST = 20_011, 64
LIST_MASKS = (4, 64, 256)


def ivf_lists(n=IVF_N, nlist=IVF_NLIST, seed=0):
    """The list of every row: list 0 and lists 8 .. 11 empty, list 2 one row, lists 4 / 5 / 6 of 255 / 256 / 257 rows, list 1 of 1900,
    the others share the rest; ids are dealt at random, so a list's rows are scattered over the id range."""
    sizes = np.zeros(nlist, np.int64)
    sizes[[2, 4, 5, 6, 1]] = (1, 255, 256, 257, 1900)
    free = [l for l in range(nlist) if l not in (0, 1, 2, 4, 5, 6, 8, 9, 10, 11)]
    rest = n - sizes.sum()
    sizes[free] = rest // len(free)
    sizes[free[:rest % len(free)]] += 1
    assert sizes.sum() == n
    lor = np.repeat(np.arange(nlist), sizes)
    return np.random.default_rng([seed, n, nlist]).permutation(lor).astype(np.int32)


def ivfpq_corpus(d, M, construction, kind, seed=0):
    """(centroids, codebooks, codes, list of every row, partner, x^ = ivfpq_restatement.decode) of an IVF-PQ census corpus.  slots: `pin0` rows under
    circle_centroids -- equal norms, so both metrics serve.  entries (M = 2: every sub-space must vary, or a list could not hold 1900
    distinct rows): centroids 1300 e_l, farther apart (1838) than twice the residual norm, so a row's own centroid is its nearest
    under L2; the norms of c_l + residual differ, so these corpora run under L2 only."""
    lor = ivf_lists(seed=seed)
    partner = list_partner(lor, LIST_MASKS, IVF_NLIST)
    if construction == "slots":
        C = circle_centroids(kind, IVF_NLIST, d, d // M)
        cb, codes, _, _ = slots(kind, d, M, partner, seed, pin0=True)
    else:
        assert kind == "int" and d >= IVF_NLIST
        C = np.zeros((IVF_NLIST, d), F32)
        C[np.arange(IVF_NLIST), np.arange(IVF_NLIST)] = 1300
        cb, codes, xr, _ = entries(kind, d, M, partner, seed)
        assert 2 * float(np.sqrt((xr.astype(np.float64) ** 2).sum(axis=1).max())) < 1300 * np.sqrt(2)
    return C, cb, codes, lor, partner, ivfpq_restatement.decode(codes, C, lor, cb)

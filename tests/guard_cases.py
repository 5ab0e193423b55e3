"""Inputs on which the exactness guard decides the answer, and a host-side check that they do.

On random data tau -- the k-th smallest bin minimum -- lies far above the k-th true distance, so a search stays exact with
eps = 0.  Here every query has k + 1 near-copies of one row as its nearest rows: the copies differ by less than the fp16
resolution of the scan, their float64 keys are all distinct, and the rounded scores order them differently from the exact
keys for a large share of the queries.  A select that drops the 2 eps term then returns a wrong id for those queries.

No GPU here: `emulated_scores` restates the scan in NumPy (inputs scaled by the library's power-of-two scales and rounded to
fp16, float32 scores) and `critical_share` is the share of queries the emulation gets wrong.  tests/test_guard_host.py holds
every case of tests/test_gpu_guard.py to a floor on that share."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

F32 = np.float32
REL = 3e-4               # relative size of a replica's perturbation: below the fp16 unit roundoff 2^-11 = 4.9e-4
FINE, FINE_RANGE = 8, 3e-4
FLOOR = 0.20             # smallest critical share a GPU case may have


def _place(reps, layout):
    """reps (c, nb, d) -> rows.  blocked: replica j in rows [j nb, (j + 1) nb).  strided: the replicas of a row s = 8 rows apart
    inside one 256-row bin, row = (i // s) * s c + j * s + i % s.  strided32: s = 32, for inverted lists -- a list keeps about
    a quarter of the rows, in order, so the replicas of a row end up about 8 list rows apart: other quads of the same bin."""
    c, nb, d = reps.shape
    if layout == "blocked":
        return reps.reshape(c * nb, d)
    s = stride_of(layout)
    assert nb % s == 0
    return np.ascontiguousarray(reps.reshape(c, nb // s, s, d).transpose(1, 0, 2, 3)).reshape(c * nb, d)


def stride_of(layout):
    if layout not in ("strided", "strided32"):
        raise ValueError(layout)
    return 8 if layout == "strided" else 32


def _frozen(*arrays):
    """the makers are cached: what they hand out is shared, so it is read-only"""
    for a in arrays:
        a.flags.writeable = False
    return arrays


def cluster_rows(nb, k, layout):
    """(nb, k + 1) int64: the rows of base row i's replicas."""
    c = k + 1
    i = np.arange(nb)[:, None]
    j = np.arange(c)[None, :]
    if layout == "blocked":
        return j * nb + i
    s = stride_of(layout)
    return (i // s) * s * c + j * s + i % s


@lru_cache(maxsize=4)
def make_clusters(nb, k, d, nq, seed, layout="blocked", kind="gauss", qnoise=None, qshift=0.37):
    """(X, Q) float32: c = k + 1 replicas of nb base rows, and nq queries next to base rows drawn without replacement.
    kind: "gauss" | "unit" (rows normalised, for IP) | "offset" (50 + 0.1 N: cancellation in ||x||^2 - 2 q.x) |
    "fine" (for 8-bit codes: the replicas are exact copies but for the last FINE coordinates, 1 + FINE_RANGE U(0, 1) -- a
    range so small that one code step of a scalar quantizer trained on the corpus stays below the fp16 resolution) |
    "bytes" (integer rows in 0..255, replicas differ by +-1 in one coordinate, queries B + qshift + qnoise N: the corpus is
    exact in fp16 and only the query rounds -- no GPU case uses it, tests/test_guard_host.py records why)."""
    rng = np.random.default_rng(seed)
    c = k + 1
    if kind == "bytes":
        B = rng.integers(1, 255, size=(nb, d)).astype(np.float64)
        reps = np.repeat(B[None], c, axis=0)
        for j in range(1, c):       # replica 0 is the base row; the others move one coordinate (a different one each) by +-1
            col = (rng.integers(0, d, nb) + j) % d
            reps[j, np.arange(nb), col] += rng.choice([-1.0, 1.0], nb)
        pick = rng.choice(nb, nq, replace=False)
        Q = B[pick] + qshift + (0.2 if qnoise is None else qnoise) * rng.standard_normal((nq, d))
        return _frozen(_place(reps, layout).astype(F32), Q.astype(F32))
    B = rng.standard_normal((nb, d))
    if kind == "offset":
        B = 50.0 + 0.1 * B
    elif kind == "unit":
        B /= np.linalg.norm(B, axis=1, keepdims=True)
    elif kind not in ("gauss", "fine"):
        raise ValueError(kind)
    if kind == "fine":
        reps = np.repeat(B[None], c, axis=0)
        reps[:, :, -FINE:] = 1.0 + FINE_RANGE * rng.random((c, nb, FINE))
    else:
        reps = B[None] * (1.0 + REL * rng.standard_normal((c, nb, d)))
    if kind == "unit":
        reps /= np.linalg.norm(reps, axis=2, keepdims=True)
    pick = rng.choice(nb, nq, replace=nq > nb)
    noise = 0.05 if qnoise is None else qnoise
    Q = B[pick] + noise * rng.standard_normal((nq, d))
    if kind == "fine":
        Q[:, -FINE:] = 1.0 + FINE_RANGE * rng.random((nq, FINE))
    return _frozen(_place(reps, layout).astype(F32), Q.astype(F32))


@lru_cache(maxsize=4)
def make_pq_clusters(nb, k, nq, seed, layout="blocked", d=64, M=16, fam=16, qnoise=0.05, rel=REL):
    """(codebooks (M, 256, d / M), codes (c nb, M) uint8, Q): every sub-space holds 256 / fam families of `fam` near-copy
    centroids; a base row draws one family per sub-space and each replica a member of it, so the reconstructed replicas are
    near-copies of one another.  The queries sit next to the family heads' row."""
    rng = np.random.default_rng(seed)
    c, dsub, nfam = k + 1, d // M, 256 // fam
    heads = rng.standard_normal((M, nfam, 1, dsub))
    cb = (heads * (1.0 + rel * rng.standard_normal((M, nfam, fam, dsub)))).reshape(M, 256, dsub).astype(F32)
    family = rng.integers(0, nfam, size=(nb, M))
    codes = (family[None] * fam + rng.integers(0, fam, size=(c, nb, M))).astype(np.uint8)
    pick = rng.choice(nb, nq, replace=False)
    base = heads[np.arange(M)[None, :], family[pick], 0].reshape(nq, d)
    Q = base + qnoise * rng.standard_normal((nq, d))
    return _frozen(cb, _place(codes, layout), Q.astype(F32))


def scales(X, Q, metric):
    """(sx, sq) as vdbhip.hip index_stats and prep.hpp query_finalize_values choose them."""
    fm = 2.0 if metric == "l2" else 1.0
    absmax = float(np.abs(X).max())
    int_unscaled = bool((X == np.rint(X)).all()) and absmax <= 2048.0
    sx = 1.0
    if not int_unscaled and absmax > 0:
        sx = float(np.ldexp(1.0, 14 - np.frexp(F32(absmax))[1]))
    amax = float(np.abs(Q).max())
    sq = 1.0
    if not (int_unscaled and bool((Q == np.rint(Q)).all()) and fm * amax <= 2048.0) and amax > 0:
        sq = float(np.ldexp(1.0, 14 - np.frexp(F32(fm * amax))[1]))
    return sx, sq


def emulated_scores(X, Q, metric):
    """(nq, n) float32 scan scores: bias cs ||x||^2 (L2) + fp16(-fm sq q) . fp16(sx x), accumulated in float32."""
    X, Q = np.asarray(X, F32), np.asarray(Q, F32)
    sx, sq = scales(X, Q, metric)
    fm = 2.0 if metric == "l2" else 1.0
    xh = (X * F32(sx)).astype(np.float16).astype(F32)
    qh = (Q * F32(-fm * sq)).astype(np.float16).astype(F32)
    s = qh @ xh.T
    if metric == "l2":
        n2 = (X.astype(np.float64) ** 2).sum(axis=1).astype(F32)
        s = s + (n2 * F32(sq * sx))[None, :]
    return s.astype(F32)


def exact_keys(X, Q, metric):
    """(nq, n) float64 order keys (smaller = nearer): ||x - q||^2 or -q.x over the float32 inputs."""
    X, Q = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    g = Q @ X.T
    if metric == "ip":
        return -g
    return (X * X).sum(axis=1)[None, :] - 2.0 * g + (Q * Q).sum(axis=1)[:, None]


def _first(keys, m):
    """per row the m smallest entries' columns in (key, column) order, and their keys"""
    part = np.sort(np.argpartition(keys, m - 1, axis=1)[:, :m], axis=1)
    kp = np.take_along_axis(keys, part, axis=1)
    order = np.argsort(kp, axis=1, kind="stable")
    return np.take_along_axis(part, order, axis=1), np.take_along_axis(kp, order, axis=1)


def critical_mask(X, Q, metric, k, restrict=None):
    """Per query: (a) the exact k-th and (k + 1)-th float64 keys differ and (b) the emulated top-k set (ties by the smaller
    row) is not the exact one.  A tie among emulated scores counts: the scans pack the id of a row's group into the low
    mantissa bits of a score, so equal scores are ordered by position, not by distance.
    restrict: (nq, n) bool, the rows a query may see (the probed lists of an IVF search)."""
    keys = exact_keys(X, Q, metric)
    emu = emulated_scores(X, Q, metric).astype(np.float64)
    if restrict is not None:
        keys = np.where(restrict, keys, np.inf)
        emu = np.where(restrict, emu, np.inf)
    cols, kk = _first(keys, k + 1)
    distinct = kk[:, k - 1] != kk[:, k]
    ecols, _ = _first(emu, k)
    differ = np.array([set(a) != set(b) for a, b in zip(cols[:, :k].tolist(), ecols.tolist())])
    return distinct & differ


def critical_share(X, Q, metric, k, restrict=None):
    """Share of the queries that `critical_mask` marks."""
    return float(np.mean(critical_mask(X, Q, metric, k, restrict)))


# ---- IVF: four injected centroids, the lists and the probed lists on the host ------------------------------------------------
def ivf_centroids(d, kind="gauss"):
    """centre +- scale e0, centre +- scale e1: under either metric a row goes by the larger of |x0 - centre|, |x1 - centre|
    and its sign, a quarter of symmetric data to each list."""
    centre, scale = 0.0, 0.5
    C = np.full((4, d), centre, F32)
    C[0, 0], C[1, 0], C[2, 1], C[3, 1] = centre + scale, centre - scale, centre + scale, centre - scale
    return C


def _coarse_keys(C, X, metric):
    C, X = np.asarray(C, np.float64), np.asarray(X, np.float64)
    g = X @ C.T
    return -g if metric == "ip" else (C * C).sum(axis=1)[None, :] - 2.0 * g


def host_assign(C, X, metric):
    """int32 list of every row: the nearest centroid in float64, the smaller list id on a tie."""
    return np.argmin(_coarse_keys(C, X, metric), axis=1).astype(np.int32)


def probed_mask(C, lor, Q, metric, nprobe):
    """(nq, n) bool: row in one of the query's nprobe nearest lists."""
    order = np.argsort(_coarse_keys(C, Q, metric), axis=1, kind="stable")[:, :nprobe]
    hit = np.zeros((len(Q), len(C)), bool)
    np.put_along_axis(hit, order, True, axis=1)
    return hit[:, lor]


def list_gaps(lor, nb, k, layout):
    """(clusters, k) list-row distance between consecutive replicas of every base row whose replicas share a list (the lists
    keep their rows in id order), and the share of the base rows that do."""
    order = np.argsort(lor, kind="stable")
    pos = np.empty(len(lor), np.int64)
    pos[order] = np.arange(len(lor))
    rows = cluster_rows(nb, k, layout)
    same = (lor[rows] == lor[rows[:, :1]]).all(axis=1)
    return np.diff(pos[rows[same]], axis=1), float(same.mean())


def check_list_layout(lor, c):
    """The replicas of a row lie where the layout of the case wants them inside their list.  blocked: every replica block gives
    every list >= 1024 rows, so two replicas are never in one bin.  strided32: for most rows consecutive replicas are 4..63 list
    rows apart -- other quads, and mostly the same bin of 64 rows or more."""
    if c.layout == "blocked":
        assert block_list_counts(lor, c.nb).min() >= 1024
        return
    gaps, same = list_gaps(lor, c.nb, c.replicas_k, c.layout)
    assert same > 0.9, same
    assert ((gaps >= 4) & (gaps < 64)).all(axis=1).mean() > 0.6, float(((gaps >= 4) & (gaps < 64)).all(axis=1).mean())


def block_list_counts(lor, nb, nlist=4):
    """(c, nlist): rows that replica block j of a blocked corpus contributes to every list."""
    return np.stack([np.bincount(b, minlength=nlist) for b in lor.reshape(-1, nb)])


# ---- the cases of tests/test_gpu_guard.py ------------------------------------------------------------------------------------
NQ = 256
SHAPES = ((16384, 1), (8192, 4), (4096, 10))        # (nb, k): 32 768 to 45 056 rows


@dataclass(frozen=True)
class Case:
    family: str              # the path family of the matrix (the mutation record counts failures per family)
    index: str               # flat | multi | partial | ivf | sq8 | pq | coarse
    metric: str
    nb: int
    k: int
    d: int
    kind: str = "gauss"
    layout: str = "blocked"
    ck: int = 0              # replicas - 1 where it is not the k of the search (0: k)
    nq: int = NQ             # queries searched; below NQ: the first nq of the NQ generated ones, critical ones first
    pre: tuple = ()          # options set before the add, ((name, value), ...)
    post: tuple = ()         # options set after it
    nprobe: int = 0
    shape: int = -1          # expected scan_shape (-1: not asserted)
    qnoise: float = None
    qshift: float = 0.37
    rel: float = REL         # pq: relative spread of a centroid family

    @property
    def replicas_k(self):
        return self.ck or self.k

    @property
    def id(self):
        opts = ",".join(f"{n}={v:g}" for n, v in self.pre + self.post)
        bits = [self.family, self.index, self.metric, f"d{self.d}", f"nb{self.nb}", f"k{self.k}", self.kind, self.layout]
        if self.ck:
            bits.append(f"replicas{self.ck + 1}")
        if self.nq != NQ:
            bits.append(f"nq{self.nq}")
        if self.nprobe:
            bits.append(f"nprobe{self.nprobe}")
        return "-".join(bits + ([opts] if opts else []))

    @property
    def data_key(self):
        """what the rows, the queries and the host condition depend on"""
        return (self.index if self.index in ("ivf", "sq8", "pq", "coarse") else "flat", self.metric, self.nb, self.k, self.d, self.kind,
                self.layout, self.replicas_k, self.nprobe, self.qnoise, self.qshift, self.rel, max(NQ, self.nq))


def case_inputs(c, seed=7):
    """(rows or codes, Q, codebooks or None): at least NQ queries, however few c.nq says."""
    nq = max(NQ, c.nq)
    if c.index == "pq":
        cb, codes, Q = make_pq_clusters(c.nb, c.replicas_k, nq, seed, c.layout, d=c.d, rel=c.rel)
        return codes, Q, cb
    if c.index == "coarse":      # the rows are the centroids, the "queries" the rows that are filed under them
        X, Q = make_clusters(c.nb, c.replicas_k, c.d, 4096, seed, c.layout, c.kind, c.qnoise, c.qshift)
        return X, Q, None
    X, Q = make_clusters(c.nb, c.replicas_k, c.d, nq, seed, c.layout, c.kind, c.qnoise, c.qshift)
    return X, Q, None


def pick_queries(c, Q, crit):
    """The c.nq queries of a case that searches fewer than it generates: critical ones first, in their order."""
    if c.nq >= len(Q):
        return np.arange(len(Q))
    order = np.concatenate([np.flatnonzero(crit), np.flatnonzero(~crit)])
    return np.sort(order[:c.nq]) if c.nq > 16 else order[:c.nq]


def _flat(family, metric, nb, k, d, **kw):
    kw.setdefault("kind", "unit" if metric == "ip" else "gauss")
    return Case(family, kw.pop("index", "flat"), metric, nb, k, d, **kw)


def _cases():
    out = []
    # flat, D <= 128, default layout x16: both metrics, every shape, a multiple of 16 dims and not; both layouts at D = 64
    for metric in ("l2", "ip"):
        for nb, k in SHAPES:
            out.append(_flat("flat128", metric, nb, k, 64, shape=16))
            out.append(_flat("flat128", metric, nb, k, 100, shape=16))
            if k == 1:      # (replicas inside one bin decide tau only at k = 1: for larger k other superbins set it far above them)
                out.append(_flat("flat128", metric, nb, k, 64, layout="strided", shape=16))
    # the 32x32 form with octs (flat_shape 32) and with quads (f16_group 4)
    for pre in ((("flat_shape", 32),), (("f16_group", 4),)):
        for nb, k in SHAPES:
            out.append(_flat("flat128", "l2", nb, k, 64, pre=pre, shape=32))
        out.append(_flat("flat128", "ip", 8192, 4, 100, pre=pre, shape=32))
        out.append(_flat("flat128", "l2", 16384, 1, 64, layout="strided", pre=pre, shape=32))
    # the three selects: 81 920 rows give 160 superbins, where select_variant 2 has a form of its own
    for v in (0, 1, 2):
        out.append(_flat("flat128", "l2", 16384, 4, 64, post=(("select_variant", v),), shape=16))
        out.append(_flat("flat128", "ip", 16384, 4, 64, post=(("select_variant", v),), shape=16))
        out.append(_flat("flat128", "l2", 16384, 1, 64, post=(("select_variant", v),), shape=16))
    # (the one-wave select and the 32-lane form on replicas inside one bin: their second-minimum re-scan; k = 1, see above)
    for v in (1, 2):
        out.append(_flat("flat128", "l2", 16384, 1, 64, ck=4, layout="strided", post=(("select_variant", v),), shape=16))
    out.append(_flat("flat128", "l2", 16384, 1, 64, layout="strided", post=(("select_variant", 1),), shape=16))
    # serving shapes (1, 2, 4 waves per workgroup and the batch shape), and the batch shape forced
    for nq in (1, 16, 200, 512):
        out.append(_flat("flat128", "l2", 16384, 1, 64, nq=nq, shape=16))
        out.append(_flat("flat128", "ip", 8192, 4, 100, nq=nq, shape=16))
    out.append(_flat("flat128", "l2", 16384, 1, 64, post=(("small_batch", 0),), shape=16))
    out.append(_flat("flat128", "l2", 4096, 10, 64, post=(("small_batch", 0),), shape=16))
    # statistics inside the prep kernel (nq D <= 4096) and in a kernel of their own
    for v in (1, 0):
        out.append(_flat("flat128", "l2", 16384, 1, 64, nq=64, post=(("fused_stats", v),), shape=16))
        out.append(_flat("flat128", "ip", 8192, 4, 64, nq=64, post=(("fused_stats", v),), shape=16))
    # flat, D > 128: the K-loop scan, resident panels and panels converted per search in several slabs
    for d in (200, 384):
        for nb, k in SHAPES:
            out.append(_flat("flat_kloop", "l2", nb, k, d, shape=0))
        out.append(_flat("flat_kloop", "ip", 8192, 4, d, shape=0))
        out.append(_flat("flat_kloop", "l2", 16384, 1, d, layout="strided", shape=0))
    for nb, k in SHAPES:
        out.append(_flat("flat_kloop", "l2", nb, k, 200, pre=(("stream_panels", 1), ("stream_slab_rows", 8192)), shape=0))
    out.append(_flat("flat_kloop", "ip", 16384, 1, 384, pre=(("stream_panels", 1), ("stream_slab_rows", 8192)), shape=0))
    # dense small-corpus path: scores of 8192 rows in LDS, of 2048 rows in registers
    for metric in ("l2", "ip"):
        out.append(_flat("dense", metric, 4096, 1, 64, shape=32))
        out.append(_flat("dense", metric, 2048, 3, 100, shape=32))
        out.append(_flat("dense", metric, 1024, 1, 64, shape=32))
        out.append(_flat("dense", metric, 1024, 1, 100, layout="strided", shape=32))
    # several shards in one handle, and per-shard partial lists merged on the device: two replicas of every row per shard
    out.append(_flat("shards", "l2", 16384, 1, 64, ck=5, index="multi"))
    out.append(_flat("shards", "ip", 16384, 1, 64, ck=5, index="multi"))
    out.append(_flat("shards", "l2", 16384, 1, 64, ck=3, index="partial"))
    # IVF-Flat, four injected centroids
    ivf_shapes = ((16384, 1), (8192, 4), (8192, 10))
    for metric in ("l2", "ip"):
        for nb, k in ivf_shapes:
            for nprobe in (1, 4):
                out.append(_flat("ivf128", metric, nb, k, 64, index="ivf", nprobe=nprobe))
        out.append(_flat("ivf128", metric, 8192, 4, 100, index="ivf", nprobe=4))
    for bt in (4, 16):
        out.append(_flat("ivf128", "l2", 8192, 4, 64, index="ivf", nprobe=4, post=(("ivf_bt", bt),)))
    # replicas inside one bin of a list (strided32): the select's second / third quad minimum and whole-bin re-scan
    out.append(_flat("ivf128", "l2", 16384, 1, 64, index="ivf", nprobe=4, layout="strided32"))
    out.append(_flat("ivf128", "l2", 8192, 4, 64, index="ivf", nprobe=4, layout="strided32"))
    out.append(_flat("ivf128", "ip", 8192, 4, 100, index="ivf", nprobe=1, layout="strided32"))
    out.append(_flat("ivf128", "l2", 8192, 4, 64, index="ivf", nprobe=4, layout="strided32", post=(("ivf_bt", 4),)))
    for tps in (16, 64):
        for nb, k in ivf_shapes:
            out.append(_flat("ivf_kloop", "l2", nb, k, 200, index="ivf", nprobe=4, pre=(("ivf_tps", tps),)))
        out.append(_flat("ivf_kloop", "ip", 8192, 4, 200, index="ivf", nprobe=1, pre=(("ivf_tps", tps),)))
        out.append(_flat("ivf_kloop", "l2", 16384, 1, 200, index="ivf", nprobe=4, layout="strided32", pre=(("ivf_tps", tps),)))
        out.append(_flat("ivf_kloop", "l2", 8192, 4, 200, index="ivf", nprobe=4, layout="strided32", pre=(("ivf_tps", tps),)))
    for group in (1, 2, 4):
        out.append(_flat("ivf_kloop", "l2", 8192, 4, 200, index="ivf", nprobe=4, pre=(("ivf_tps", 16),), post=(("ivf_group", group),)))
    for tile in (1, 2):
        out.append(_flat("ivf_kloop", "l2", 16384, 1, 200, index="ivf", nprobe=4, pre=(("ivf_tps", 16),), post=(("ivf_tile", tile),)))
    # the coarse quantizer itself: 64 pairs of near-copy centroids, rows filed under the nearer one (set-only register select)
    for metric in ("l2", "ip"):
        out.append(_flat("coarse", metric, 64, 1, 64, index="coarse", nprobe=1))
    # IVF-SQ8: ranges trained on the corpus, the decoded rows are the corpus of the oracle and of the host condition
    for metric in ("l2", "ip"):
        for nb, k in ivf_shapes:
            out.append(_flat("ivf_sq8", metric, nb, k, 64, index="sq8", kind="fine", nprobe=4))
        out.append(_flat("ivf_sq8", metric, 8192, 4, 64, index="sq8", kind="fine", nprobe=1))
    out.append(_flat("ivf_sq8", "l2", 16384, 1, 64, index="sq8", kind="fine", nprobe=4, layout="strided32"))
    out.append(_flat("ivf_sq8", "ip", 8192, 4, 64, index="sq8", kind="fine", nprobe=4, layout="strided32"))
    # PQ16 with injected codebooks of near-copy centroid families
    for metric in ("l2", "ip"):
        for nb, k in SHAPES:
            out.append(Case("pq", "pq", metric, nb, k, 64, kind="families", post=(("pq_slab_chunks", 1),),
                            rel=REL if metric == "l2" else 1e-4))
        out.append(Case("pq", "pq", metric, 16384, 1, 64, kind="families", layout="strided", post=(("pq_slab_chunks", 1),),
                        rel=REL if metric == "l2" else 1e-4))
    return out


CASES = _cases()

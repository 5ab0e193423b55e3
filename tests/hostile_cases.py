"""Hostile values for every search path: the inputs of tests/test_hostile_host.py and tests/test_gpu_hostile.py.

NumPy only, no GPU import.  include/vdbhip.h promises a result that is exact "for any input"; the fp16 / int8 scans only nominate
candidates, and a batch whose scales are unusable is served by the exhaustive float64 pass.  What decides that is value
arithmetic (corpus_stats_kernel, index_stats, query_finalize_values).  The families below put magnitudes, infinities and NaNs on
both sides of every threshold of that arithmetic:

  ladder    X = G 10^a, Q = H 10^b, a and b over LADDER (float32 subnormals at the bottom, clipped to FLT_MAX at the top)
  outlier   a unit-scale corpus with m rows scaled by 10^18 / 10^30 (every other row's fp16 image is 0), and the transpose;
            one row with a squared norm of 2e38, finite but above the scans' marker of a padding row
  tiny      one dimension of every row is 1e15, the others ~1
  subnormal rows m 2^-149 e_d, queries of subnormal primes, -0.0 among the zeros
  inf-rows  r rows with one +-inf coordinate (keys +-inf, never NaN), k inside / at / past the finite rows
  inf-query, nan-query   one query of a batch of 8 holds inf / NaN; the same query alone
  nan-rows  a few rows hold np.nan
  bytes     a 0..255 integer corpus (keeps the int8 copy) under the ladder's, the inf / NaN and near-byte query batches

`groups(family, n, d)` returns the corpora of a family with the query batches each one is searched with (one index per corpus
serves all of them); `cases(family, n, d)` flattens that to (name, X, Q, metric, k, expectations) tuples.  `corpus_scales` and
`batch_label` restate the scale arithmetic in NumPy float32 and label a (corpus, batch, metric) "must" (the batch must be
flagged for the exhaustive pass), "may" (the MFMA scan must serve it) or None (nearer than a factor 4 to a threshold: only the
result is compared)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

SEED = 20261020
D = 16
NQ = 8
K = 10
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
TINY = 2.0 ** -149                       # the smallest float32 subnormal
LADDER = (-44, -40, -36, -30, -20, -10, 0, 10, 20, 30, 36, 38)
FAMILIES = ("ladder", "outlier", "tiny", "subnormal", "inf-rows", "inf-query", "nan-query", "nan-rows", "bytes")
BAD_QUERY = 3                            # the query of a batch of 8 that holds the inf / NaN
# thresholds of query_finalize_values (csrc/prep.hpp); tests/test_hostile_host.py reads them back from the source
TOP_MAX, SCALE_MIN, AMAX_GATE, Q_FP16_MAX, NORM_MAX, LABEL_MARGIN = 1.0e30, 1.0e-30, 3.0e38, 65504.0, 0.9e38, 4.0


@dataclass(frozen=True, eq=False)
class Corpus:
    name: str
    X: np.ndarray
    expect: Dict[str, object] = field(default_factory=dict)


@dataclass(frozen=True, eq=False)
class Batch:
    name: str
    Q: np.ndarray
    expect: Dict[str, object] = field(default_factory=dict)


@dataclass(frozen=True, eq=False)
class Group:
    corpus: Corpus
    batches: Tuple[Batch, ...]
    metrics: Tuple[str, ...] = ("l2", "ip")
    ks: Tuple[int, ...] = (K,)


def _rng(*tag) -> np.random.Generator:
    return np.random.default_rng([SEED, zlib.crc32(repr(tag).encode())])


def _f32(a) -> np.ndarray:
    with np.errstate(over="ignore", under="ignore"):
        return np.ascontiguousarray(np.clip(a, -FLT_MAX, FLT_MAX).astype(F32))


@lru_cache(maxsize=None)
def _gauss(tag: str, n: int, d: int) -> np.ndarray:
    g = _rng("gauss", tag, n, d).standard_normal((n, d))
    g.setflags(write=False)
    return g


def _unit_queries(d: int, nq: int = NQ, tag: str = "H") -> np.ndarray:
    """Gaussian queries, every coordinate at least 0.1 from zero (so q_c * inf is +-inf, never NaN)"""
    h = _gauss(tag, nq, d).copy()
    return np.where(np.abs(h) < 0.1, np.copysign(0.1, h), h)


# ---- the scale arithmetic of the library, restated -----------------------------------------------------------------------------
def corpus_scales(X: np.ndarray) -> Dict[str, object]:
    """index_stats (csrc/vdbhip.hip) on the statistics of corpus_stats_kernel (csrc/prep.hpp)"""
    X = np.asarray(X, F32)
    with np.errstate(all="ignore"):
        nonfinite = bool(not np.isfinite(X).all())
        absmax = F32(np.fmax.reduce(np.abs(X), axis=None, initial=F32(0)))          # fmaxf drops NaN
        norm2_f64 = (X.astype(np.float64) ** 2).sum(axis=1)
        maxnorm2 = F32(np.fmax.reduce(norm2_f64.astype(F32), initial=F32(0)))       # float64 sum, rounded once
        not_integer = bool((X != np.rint(X)).any())
        int_unscaled = (not not_integer) and (not nonfinite) and bool(absmax <= F32(2048))
        sx = F32(1)
        if not int_unscaled and absmax > 0 and not nonfinite:
            sx = np.ldexp(F32(1), 14 - int(np.frexp(absmax)[1])).astype(F32)
        byte = (not nonfinite) and (not not_integer) and bool(((X >= 0) & (X <= 255)).all() or ((X >= -128) & (X <= 127)).all())
        norm32 = F32(0)                                                              # what a float32 accumulation would give
        if not nonfinite:
            acc = np.zeros(len(X), F32)
            for c in range(X.shape[1]):
                acc = (acc + X[:, c] * X[:, c]).astype(F32)
            norm32 = F32(acc.max(initial=F32(0)))
    return dict(nonfinite=nonfinite, absmax=absmax, maxnorm2=maxnorm2, int_unscaled=int_unscaled, sx=sx, byte=byte,
                norm_overflow=bool(np.isinf(maxnorm2)) and not nonfinite, sx_overflow=bool(np.isinf(sx)),
                norm32_max=norm32, norm64_max=float(norm2_f64.max(initial=0.0)) if not nonfinite else float("nan"))


def batch_scales(cs: Dict[str, object], Q: np.ndarray, metric: str) -> Dict[str, object]:
    """query_finalize_values (csrc/prep.hpp): sq, top = sq sx maxnorm2, force_fallback, the int8 window"""
    Q = np.asarray(Q, F32)
    with np.errstate(all="ignore"):
        fm = F32(2 if metric == "l2" else 1)
        amax = F32(np.fmax.reduce(np.abs(Q), axis=None, initial=F32(0)))
        nonfinite = bool(not np.isfinite(Q).all())
        not_integer = bool((Q != np.rint(Q)).any())
        int_ok = bool(cs["int_unscaled"]) and not not_integer and bool(fm * amax <= F32(2048))
        sq = F32(1)
        if not int_ok and amax > 0 and amax <= F32(AMAX_GATE):
            sq = np.ldexp(F32(1), 14 - int(np.frexp(F32(fm * amax))[1])).astype(F32)
        scale = F32(sq * cs["sx"])
        top = F32(scale * cs["maxnorm2"])
        qtop = F32(F32(fm * amax) * sq)                      # the largest scaled query value: must stay finite in fp16
        fallback = nonfinite or not bool(top < F32(TOP_MAX)) or not bool(scale > F32(SCALE_MIN)) or \
            not bool(qtop <= F32(Q_FP16_MAX)) or not bool(cs["maxnorm2"] < F32(NORM_MAX))
        u8 = (not not_integer) and bool(((Q >= 0) & (Q <= 255)).all())
        s8 = (not not_integer) and bool(((Q >= -128) & (Q <= 127)).all())
    return dict(sq=sq, scale=scale, top=top, qtop=qtop, nonfinite=nonfinite, fallback=fallback, amax=amax,
                i8=bool(cs["byte"]) and not nonfinite and (u8 or s8))


def batch_label(cs: Dict[str, object], Q: np.ndarray, metric: str) -> Optional[str]:
    """"exact": a non-finite corpus keeps no scan copy.  "must": the batch must be flagged.  "may": the scan must serve it.
    None: top, the scale or the largest scaled query value is within LABEL_MARGIN of its threshold (a last-bit difference could flip the device's decision)."""
    if cs["nonfinite"]:
        return "exact"
    b = batch_scales(cs, Q, metric)
    if b["nonfinite"]:
        return "must"
    with np.errstate(all="ignore"):
        top_above = not bool(b["top"] < F32(TOP_MAX * LABEL_MARGIN))           # (NaN and inf included)
        top_below = bool(b["top"] < F32(TOP_MAX / LABEL_MARGIN))
        scale_below = not bool(b["scale"] > F32(SCALE_MIN / LABEL_MARGIN))
        scale_above = bool(b["scale"] > F32(SCALE_MIN * LABEL_MARGIN))
        q_above = not bool(b["qtop"] <= F32(Q_FP16_MAX * LABEL_MARGIN))
        q_below = bool(b["qtop"] <= F32(Q_FP16_MAX / LABEL_MARGIN))
        norm_above = not bool(cs["maxnorm2"] < F32(NORM_MAX) * F32(LABEL_MARGIN))      # (float32: only inf is that far above)
        norm_below = bool(cs["maxnorm2"] < F32(NORM_MAX / LABEL_MARGIN))
    if top_above or scale_below or q_above or norm_above:
        return "must"
    if top_below and scale_above and q_below and norm_below:
        return "may"
    return None


# ---- corpora and batches ---------------------------------------------------------------------------------------------------------
def _corpus(name: str, X: np.ndarray, **expect) -> Corpus:
    X = _f32(X) if X.dtype != F32 else np.ascontiguousarray(X)
    X.setflags(write=False)
    return Corpus(name, X, dict(expect))


def _batch(name: str, Q: np.ndarray, **expect) -> Batch:
    Q = _f32(Q) if Q.dtype != F32 else np.ascontiguousarray(Q)
    Q.setflags(write=False)
    return Batch(name, Q, dict(expect))


def ladder_corpus(a: int, n: int, d: int) -> Corpus:
    return _corpus(f"ladder-x{a:+d}", _gauss("G", n, d) * 10.0 ** a, step=a)


@lru_cache(maxsize=None)
def ladder_batches(d: int, nq: int = NQ) -> Tuple[Batch, ...]:
    return tuple(_batch(f"q{b:+d}", _gauss("H", nq, d) * 10.0 ** b, step=b) for b in LADDER)


def unit_corpus(n: int, d: int) -> Corpus:
    return _corpus("unit", _gauss("G", n, d))


def unit_batch(d: int, nq: int = NQ) -> Batch:
    return _batch("q-unit", _unit_queries(d, nq))


def _spread(n: int, r: int, lo: int = 0) -> np.ndarray:
    """r row numbers spread over [lo, n): the first, the last and evenly between"""
    return np.unique(np.linspace(lo, n - 1, r).round().astype(np.int64)) if r > 1 else np.array([lo + (n - lo) // 2])


def outlier_groups(n: int, d: int) -> List[Group]:
    out = []
    G = _gauss("G", n, d)
    for s in (18, 30):
        for m in (1, 5):
            X = G.copy()
            rows = _spread(n, m)
            X[rows] *= 10.0 ** s
            out.append(Group(_corpus(f"outlier-{m}x1e{s}", X, outliers=tuple(rows.tolist()), scale=s), (unit_batch(d),)))
    # one row whose squared norm, 2e38, is finite in float32 but above the 0.9e38 that the scans read as a padding row; the first
    # query is that row itself, so it is the nearest neighbour of a query (L2 key 0, and the largest inner product)
    X = G.copy()
    row = n // 2
    X[row] *= np.sqrt(2.0e38 / (X[row] ** 2).sum())
    Q = _unit_queries(d)
    Q[0] = X[row]
    out.append(Group(_corpus("outlier-norm-2e38", X, outliers=(row,), scale=19), (_batch("q-on-the-outlier", Q),)))
    # ... and the whole corpus at that scale (largest squared norm 2e38): the rows of largest norm lie above 0.9e38, the queries are
    # the eight longest of them shrunk by 0.1 %, so each query's nearest row is one of those, and keys of one magnitude do not tie
    g2 = (G ** 2).sum(axis=1)
    c = np.sqrt(2.0e38 / g2.max())
    longest = np.sort(np.argsort(g2)[-NQ:])
    out.append(Group(_corpus("scaled-to-norm-2e38", G * c, scale=19, longest=tuple(longest.tolist())),
                     (_batch("q-near-the-longest-rows", G[longest] * (c * 0.999)),)))
    tb = []
    for s in (18, 30):                                     # the transpose: one query of the batch scaled, the other seven not
        Q = _unit_queries(d)
        Q[BAD_QUERY] *= 10.0 ** s
        tb.append(_batch(f"q-outlier-1e{s}", Q, scaled_query=BAD_QUERY, scale=s))
    out.append(Group(unit_corpus(n, d), tuple(tb)))
    return out


def tiny_groups(n: int, d: int) -> List[Group]:
    """dimension 0 of every row is 1e15 (exactly float32(1e15)); the other dimensions, ~1, decide the order for the queries
    that hold the same 1e15 (L2: the difference is 0) or 0 (IP: the product is 0) there.  The remaining queries hold the other of
    the two, so the float64 keys absorb the small dimensions and tie: those queries come back in id order."""
    X = _gauss("G", n, d).copy()
    X[:, 0] = 1.0e15
    Q = _unit_queries(d)
    Q[0::2, 0] = 1.0e15
    Q[1::2, 0] = 0.0
    return [Group(_corpus("tiny-next-to-huge", X, huge_dim=0), (_batch("q-tiny", Q),))]


def _primes_above(lo: int, count: int) -> np.ndarray:
    out, c = [], lo + 1
    while len(out) < count:
        if all(c % p for p in range(2, int(c ** 0.5) + 1)):
            out.append(c)
        c += 1
    return np.array(out, np.float64)


def subnormal_groups(n: int, d: int) -> List[Group]:
    """row j = +-m 2^-149 e_c with c = j % d, m = 1 + j // d (negative for every third row), -0.0 in the zeros of odd rows;
    query i = S p_c 2^-149 with p the primes above M = max m, rotated by i and with alternating signs.  Every product q_c m is
    distinct (m is smaller than every prime), so IP keys never tie; with S a power of two above M^2 / 2 the L2 keys
    |q|^2 + m^2 - 2 q_c m cannot tie either (two products differ by at least S).  S is halved while a query value would leave
    the subnormal range (corpora of more than ~2000 rows at d = 16): L2 keys may then tie, and the id decides.  All arithmetic is
    exact in float64 (integers times 2^-298)."""
    X = np.zeros((n, d))
    j = np.arange(n)
    X[1::2] = -0.0
    X[j, j % d] = np.where(j % 3 == 2, -1.0, 1.0) * (1 + j // d) * TINY
    M = 1 + (n - 1) // d
    p = _primes_above(M, d)
    S = 1
    while 2 * S <= M * M:
        S *= 2
    while S > 1 and S * p.max() >= 2 ** 23:
        S //= 2
    p = p * S
    Q = np.stack([np.roll(p, i) * np.where((np.arange(d) + i) % 2, -1.0, 1.0) for i in range(NQ)]) * TINY
    return [Group(_corpus("subnormal", X), (_batch("q-subnormal", Q),))]


def inf_row_groups(n: int, d: int, with_centroid: int = 0) -> List[Group]:
    """r rows with one +-inf coordinate each (signs alternate); `with_centroid`: the first of them is moved below that row
    number (an IVF test takes its centroids from the first rows).  Small corpora get the k sweep around the finite rows."""
    out = []
    for r in (1, 7):
        X = _gauss("G", n, d).astype(F32)
        rows = _spread(n, r, lo=min(20, n // 2))
        if with_centroid:
            rows[0] = with_centroid - 1
        for i, row in enumerate(rows):
            X[row, (3 * i + 1) % d] = np.inf if i % 2 == 0 else -np.inf
        ks = [K]
        if n <= 2000:
            ks = sorted({max(1, n - r - 3), n - r, n - r + 1, n, min(n + 5, 2048)})
        out.append(Group(_corpus(f"inf-rows-{r}" + ("-centroid" if with_centroid else ""), X, inf_rows=tuple(rows.tolist())),
                         (unit_batch(d),), ks=tuple(ks)))
    return out


def bad_query_batches(d: int, value: float, name: str) -> Tuple[Batch, ...]:
    Q = _unit_queries(d).astype(F32)
    Q[BAD_QUERY, 5 % d] = value
    return (_batch(f"q-{name}-of-8", Q, bad_queries=(BAD_QUERY,)),
            _batch(f"q-{name}-alone", Q[BAD_QUERY:BAD_QUERY + 1].copy(), bad_queries=(0,)))


def nan_row_groups(n: int, d: int) -> List[Group]:
    X = _gauss("G", n, d).astype(F32)
    rows = _spread(n, 5, lo=min(20, n // 2))
    for i, row in enumerate(rows):
        X[row, (5 * i + 2) % d] = np.nan               # np.nan: the positive quiet NaN
    ks = (K,) if n > 2000 else (K, n - len(rows), n)
    return [Group(_corpus("nan-rows", X, nan_rows=tuple(rows.tolist())), (unit_batch(d),), ks=ks)]


def byte_corpus(n: int, d: int) -> Corpus:
    X = _rng("bytes", n, d).integers(0, 256, size=(n, d)).astype(np.float64)
    X[:, 5 % d] = np.maximum(X[:, 5 % d], 1.0)         # (the coordinate of the inf query: 0 * inf would be a NaN key under IP)
    return _corpus("bytes", X)


def byte_groups(n: int, d: int) -> List[Group]:
    Qb = _rng("qbytes", d).integers(0, 256, size=(NQ, d)).astype(np.float64)
    near = []
    for v, name in ((255.5, "255.5"), (1.0e6, "1e6")):
        Q = Qb.copy()
        Q[2, 5 % d] = v
        near.append(_batch(f"q-bytes-{name}", Q))
    batches = (_batch("q-bytes", Qb),) + tuple(near) + ladder_batches(d) + bad_query_batches(d, np.inf, "inf") + \
        bad_query_batches(d, np.nan, "nan")
    return [Group(byte_corpus(n, d), batches)]


@lru_cache(maxsize=None)
def groups(family: str, n: int, d: int = D, with_centroid: int = 0) -> Tuple[Group, ...]:
    if family == "ladder":
        return tuple(Group(ladder_corpus(a, n, d), ladder_batches(d)) for a in LADDER)
    if family == "outlier":
        return tuple(outlier_groups(n, d))
    if family == "tiny":
        return tuple(tiny_groups(n, d))
    if family == "subnormal":
        return tuple(subnormal_groups(n, d))
    if family == "inf-rows":
        return tuple(inf_row_groups(n, d, with_centroid))
    if family == "inf-query":
        return (Group(unit_corpus(n, d), bad_query_batches(d, np.inf, "inf")),)
    if family == "nan-query":
        return (Group(unit_corpus(n, d), bad_query_batches(d, np.nan, "nan")),)
    if family == "nan-rows":
        return tuple(nan_row_groups(n, d))
    if family == "bytes":
        return tuple(byte_groups(n, d))
    raise AssertionError(family)


def cases(family: str, n: int, d: int = D):
    """(name, X, Q, metric, k, expectations) of every search of a family; expectations: the corpus's and the batch's facts, the
    restated scales and the path label"""
    out = []
    for g in groups(family, n, d):
        cs = corpus_scales(g.corpus.X)
        for b in g.batches:
            for metric in g.metrics:
                exp = dict(g.corpus.expect)
                exp.update(b.expect)
                exp.update(corpus=cs, batch=batch_scales(cs, b.Q, metric), label=batch_label(cs, b.Q, metric))
                for k in g.ks:
                    out.append((f"{g.corpus.name}/{b.name}/{metric}/k{k}", g.corpus.X, b.Q, metric, k, exp))
    return out

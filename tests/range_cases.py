"""Inputs on which the `+ eps` of a range search's prefilter threshold decides the answer, and its restatement on the host.

A range search keeps every row whose fp16 scan score is <= thr[q] = cs (radius - ||q||^2) + eps[q] (L2) or
cs (-radius) + eps[q] (IP) and filters those exactly.  On random data the scores near the radius are far apart and eps = 0 would do.
Here the radius cuts through clusters of near-copies: c = 11 replicas of nb base rows, B (1 + REL N(0, 1)), differ by less than the
fp16 resolution of the scan, and every query sits at the radius from its base row -- so about half of the replicas of its cluster
are true results, and their rounded scores fall on either side of an unwidened threshold.

  L2   query = B[pick] + rho u, u a unit vector; radius = float32(rho^2)
  IP   query = B[pick] rho / ||B[pick]||^2, so that q . B[pick] = rho; radius = rho (Gaussian rows: unit rows under IP with
       rho = 1 give no true result at all)

NumPy only.  `emulated_threshold` restates range_thr_kernel with a given eps, `library_eps` restates query_eps_body (csrc/prep.hpp);
tests/test_range_host.py holds every case to guard_cases.FLOOR with eps = 0 and to no miss with the library's bound, and
tests/test_gpu_range.py runs the same cases on the GPU bit for bit."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import guard_cases as gc

F32 = np.float32
REPLICAS = 11


@dataclass(frozen=True)
class Case:
    nb: int
    d: int
    nq: int
    metric: str
    rho: float

    @property
    def id(self):
        return f"nb{self.nb}-d{self.d}-nq{self.nq}-{self.metric}-rho{self.rho:g}"


# 16 500 rows at D = 64 take layout "x16", 2 200 rows at D = 200 the p16 panels
CASES = (Case(1500, 64, 256, "l2", 0.4), Case(1500, 64, 256, "l2", 2.0), Case(1500, 64, 256, "ip", 60.0),
         Case(200, 200, 64, "l2", 0.7), Case(200, 200, 64, "ip", 150.0))


@lru_cache(maxsize=None)
def make(c: Case, seed: int = 11):
    """(X (11 nb, d), Q (nq, d), radius) float32, read-only"""
    rng = np.random.default_rng([seed, c.nb, c.d, c.nq])
    B = rng.standard_normal((c.nb, c.d))
    reps = B[None] * (1.0 + gc.REL * rng.standard_normal((REPLICAS, c.nb, c.d)))
    X = reps.reshape(REPLICAS * c.nb, c.d).astype(F32)
    pick = rng.choice(c.nb, c.nq, replace=False)
    if c.metric == "l2":
        u = rng.standard_normal((c.nq, c.d))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        Q = B[pick] + c.rho * u
        radius = F32(c.rho * c.rho)
    else:
        Q = B[pick] * (c.rho / (B[pick] ** 2).sum(axis=1))[:, None]
        radius = F32(c.rho)
    Q = Q.astype(F32)
    X.flags.writeable = False
    Q.flags.writeable = False
    return X, Q, radius


def expected(keys: np.ndarray, radius, metric: str, id_base: int = 0):
    """The contract applied to canonical float64 keys (nq, N): (lims, D, I), ascending id per query."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (keys if metric == "l2" else -keys).astype(F32)
        hit = d < F32(radius) if metric == "l2" else d > F32(radius)
    lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    q, row = np.nonzero(hit)                 # row-major: ascending row inside ascending query
    return lims, d[q, row], (row + id_base).astype(np.int64)


def ksteps(d: int) -> int:
    return 4 if d <= 64 else 8 if d <= 128 else (d + 63) // 64 * 4


def library_eps(X, Q, metric):
    """(nq,) float32: query_eps_body (csrc/prep.hpp) for the fp16 scan, in scan units."""
    X, Q = np.asarray(X, F32), np.asarray(Q, F32)
    sx, sq = gc.scales(X, Q, metric)
    l2 = metric == "l2"
    fm = 2.0 if l2 else 1.0
    bs, cs = F32(-fm * sq), sq * sx
    d = Q.shape[1]
    maxnorm2 = F32((X.astype(np.float64) ** 2).sum(axis=1).astype(F32).max())
    Xn = float(F32(np.sqrt(maxnorm2, dtype=F32) * F32(1.0000002)))
    xs = X * F32(sx)
    corpus_exact = bool((xs.astype(np.float16).astype(F32) == xs).all())
    int_unscaled = bool((X == np.rint(X)).all()) and float(np.abs(X).max()) <= 2048.0
    qs = Q * bs
    inexact = (qs.astype(np.float16).astype(F32) != qs).any(axis=1)
    notint = (Q != np.rint(Q)).any(axis=1)
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(axis=1))
    u = 2.0 ** -11
    ux, uq = (0.0 if corpus_exact else u), np.where(inexact, u, 0.0)
    rel_in = ux + uq + ux * uq
    mag = Xn * Xn + 2.0 * qn * Xn if l2 else qn * Xn
    dot_err = rel_in * qn * Xn + np.where(rel_in > 0, 2.0 ** -36 * np.sqrt(d) * qn * Xn, 0.0)
    dot_err = dot_err + np.where(inexact, 2.0 ** -25 / abs(float(bs)) * np.sqrt(d) * Xn, 0.0)
    int_exact = int_unscaled & ~notint & (sq == 1.0) & (sx == 1.0) & (mag * 1.000001 < 16777216.0)
    acc_err = np.where(int_exact, 0.0, (ksteps(d) * 16 + 3) * 2.0 ** -23 * mag)
    pack_err = 2.0 ** -17 * mag
    bias_err = np.where(int_exact, 0.0, 2.0 ** -24 * Xn * Xn) if l2 else 0.0
    key_err = np.where(int_exact, 0.0, (d + 3) * 2.0 ** -52 * (qn + Xn) ** 2) if l2 else 0.0
    e = np.minimum(cs * (fm * dot_err + acc_err + pack_err + bias_err + key_err) * 1.02, 1.0e37)
    return e.astype(F32) + F32(1.0e-30)


def emulated_threshold(X, Q, radius, metric, eps):
    """(nq,) float32: range_thr_kernel (csrc/range.hpp) with the given eps -- float64, rounded up."""
    X, Q = np.asarray(X, F32), np.asarray(Q, F32)
    sx, sq = gc.scales(X, Q, metric)
    cs, r, d = sq * sx, float(radius), Q.shape[1]
    eps = np.asarray(eps, np.float64)
    if metric == "l2":
        n2 = (Q.astype(np.float64) ** 2).sum(axis=1)
        t = cs * (r - n2)
        allow = cs * (d + 4) * 2.0 ** -52 * (abs(r) + n2) * (eps > 0)       # (eps = 0: the bare threshold)
    else:
        t, allow = np.full(len(Q), cs * -r), 0.0
    t = t + eps + allow
    t = t + np.abs(t) * 2.0 ** -52 * (eps > 0)
    tf = t.astype(F32)
    return np.where(tf.astype(np.float64) < t, np.nextafter(tf, F32(np.inf)), tf)


def missed_share(X, Q, radius, metric, keys, eps):
    """(share of the queries with at least one true result whose emulated score lies above the threshold, mean true results)"""
    hit = expected(keys, radius, metric)[0]
    d = (keys if metric == "l2" else -keys).astype(F32)
    truth = d < radius if metric == "l2" else d > radius
    cand = gc.emulated_scores(X, Q, metric) <= emulated_threshold(X, Q, radius, metric, eps)[:, None]
    return float((truth & ~cand).any(axis=1).mean()), float(np.diff(hit).mean())

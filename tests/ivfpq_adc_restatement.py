"""NumPy restatement of the lookup-table (ADC) scan of the probed lists of an IVF<nlist>,PQ<M> index (csrc/ivf_pq_adc.hpp,
DESIGN 4.4 "IVF-PQ ADC scan").  Test infrastructure only: nothing in the product imports it.

  n2       n2[i] = float32 of the float64 chain sum_d fma(x^_d, x^_d, acc), d ascending, x^ = float32(c_l[d] + codebook entry)
  handle   Xn^2 = max n2 (the float32 values), Cn = max ||c_l||, Rn = sqrt(sum_m max_c ||cb[m][c]||^2); usable when Xn^2 and
           (Cn + Rn)^2 lie in [1e-30, 1e30]
  mag'     Xn^2 + 2 qn (Cn + Rn) (L2) | qn (Cn + Rn) (IP), qn^2 the float64 chain sum_d fma(q_d, q_d, acc)
  cs       2^-ilogb(largest mag' of the batch's usable queries) (1 when there is none); a query is flagged (exact list scan) when it
           is not finite, its mag' lies outside [1e-35, 1e35], cs mag' < 1e-25, or (L2) ||q||^2 > 1e8 (Cn + Rn)^2
  T        pq_adc_restatement.tables
  B        B[q][p] = float32(bs * acc), acc = sum_d fma(q_d, c_l[d], acc), bs = -2 cs (L2) | -cs (IP)
  score    s_0 = float32(cs * n2[row]) (L2) | 0 (IP); s_1 = s_0 + B; s_{m+2} = s_{m+1} + T[m][code[row][m]]: float32 adds, m ascending
  eps      float32(1.02 cs (M + 4) 2^-23 mag') + 1e-30
  tail     tau = the k-th smallest score of the query's probed rows (+inf when there are fewer); candidates: s <= tau + 2 eps
  admission  ivf_adc_plan (csrc/ivf_plan.hpp)
"""
from __future__ import annotations

import math

import numpy as np

from tests import pq_adc_restatement as ar

F32 = np.float32
MAX_BATCH, MAX_K, MAX_PARTS, AUX_BYTES, LDS_BUDGET, SCORE_BYTES, CAND_MAX = 512, 1024, 64, 128, 160 * 1024, 256 << 20, 4096


def _chain(a, b):
    """float64 (rows,): acc = fma(a[:, d], b[:, d], acc), d ascending from 0.0 (a, b broadcastable to one 2-d shape)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    acc = np.zeros(a.shape[0], np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        wild = ~np.isfinite((a * b).sum(axis=1))      # rows with a NaN, an infinity or an overflow: plain arithmetic names the outcome
        fine = np.flatnonzero(~wild)
        for d in range(a.shape[1]):
            acc[fine] = ar._fma_add(a[fine, d], b[fine, d], acc[fine])
        acc[wild] = (a[wild] * b[wild]).sum(axis=1)
    return acc


def n2_of(Xhat):
    """float32 (n,)"""
    with np.errstate(over="ignore"):
        return _chain(Xhat, Xhat).astype(F32)


def handle(Xhat, C, cb):
    """(Xn2, CR, usable): the three magnitudes of the bound as the host computes them (plain float64 sums: compare eps to 1e-6)."""
    Xn2 = float(n2_of(Xhat).max())
    C64, cb64 = np.asarray(C, F32).astype(np.float64), np.asarray(cb, F32).astype(np.float64)
    Cn = math.sqrt(float((C64 * C64).sum(axis=1).max()))
    Rn = math.sqrt(float((cb64 * cb64).sum(axis=2).max(axis=1).sum()))
    CR = Cn + Rn
    ok = (1.0e-30 <= Xn2 <= 1.0e30) and (1.0e-30 <= CR * CR <= 1.0e30)
    return Xn2, CR, ok


def mags(Q, metric, Xn2, CR):
    """(qn2, mag') float64 (nq,)"""
    with np.errstate(over="ignore", invalid="ignore"):
        qn2 = _chain(Q, Q)
        qn = np.sqrt(qn2)
        return qn2, (Xn2 + 2.0 * qn * CR if metric == "l2" else qn * CR)


def usable(qn2, mag):
    with np.errstate(invalid="ignore"):
        return (qn2 <= 1.0e300) & (mag >= 1.0e-35) & (mag <= 1.0e35)


def cs_of(qn2, mag):
    ok = usable(qn2, mag)
    if not ok.any():
        return 1.0
    _, e = math.frexp(float(mag[ok].max()))        # top = m 2^e, m in [0.5, 1): ilogb = e - 1
    return 2.0 ** (1 - e)


def flags(qn2, mag, cs, metric, CR):
    with np.errstate(invalid="ignore", over="ignore"):
        long_query = (qn2 > 1.0e8 * CR * CR) if metric == "l2" else np.zeros(len(qn2), bool)
        return ~usable(qn2, mag) | (cs * mag < 1.0e-25) | long_query


def eps_of(mag, M, cs, flagged):
    with np.errstate(invalid="ignore", over="ignore"):
        e = 1.02 * cs * (M + 4) * 2.0 ** -23 * mag
        e = np.where(e < 1.0e37, e, 1.0e37)
        return np.where(flagged, F32(0.0), e.astype(F32) + F32(1.0e-30)).astype(F32)


def B_of(Q, C, lists, metric, cs):
    """float32 (nq, len(lists)): the centroid term of every query against the given lists."""
    Q, C = np.asarray(Q, F32), np.asarray(C, F32)
    bs = (-2.0 if metric == "l2" else -1.0) * cs
    L = len(lists)
    with np.errstate(over="ignore", invalid="ignore"):      # (one chain per (query, list) pair, all pairs side by side)
        acc = _chain(np.repeat(Q, L, axis=0), np.tile(C[np.asarray(lists)], (len(Q), 1)))
        return (bs * acc).astype(F32).reshape(len(Q), L)


def scores(T, codes, n2, B, cs, metric):
    """float32 (nq, n): rows of ONE list (codes (n, M), n2 (n,)), B (nq,) the centroid term of that list."""
    codes = np.asarray(codes)
    nq = T.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        s0 = (F32(cs) * np.asarray(n2, F32)).astype(F32) if metric == "l2" else np.zeros(len(codes), F32)
        s = (np.broadcast_to(s0[None, :], (nq, len(codes))) + np.asarray(B, F32)[:, None]).astype(F32)
        for m in range(codes.shape[1]):
            s = (s + T[:, m, :][:, codes[:, m]]).astype(F32)
    return s


class Batch:
    """Everything the scan computes for one batch on one index: list-order codes / lists given in id order."""

    def __init__(self, Xhat, C, cb, codes, lor, Q, metric):
        self.metric, self.M = metric, cb.shape[0]
        self.Xn2, self.CR, self.handle_ok = handle(Xhat, C, cb)
        self.n2 = n2_of(Xhat)
        self.qn2, self.mag = mags(Q, metric, self.Xn2, self.CR)
        self.cs = cs_of(self.qn2, self.mag)
        self.flag = flags(self.qn2, self.mag, self.cs, metric, self.CR)
        self.eps = eps_of(self.mag, self.M, self.cs, self.flag)
        self.codes, self.lor, self.C, self.cb, self.Q, self.Xhat = np.asarray(codes), np.asarray(lor), C, cb, Q, Xhat
        self._T = None

    @property
    def T(self):
        """float32 (nq, M, 256): the tables, made when first asked for (finite queries only)"""
        if self._T is None:
            self._T = ar.tables(self.cb, self.Q, self.metric, self.cs)
        return self._T

    def all_scores(self):
        """float32 (nq, n) in id order: every row scored with the centroid term of its own list."""
        out = np.empty((len(self.Q), len(self.codes)), F32)
        lists = np.unique(self.lor)
        B = B_of(self.Q, self.C, lists, self.metric, self.cs)
        for j, l in enumerate(lists):
            rows = np.flatnonzero(self.lor == l)
            out[:, rows] = scores(self.T, self.codes[rows], self.n2[rows], B[:, j], self.cs, self.metric)
        return out

    def keys(self):
        """float64 (nq, n): the ideal scaled keys"""
        return ar.exact_scaled_keys(self.Xhat, self.Q, self.metric, self.cs)


def probes_of(C, Q, nprobe, metric):
    """(nq, nprobe) the nprobe nearest lists by plain float64 arithmetic (a coarse near-tie may order two lists the other way: the
    candidate counts this feeds do not hang on one list)."""
    C64, Q64 = np.asarray(C, np.float64), np.asarray(Q, np.float64)
    g = Q64 @ C64.T
    key = -g if metric == "ip" else (C64 * C64).sum(axis=1)[None, :] - 2.0 * g
    return np.argsort(key, axis=1, kind="stable")[:, :nprobe]


def candidate_counts(s, eps, probed_mask, k):
    """(nq,) rows with s <= tau + 2 eps among each query's probed rows (probed_mask (nq, n) bool), tau the k-th smallest of them."""
    s64 = np.where(probed_mask, s.astype(np.float64), np.inf)
    P = probed_mask.sum(axis=1)
    srt = np.sort(s64, axis=1)
    tau = np.where(P >= k, srt[:, min(k, s.shape[1]) - 1], np.inf)
    thr = tau + 2.0 * eps.astype(np.float64)
    return (probed_mask & (s64 <= thr[:, None])).sum(axis=1)


def cand_cap(k, list_cap=0):
    return min(CAND_MAX, list_cap if list_cap > 0 else max(64, 2 * k + 32))


def plan(codec, M, ranges_ok, N, max_list, nq, k, nprobe, force_path=0, ivfpq_adc_max_batch=0, ivfpq_adc_part_rows=0, list_cap=0):
    """ivf_adc_plan: None when the batch is not admitted, else dict(part_rows, parts, stride, cand_cap, lds_bytes)."""
    if codec != 2 or force_path != 0:
        return None
    if nq < 1 or nq > ivfpq_adc_max_batch or nq > MAX_BATCH or k > MAX_K:
        return None
    if M < 1 or M * 1024 + AUX_BYTES > LDS_BUDGET:
        return None
    if not ranges_ok or N <= 0 or max_list <= 0 or nprobe < 1:
        return None
    stride = min(N, nprobe * max_list)
    if nq * stride * 4 > SCORE_BYTES:
        return None
    pairs = nq * nprobe
    part = ivfpq_adc_part_rows if ivfpq_adc_part_rows > 0 else 256 if pairs < 256 else 512 if pairs < 1024 else 1024
    least = ((max_list + MAX_PARTS - 1) // MAX_PARTS + 255) // 256 * 256
    part = max(part, least)
    return dict(part_rows=part, parts=(max_list + part - 1) // part, stride=stride, cand_cap=cand_cap(k, list_cap), lds_bytes=M * 1024)

"""NumPy restatement of the IVF<nlist>,PQ<M> contract of include/vdbhip.h (train-free: centroids and codebooks are injected).
Test infrastructure only: nothing in the product imports it.  The twin of pq_restatement.py, whose float64 argmin it applies
to the residual.

  residual   r[i] = x[i] - c_l, one float32 subtraction per dimension (c_l = centroid of the row's list)
  codes      code[i][m] = argmin over c of the canonical float64 L2 key between r[i][m dsub .. (m + 1) dsub) and
             codebook[m][c] (pq_restatement.l2_keys: acc = fma(t, t, acc), j ascending); ties to the smaller c
  x^         x^[i][d] = c_l[d] + codebook[m][code[i][m]][j], one float32 addition
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import pq_restatement as pq

F32 = np.float32


def residual(x: np.ndarray, centroids: np.ndarray, list_of_row: np.ndarray) -> np.ndarray:
    """float32 (n, D)"""
    x = np.asarray(x, dtype=F32)
    c = np.asarray(centroids, dtype=F32)
    return (x - c[np.asarray(list_of_row)]).astype(F32)


def encode(x: np.ndarray, centroids: np.ndarray, list_of_row: np.ndarray, codebooks: np.ndarray) -> np.ndarray:
    """uint8 (n, M).  The argmin is pq_restatement's (the canonical chain, ties to the smaller c); to keep thousands of rows
    affordable the chain is run only where it can matter: plain float64 sums of squares (every term >= 0, so they are within
    dsub * 2^-51 relative of the chain's keys) name the rows whose smallest key is alone below min * (1 + 1e-9) -- there the argmin
    is already decided -- and the other rows (ties, near-ties) go through pq_restatement.l2_keys."""
    r = residual(x, centroids, list_of_row)
    cb = np.asarray(codebooks, dtype=F32)
    M, _, dsub = cb.shape
    assert r.shape[1] == M * dsub
    out = np.empty((r.shape[0], M), dtype=np.uint8)
    for m in range(M):
        rs = r[:, m * dsub:(m + 1) * dsub]
        rs64, c64 = rs.astype(np.float64), cb[m].astype(np.float64)
        approx = np.zeros((rs.shape[0], 256), dtype=np.float64)
        for j in range(dsub):
            t = rs64[:, j:j + 1] - c64[:, j][None, :]
            approx += t * t
        lo = approx.min(axis=1, keepdims=True)
        out[:, m] = np.argmin(approx, axis=1)
        close = np.flatnonzero((approx <= lo * (1.0 + 1e-9)).sum(axis=1) > 1)
        if len(close):
            out[close, m] = np.argmin(pq.l2_keys(rs[close], cb[m]), axis=1)      # (first minimum: the smaller c keeps a tie)
    return out


def decode(codes: np.ndarray, centroids: np.ndarray, list_of_row: np.ndarray, codebooks: np.ndarray) -> np.ndarray:
    """float32 (n, D): the rows a search scores"""
    c = np.asarray(centroids, dtype=F32)
    return np.ascontiguousarray((c[np.asarray(list_of_row)] + pq.reconstruct(codes, codebooks)).astype(F32))


def encode_bruteforce(x: np.ndarray, centroids: np.ndarray, list_of_row: np.ndarray, codebooks: np.ndarray) -> np.ndarray:
    """The same codes by a plain Python loop: float32 residual, then exact rational arithmetic rounded to float64 once per step
    (tiny cases only)."""
    x = np.asarray(x, dtype=F32)
    c = np.asarray(centroids, dtype=F32)
    cb = np.asarray(codebooks, dtype=F32)
    M, K, dsub = cb.shape
    out = np.zeros((x.shape[0], M), dtype=np.uint8)
    for i in range(x.shape[0]):
        cl = c[list_of_row[i]]
        for m in range(M):
            best, arg = None, 0
            for k in range(K):
                acc = 0.0
                for j in range(dsub):
                    r = F32(x[i, m * dsub + j]) - F32(cl[m * dsub + j])          # float32, rounded once
                    t = float(np.float64(r) - np.float64(cb[m, k, j]))
                    acc = float(Fraction(t) * Fraction(t) + Fraction(acc))
                if best is None or acc < best:
                    best, arg = acc, k
            out[i, m] = arg
    return out


def decode_bruteforce(codes: np.ndarray, centroids: np.ndarray, list_of_row: np.ndarray, codebooks: np.ndarray) -> np.ndarray:
    c = np.asarray(centroids, dtype=F32)
    cb = np.asarray(codebooks, dtype=F32)
    M, _, dsub = cb.shape
    out = np.zeros((len(codes), M * dsub), dtype=F32)
    for i in range(len(codes)):
        for m in range(M):
            for j in range(dsub):
                out[i, m * dsub + j] = F32(c[list_of_row[i], m * dsub + j]) + F32(cb[m, codes[i, m], j])
    return out

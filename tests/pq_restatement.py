"""NumPy restatement of the PQ<M> contract of include/vdbhip.h (codes, reconstruction).  Test infrastructure only: nothing in
the product imports it.

  codebooks  float32 (M, 256, dsub), dsub = D / M
  codes      code[i][m] = argmin over c of  acc_c = sum_j fma(t, t, acc), t = float64(x[i][m dsub + j]) - float64(cb[m][c][j]),
             j ascending from acc = 0.0; ties to the smaller c.  t is exact in float64 for float32 inputs of ordinary range and
             t * t is rounded once before the add in NumPy, whereas fma rounds once in all: the two differ only when t * t is
             inexact in float64, so the restatement carries the product in two exact halves (Dekker) and adds them in the one
             rounding an fma makes -- see `_fma_sq_add`.
  x^         x^[i] = cb[0][code[i][0]] ++ ... ++ cb[M-1][code[i][M-1]], a pure lookup
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def _fma_sq_add(t: np.ndarray, acc: np.ndarray) -> np.ndarray:
    """fma(t, t, acc) element-wise in float64, correctly rounded.  t * t = hi + lo exactly (Veltkamp / Dekker split); the sum
    acc + hi + lo is then rounded once: s = acc + hi with its exact error e (two-sum), and the result is s + (e + lo), which is
    the correctly rounded value whenever e + lo is exact: s + (e + lo) is then ONE rounding of acc + t * t.  Whether it is
    exact is read from the error term of a second two-sum; an element where it is not is recomputed in exact rational
    arithmetic."""
    t = np.asarray(t, dtype=np.float64)
    acc = np.asarray(acc, dtype=np.float64)
    c = 134217729.0 * t                      # 2^27 + 1
    th = c - (c - t)
    tl = t - th
    hi = t * t
    lo = ((th * th - hi) + 2.0 * th * tl) + tl * tl
    s = acc + hi
    bb = s - acc
    e = (acc - (s - bb)) + (hi - bb)
    r = s + (e + lo)
    # certify: exact recomputation where the cheap path is not provably the single rounding
    tail = e + lo
    tb = tail - e
    doubtful = ((e - (tail - tb)) + (lo - tb)) != 0.0        # (two-sum: the error of e + lo)
    if np.any(doubtful):
        idx = np.flatnonzero(doubtful)
        tf, af, rf = t.ravel(), acc.ravel(), r.ravel().copy()
        for i in idx:
            rf[i] = float(Fraction(float(tf[i])) * Fraction(float(tf[i])) + Fraction(float(af[i])))
        r = rf.reshape(r.shape)
    return r


def l2_keys(xs: np.ndarray, cents: np.ndarray) -> np.ndarray:
    """float64 (n, 256): canonical L2 keys of the sub-vectors xs (n, dsub) against cents (256, dsub)"""
    xs64 = np.asarray(xs, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(cents, dtype=np.float32).astype(np.float64)
    acc = np.zeros((xs64.shape[0], c64.shape[0]), dtype=np.float64)
    for j in range(xs64.shape[1]):           # j ascending, one rounding per step
        acc = _fma_sq_add(xs64[:, j:j + 1] - c64[:, j][None, :], acc)
    return acc


def encode(x: np.ndarray, codebooks: np.ndarray, block: int = 4096) -> np.ndarray:
    """uint8 (n, M)"""
    x = np.asarray(x, dtype=np.float32)
    cb = np.asarray(codebooks, dtype=np.float32)
    M, _, dsub = cb.shape
    assert x.shape[1] == M * dsub
    out = np.empty((x.shape[0], M), dtype=np.uint8)
    for r0 in range(0, x.shape[0], block):
        for m in range(M):
            keys = l2_keys(x[r0:r0 + block, m * dsub:(m + 1) * dsub], cb[m])
            out[r0:r0 + block, m] = np.argmin(keys, axis=1)      # (first minimum: the smaller c keeps a tie)
    return out


def reconstruct(codes: np.ndarray, codebooks: np.ndarray) -> np.ndarray:
    """float32 (n, D)"""
    cb = np.asarray(codebooks, dtype=np.float32)
    codes = np.asarray(codes)
    return np.ascontiguousarray(np.concatenate([cb[m][codes[:, m]] for m in range(cb.shape[0])], axis=1), dtype=np.float32)


def encode_bruteforce(x: np.ndarray, codebooks: np.ndarray) -> np.ndarray:
    """The same codes by a plain Python loop in exact rational arithmetic, rounded to float64 once per step (tiny cases only)."""
    x = np.asarray(x, dtype=np.float32)
    cb = np.asarray(codebooks, dtype=np.float32)
    M, K, dsub = cb.shape
    out = np.zeros((x.shape[0], M), dtype=np.uint8)
    for i in range(x.shape[0]):
        for m in range(M):
            best, arg = None, 0
            for c in range(K):
                acc = 0.0
                for j in range(dsub):
                    t = float(np.float64(x[i, m * dsub + j]) - np.float64(cb[m, c, j]))
                    acc = float(Fraction(t) * Fraction(t) + Fraction(acc))
                if best is None or acc < best:
                    best, arg = acc, c
            out[i, m] = arg
    return out

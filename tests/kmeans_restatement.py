"""NumPy restatement of the k-means training contract of include/vdbhip.h (vdb_ivf_train, vdb_pq_train, vdb_ivfpq_train), plus a
pure-Python mt19937_64.  Test infrastructure only: nothing in the product imports it.

  sample     pick = 0 .. n-1; for i < min(ns, n - 1): j = i + rng() % (n - i), swap pick[i], pick[j]; the sample is pick[:ns]
  init       the first nlist sample rows
  assign     injected: assign(C, S, metric) -> list of every sample row (the tests pass oracle.c_oracle.ivf_assign)
  update     non-empty list: float64 sum of its rows in sample order, ONE rounding per add (np.cumsum along the rows, never sum or
             mean), divided by the count, rounded to float32; an empty list keeps its centroid
  spherical  (IP) n2 = sum over the 64-dimension blocks, in order, of the butterfly sum of (double)(float)m squared; n2 > 0:
             centroid *= (float)(1 / sqrt(n2)) as a float32 product
  split      after the update, for every empty list in ascending order: halve the first largest list (+-1/1024, float32)
"""
from __future__ import annotations

from typing import Callable, Tuple

import numpy as np

F32 = np.float32
MASK64 = (1 << 64) - 1


class MT19937_64:
    """std::mt19937_64: the 64-bit Mersenne Twister of Matsumoto and Nishimura, seeded as the C++ standard seeds it."""

    NN, MM = 312, 156
    MATRIX_A, UPPER, LOWER = 0xB5026F5AA96619E9, 0xFFFFFFFF80000000, 0x7FFFFFFF

    def __init__(self, seed: int = 5489):
        mt = [int(seed) & MASK64]
        for i in range(1, self.NN):
            mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & MASK64)
        self.mt, self.at = mt, self.NN

    def _twist(self) -> None:
        mt, nn, mm = self.mt, self.NN, self.MM
        for i in range(nn):
            x = (mt[i] & self.UPPER) | (mt[(i + 1) % nn] & self.LOWER)
            mt[i] = mt[(i + mm) % nn] ^ (x >> 1) ^ (self.MATRIX_A if x & 1 else 0)
        self.at = 0

    def __call__(self) -> int:
        if self.at >= self.NN:
            self._twist()
        x = self.mt[self.at]
        self.at += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEFB00000000
        x ^= x >> 43
        return x & MASK64


def sample_rows(n: int, ns: int, seed: int) -> np.ndarray:
    """int64 (n): a permutation of 0 .. n-1 whose first ns entries are the sample, in draw order (sample_rows of the library)."""
    pick = list(range(n))
    rng = MT19937_64(seed)
    for i in range(min(ns, n - 1)):
        j = i + rng() % (n - i)
        pick[i], pick[j] = pick[j], pick[i]
    return np.array(pick, np.int64)


def list_mean(rows: np.ndarray) -> np.ndarray:
    """float32 (D): the float64 sum of the float32 rows in the order given, one rounding per add, over the count."""
    acc = np.cumsum(rows.astype(np.float64), axis=0)[-1]
    return (acc / np.float64(rows.shape[0])).astype(F32)


def butterfly_sum(v: np.ndarray) -> np.float64:
    """Sum of 64 float64 lanes as the xor-shuffle reduction adds them: v = v[:w] + v[w:2w] for w = 32, 16, .., 1."""
    v = np.asarray(v, np.float64)
    assert v.shape == (64,)
    w = 32
    while w:
        v = v[:w] + v[w:2 * w]
        w >>= 1
    return v[0]


def squared_norm(m32: np.ndarray) -> np.float64:
    """n2 of one float32 centroid: the butterfly sums of its squares per 64-dimension block, added in block order."""
    D = m32.shape[0]
    sq = np.zeros(-(-D // 64) * 64, np.float64)
    sq[:D] = m32.astype(np.float64) * m32.astype(np.float64)
    n2 = np.float64(0.0)
    for d0 in range(0, D, 64):
        n2 = n2 + butterfly_sum(sq[d0:d0 + 64])
    return n2


def normalize(m32: np.ndarray) -> np.ndarray:
    n2 = squared_norm(m32)
    if not n2 > 0.0:
        return m32
    inv = F32(np.float64(1.0) / np.sqrt(n2))
    return (m32 * inv).astype(F32)


def split_empty(cent: np.ndarray, cnt) -> int:
    """The empty-cell rule, in place on cent (float32 (nlist, D)) and cnt (int64 (nlist)); returns the number of splits."""
    nlist, D = cent.shape
    e = np.where(np.arange(D) & 1, F32(1.0) / F32(1024.0), -F32(1.0) / F32(1024.0)).astype(F32)
    up, down = (F32(1.0) + e).astype(F32), (F32(1.0) - e).astype(F32)
    splits = 0
    for l in range(nlist):
        if cnt[l] != 0:
            continue
        big = int(np.argmax(cnt))                                    # the first index holding the maximum
        c = cent[big].copy()
        cent[l] = c * up
        cent[big] = c * down
        cnt[l] = cnt[big] // 2
        cnt[big] -= cnt[l]
        splits += 1
    return splits


def kmeans(X: np.ndarray, nlist: int, niter: int, seed: int, mpc: int, metric: str,
           assign: Callable[[np.ndarray, np.ndarray, str], np.ndarray]) -> Tuple[np.ndarray, int, np.ndarray]:
    """(centroids float32 (nlist, D), splits over all iterations, list sizes int64 (nlist) of the last assignment)."""
    X = np.ascontiguousarray(X, dtype=F32)
    n, D = X.shape
    mpc = 256 if mpc <= 0 else mpc
    ns = min(n, mpc * nlist)
    S = np.ascontiguousarray(X[sample_rows(n, ns, seed)[:ns]])
    cent = S[:nlist].copy()
    splits, sizes = 0, np.zeros(nlist, np.int64)
    for _ in range(niter):
        lor = np.asarray(assign(cent, S, metric), dtype=np.int64)
        assert lor.shape == (ns,) and lor.min() >= 0 and lor.max() < nlist
        order = np.argsort(lor, kind="stable")                       # rows stay in sample order within a list
        sizes = np.bincount(lor, minlength=nlist).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        for c in np.nonzero(sizes)[0]:
            m32 = list_mean(S[order[off[c]:off[c + 1]]])
            cent[c] = normalize(m32) if metric == "ip" else m32
        splits += split_empty(cent, sizes.copy())
    return cent, splits, sizes


def _sub_codebooks(S: np.ndarray, M: int, niter: int, seed: int, mpc: int, assign):
    D = S.shape[1]
    dsub = D // M
    cb = np.empty((M, 256, dsub), F32)
    splits = []
    for m in range(M):
        sub = np.ascontiguousarray(S[:, m * dsub:(m + 1) * dsub])
        cb[m], s, _ = kmeans(sub, 256, niter, (seed + m) & MASK64, mpc, "l2", assign)
        splits.append(s)
    return cb, splits


def pq_codebooks(X: np.ndarray, M: int, niter: int, seed: int, mpc: int, assign):
    """(codebooks float32 (M, 256, dsub), splits per sub-space) of vdb_pq_train."""
    X = np.ascontiguousarray(X, dtype=F32)
    mpc = 256 if mpc <= 0 else mpc
    n = X.shape[0]
    ns = min(n, 256 * mpc)
    return _sub_codebooks(X[sample_rows(n, ns, seed)[:ns]], M, niter, seed, mpc, assign)


def ivfpq_codebooks(X: np.ndarray, C: np.ndarray, M: int, niter: int, seed: int, mpc: int, metric: str, assign):
    """(codebooks, splits per sub-space) of vdb_ivfpq_train against the installed centroids C under the index metric."""
    X, C = np.ascontiguousarray(X, dtype=F32), np.ascontiguousarray(C, dtype=F32)
    mpc = 256 if mpc <= 0 else mpc
    n = X.shape[0]
    ns = min(n, 256 * mpc)
    S = np.ascontiguousarray(X[sample_rows(n, ns, seed)[:ns]])
    R = (S - C[np.asarray(assign(C, S, metric), dtype=np.int64)]).astype(F32)
    return _sub_codebooks(R, M, niter, seed, mpc, assign)

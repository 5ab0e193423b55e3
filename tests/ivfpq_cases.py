"""Inputs shared by tests/test_ivf_pq_host.py and tests/test_gpu_ivf_pq.py (test infrastructure only).

`parity_inputs`   clustered rows, 24 injected centroids and random codebooks for the code / search parity shapes.
`near_tie_inputs` an IVF-PQ index on which the exactness guard decides the answer: four injected centroids
                  (guard_cases.ivf_centroids), codebooks of near-copy centroid families and codes whose k + 1 replicas per base
                  row differ by one family member per sub-space (guard_cases.make_pq_clusters), every replica of a base row in
                  the same list, blocked layout (every replica in another bin: each is a bin minimum).  The decoded rows x^ of
                  the replicas differ by less than the fp16 resolution of the scan; some replicas are made exact duplicates
                  (identical codes, same list: ties by id).  The queries sit next to the decoded base rows.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import guard_cases as gc
import ivfpq_restatement as ref

F32 = np.float32
PARITY_SHAPES = ((50, 50), (64, 8), (128, 64), (384, 64))      # (D, M): dsub 1, 8, 2, 6; D4 padding at 50; D > 128
PARITY_ROWS, PARITY_LISTS = 6000, 24
NEAR_TIE_NB, NEAR_TIE_K, NEAR_TIE_D, NEAR_TIE_M, NEAR_TIE_NQ = 8192, 4, 64, 16, 256


@lru_cache(maxsize=8)
def parity_inputs(d, M, nq=320, seed=0):
    """(X, Q, C, codebooks): rows around 24 centres, centroids drawn from the rows, codebooks of the residuals' scale with two
    equal entries per sub-space (a tie for the smaller c) -- all float32, read-only."""
    rng = np.random.default_rng(seed + 1000 * d + M)
    centers = rng.standard_normal((PARITY_LISTS, d)).astype(F32) * 3
    X = (centers[rng.integers(0, PARITY_LISTS, PARITY_ROWS)] + rng.standard_normal((PARITY_ROWS, d))).astype(F32)
    Q = (centers[rng.integers(0, PARITY_LISTS, nq)] + rng.standard_normal((nq, d))).astype(F32)
    C = X[rng.choice(PARITY_ROWS, PARITY_LISTS, replace=False)].copy()
    cb = (rng.standard_normal((M, 256, d // M)) * 1.2).astype(F32)
    cb[:, 200] = cb[:, 17]
    X[40:60] = X[0:20]                                           # duplicated rows: equal codes wherever they share a list
    for a in (X, Q, C, cb):
        a.flags.writeable = False
    return X, Q, C, cb


@lru_cache(maxsize=2)
def near_tie_inputs(metric, seed=11):
    """dict(C, cb, codes, lor, Q, Xhat, k): see the module docstring."""
    nb, k, d, M = NEAR_TIE_NB, NEAR_TIE_K, NEAR_TIE_D, NEAR_TIE_M
    cb, codes, _ = gc.make_pq_clusters(nb, k, NEAR_TIE_NQ, seed, "blocked", d=d, M=M, rel=gc.REL if metric == "l2" else 1e-4)
    codes = codes.copy()
    codes[nb:nb + 64] = codes[0:64]                              # replica 1 of base rows 0 .. 63: an exact duplicate of replica 0
    C = gc.ivf_centroids(d)
    lor = np.tile((np.arange(nb) % 4).astype(np.int32), k + 1)   # every replica of base row i in list i % 4
    Xhat = ref.decode(codes, C, lor, cb)
    rng = np.random.default_rng(seed + 1)
    pick = np.concatenate([np.arange(32), 64 + rng.choice(nb - 64, NEAR_TIE_NQ - 32, replace=False)])   # (32 queries at duplicated rows)
    Q = (Xhat[pick].astype(np.float64) + 0.05 * rng.standard_normal((NEAR_TIE_NQ, d))).astype(F32)
    out = dict(C=C, cb=cb, codes=codes, lor=lor, Q=Q, Xhat=Xhat, k=k)
    for a in (codes, lor, Q, Xhat):
        a.flags.writeable = False
    return out

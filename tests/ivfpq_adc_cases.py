"""Inputs shared by tests/test_ivfpq_adc_host.py and tests/test_gpu_ivfpq_adc.py (test infrastructure only).

`shape_case(d, M)`   the parity corpus of ivfpq_cases (6000 rows, 24 lists) with 512 queries, its lists, restated codes and decoded rows
`family(kind, M)`    a small index whose values come from one of KINDS: the six families the bound is held on, and two more inside the
                     range a handle is admitted in ("small", "large": "tiny" and "huge" are refused by the admission rule)
`census_case()`      lists of 0, 1, 255, 256, 257, 511, 513 and about 1900 rows: every part, list and 256-row boundary
"""
from __future__ import annotations

from functools import lru_cache

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))      # (ivfpq_cases imports its neighbours by their bare names)

from tests import ivfpq_cases as cases  # noqa: E402
from tests import ivfpq_restatement as ref  # noqa: E402

F32 = np.float32
SHAPES = cases.PARITY_SHAPES + ((80, 20),)        # (80, 20): 16 + 4 codes, the remainder of the dword path
KINDS = ("gauss", "unit", "ints", "tiny", "huge", "offset", "small", "large")
SCALE = {"tiny": 1e-20, "huge": 1e18, "small": 1e-12, "large": 1e12}
FAMILY_ROWS, FAMILY_LISTS, FAMILY_NQ = 3000, 8, 64
CENSUS_LISTS = (0, 1, 255, 256, 257, 511, 513, 1900)
SEARCH_NPROBE, SEARCH_K, SEARCH_NQ = (1, 4, cases.PARITY_LISTS), (1, 10, 100, 1024), (1, 8, 9, 300, 512)


def assign(C, X, metric):
    from oracle import c_oracle

    return c_oracle.ivf_assign(C, X, metric)


@lru_cache(maxsize=12)
def shape_case(d, M, metric):
    """dict(X, Q, C, cb, lor, codes, Xhat)"""
    X, Q, C, cb = cases.parity_inputs(d, M, nq=512)
    lor = assign(C, X, metric)
    codes = ref.encode(X, C, lor, cb)
    return dict(X=X, Q=Q, C=C, cb=cb, lor=lor, codes=codes, Xhat=ref.decode(codes, C, lor, cb))


@lru_cache(maxsize=64)
def family(kind, M, seed=0):
    """dict(C, cb, codes, lor, Q, Xhat): random codes under random lists (the decoded rows are the corpus)."""
    d = 100 if M == 50 else 64
    dsub = d // M
    rng = np.random.default_rng(1000 * M + len(kind) + seed)
    n, nlist, nq = FAMILY_ROWS, FAMILY_LISTS, FAMILY_NQ
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    lor = rng.integers(0, nlist, size=n).astype(np.int32)
    if kind == "unit":          # rows of norm about 1: unit centroids scaled by 0.8, residuals of norm 0.6
        C = rng.standard_normal((nlist, d))
        C *= 0.8 / np.linalg.norm(C, axis=1, keepdims=True)
        cb = rng.standard_normal((M, 256, dsub))
        cb *= 0.6 / (np.linalg.norm(cb, axis=2, keepdims=True) * np.sqrt(M))
    elif kind == "ints":        # SIFT-like: integer centroids and integer residuals
        C = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(nlist, d))), 0, 218)
        cb = np.rint(rng.standard_normal((M, 256, dsub)) * 12.0)
    elif kind == "offset":      # centroids of norm about 1000 x the residuals
        C = rng.standard_normal((nlist, d)) * (1000.0 / np.sqrt(d))
        cb = rng.standard_normal((M, 256, dsub)) / np.sqrt(d)
    else:
        s = SCALE.get(kind, 1.0)
        C = rng.standard_normal((nlist, d)) * (3.0 * s)
        cb = rng.standard_normal((M, 256, dsub)) * s
    C, cb = np.ascontiguousarray(C, F32), np.ascontiguousarray(cb, F32)
    Xhat = ref.decode(codes, C, lor, cb)
    pick = rng.choice(n, nq, replace=False)
    with np.errstate(over="ignore"):
        spread = float(np.sqrt(np.mean(cb.astype(np.float64) ** 2)))
        Q = (Xhat[pick].astype(np.float64) + spread * rng.standard_normal((nq, d))).astype(F32)
    if kind == "unit":
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    elif kind == "ints":
        Q = np.rint(Q)
    Q[1] *= F32(1.0e-3)         # a query far below the batch's largest
    Q = np.ascontiguousarray(Q, F32)
    for a in (C, cb, codes, lor, Q, Xhat):
        a.flags.writeable = False
    return dict(C=C, cb=cb, codes=codes, lor=lor, Q=Q, Xhat=Xhat, d=d, M=M)


@lru_cache(maxsize=2)
def census_case(metric, d=64, M=16, seed=5):
    """dict(X, C, cb, lor, codes, Xhat): rows around their list's centroid, the lists' lengths CENSUS_LISTS (the first list is empty),
    filed in an order that interleaves the lists."""
    rng = np.random.default_rng(seed)
    nlist = len(CENSUS_LISTS)
    C = (rng.standard_normal((nlist, d)) * 3).astype(F32)
    lor = rng.permutation(np.repeat(np.arange(nlist), CENSUS_LISTS)).astype(np.int32)
    X = (C[lor] + rng.standard_normal((len(lor), d))).astype(F32)
    cb = (rng.standard_normal((M, 256, d // M)) * 1.2).astype(F32)
    codes = ref.encode(X, C, lor, cb)
    return dict(X=X, C=C, cb=cb, lor=lor, codes=codes, Xhat=ref.decode(codes, C, lor, cb), d=d, M=M)

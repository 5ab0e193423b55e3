"""Shapes, masks and the reference of the filtered k-NN search (vdb_filter_set / vdb_search_filtered), shared by
tests/test_filter_host.py and tests/test_gpu_filter.py.

Reference: the oracle's k-NN over the ADMITTED rows only -- X[rows], k' = min(k, len(rows)) -- with the ids mapped back through the
ascending row list plus id_base and padded to k by the convention of vdb_search (-1, +FLT_MAX under L2 / -FLT_MAX under IP).  The key
of a row does not depend on the other rows and an ascending map keeps (key, id) order, so this is the contract restated.

Shapes are the smallest that reach each route of search_batch; `force` is option "force_path" (2 where the pair-count gate would
send a corpus below 32 768 rows to the exact kernels).  NumPy only."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Tuple

import numpy as np

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)


@dataclass(frozen=True)
class Route:
    name: str
    n: int
    d: int
    kind: str = "gauss"            # rows: "gauss" | "bytes" (integers 0..255)
    qkind: str = "gauss"           # queries: "gauss" | "bytes" (integer batch in the byte window) | "bytes+" (one non-integer value)
    opts: Tuple[Tuple[str, float], ...] = ()
    force: int = 2
    scan_shape: int = 16           # vdb_stats.scan_shape after the add
    scan_dtype: int = 0            # ... and scan_dtype after a masked scan
    nqs: Tuple[int, ...] = (1, 5, 64, 513)
    span: int = 512                # rows per span of the scan copies

    @property
    def id(self):
        return self.name


ROUTES = (
    Route("x16-f16", 20000, 32),
    Route("x16-i8", 20000, 32, "bytes", "bytes", scan_dtype=1),
    Route("x16-pair-f16", 20000, 32, "bytes", "bytes+"),
    Route("x16-i8only", 33000, 32, "bytes", "bytes", opts=(("int8_only", 1),), scan_dtype=1, nqs=(1, 5, 64)),
    Route("x16-i8only-f16", 33000, 32, "bytes", "bytes+", opts=(("int8_only", 1),), nqs=(5, 64)),
    Route("s32-small", 9000, 24, scan_shape=32, nqs=(1, 5, 64)),
    Route("s32-forced", 20000, 32, opts=(("flat_shape", 32),), scan_shape=32),
    Route("p16-kloop", 4100, 136, scan_shape=0, nqs=(1, 5, 64), span=1024),
    Route("p16-streamed", 4100, 136, opts=(("stream_panels", 1),), scan_shape=0, nqs=(1, 5, 64), span=1024),
    Route("dense", 3000, 16, force=0, scan_shape=32, nqs=(64, 5)),
    Route("exact-small", 300, 7, force=0, scan_shape=32, nqs=(1, 5, 64)),
    Route("exact-forced", 20000, 32, force=1, nqs=(1, 5, 64)),
)
SCAN_ROUTES = tuple(r for r in ROUTES if r.force == 2)
KS = (1, 10, 100)
ID_BASES = (0, 1_000_003)


@lru_cache(maxsize=None)
def corpus(r: Route):
    rng = np.random.default_rng([41, r.n, r.d, r.kind == "bytes"])
    if r.kind == "bytes":
        X = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(r.n, r.d))), 0, 255).astype(F32)
    else:
        X = rng.standard_normal((r.n, r.d)).astype(F32)
    X.flags.writeable = False
    return X


@lru_cache(maxsize=None)
def queries(r: Route, nq: int = 513):
    rng = np.random.default_rng([43, r.n, r.d, len(r.qkind)])
    if r.qkind.startswith("bytes"):
        Q = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(nq, r.d))), 0, 255).astype(F32)
        if r.qkind == "bytes+":
            Q[0, 0] += F32(0.5)              # one non-integer value: the device puts the whole batch on the fp16 scan
    else:
        Q = rng.standard_normal((nq, r.d)).astype(F32)
    Q.flags.writeable = False
    return Q


def masks(n: int, k: int, span: int = 512):
    """name -> bool mask (n,), read-only; `k` places the k - 1 / k / k + 1 masks"""
    rng = np.random.default_rng([47, n, k])
    out = {}

    def put(name, rows=None, cleared=None):
        m = np.zeros(n, np.bool_) if cleared is None else np.ones(n, np.bool_)
        m[np.asarray(rows if cleared is None else cleared, np.int64)] = cleared is None
        m.flags.writeable = False
        out[name] = m

    put("all-ones", cleared=[])
    put("all-zeros", rows=[])
    put("row-0", rows=[0])
    put("row-last", rows=[n - 1])
    put("word-edges", rows=[31, 32, 63, 64])
    put("alternating", rows=np.arange(0, n, 2))
    put("bin-cleared", cleared=np.arange(256, 512) if n >= 512 else np.arange(n // 2, n))     # (fewer rows than two bins: the upper half)
    c0 = min(8192, n // 2 // span * span)
    put("chunk-cleared", cleared=np.arange(c0, min(n, 2 * c0)) if c0 else np.arange(0, n // 2))
    put("last-span-only", rows=np.arange((n - 1) // span * span, n))
    for dens in (0.5, 0.1, 0.01):
        put(f"random-{dens}", rows=np.flatnonzero(rng.random(n) < dens))
    for m in (k - 1, k, k + 1):
        put(f"admits-{m - k:+d}", rows=rng.choice(n, min(m, n), replace=False))
    return out


def tail_set_words(mask: np.ndarray) -> np.ndarray:
    """the mask packed by hand, with every bit of the last word beyond n SET (the library must ignore them)"""
    n = len(mask)
    words = np.zeros((n + 31) // 32, np.uint32)
    rows = np.flatnonzero(mask)
    np.bitwise_or.at(words, rows // 32, (np.uint32(1) << (rows % 32).astype(np.uint32)))
    if n % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return words


def pad_value(metric: str):
    return FLT_MAX if metric == "l2" else -FLT_MAX


def reference(knn, X, Q, k: int, metric: str, mask: np.ndarray, id_base: int = 0):
    """(D (nq, k) float32, I (nq, k) int64) of the contract; knn(X, Q, k, metric) -> (D, I) is the oracle's exhaustive search"""
    rows = np.flatnonzero(mask).astype(np.int64)
    nq = len(Q)
    D = np.full((nq, k), pad_value(metric), F32)
    I = np.full((nq, k), -1, np.int64)
    kk = min(k, len(rows))
    if kk:
        d, i = knn(np.ascontiguousarray(X[rows]), Q, kk, metric)
        D[:, :kk] = d
        I[:, :kk] = np.where(i >= 0, rows[np.maximum(i, 0)] + id_base, -1)
    return D, I


def brute_reference(X, Q, k: int, metric: str, mask: np.ndarray, id_base: int = 0):
    """the same contract from a masked argsort over float64 keys made with NumPy: stable sort = ties by ascending id"""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    nq, n = len(Q), len(X)
    keys = np.empty((nq, n))
    for q in range(nq):                         # d ascending, one fused step each: the canonical chain
        acc = np.zeros(n)
        for d in range(X.shape[1]):
            if metric == "l2":
                t = X64[:, d] - Q64[q, d]
                acc = t * t + acc
            else:
                acc = Q64[q, d] * X64[:, d] + acc
        keys[q] = acc if metric == "l2" else -acc
    rows = np.flatnonzero(mask)
    D = np.full((nq, k), pad_value(metric), F32)
    I = np.full((nq, k), -1, np.int64)
    kk = min(k, len(rows))
    if kk:
        order = np.argsort(keys[:, rows], axis=1, kind="stable")[:, :kk]
        I[:, :kk] = rows[order] + id_base
        kd = np.take_along_axis(keys[:, rows], order, axis=1)
        D[:, :kk] = (kd if metric == "l2" else -kd).astype(F32)
    return D, I


def expected_path(r: Route, nq: int, k: int, n_allowed: int):
    """vdb_stats.last_path_name of a filtered search with option "filter_sparse_pairs" = 0 (filter_plan.hpp, search_batch); None: the
    path vdb_search takes for the same batch on the same handle (force_path 2: the scan wherever its geometry serves k)"""
    if r.force == 0 and n_allowed < 2 * k + 64:
        return "filter_rows"
    if r.force == 1:
        return "exact_scan"
    if r.force == 2:
        return None
    return "mfma_scan" if nq >= 64 and 2 * k <= n_allowed and k <= 1024 else "exact_scan"       # (the dense path reports mfma_scan)

"""Shapes, masks and the reference of the filtered k-NN search on IVF-Flat indexes (vdb_ivf_filter_set / vdb_ivf_search_filtered;
DESIGN 4.15), shared by tests/test_ivf_filter_host.py and tests/test_gpu_ivf_filter.py.

Reference: the oracle's IVF search over the ADMITTED rows only -- ivf_search(X[rows], C, lor[rows], Q, k, nprobe, metric) -- with the
ids mapped back through the ascending row list plus id_base.  The coarse choice depends on C and Q only, the key of a row does not
depend on the other rows and an ascending subset keeps (key, id) order inside every list, so this is the contract restated.

Shapes are those of tests/test_gpu_ivf_paths.py and tests/test_gpu_ivf.py: the smallest at which each launch family of the list scans
still runs.  NumPy only."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Tuple

import numpy as np

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
ID_BASES = (0, 1_000_003)
KS = (1, 10, 100)


@dataclass(frozen=True)
class Shape:
    name: str
    n: int
    d: int
    nlist: int
    kind: str = "gauss"            # rows: "gauss" | "bytes" (integers 0..255)
    qkind: str = "float"           # "float" | "int" (bytes rows only: an integer batch, which the device puts on the int8 list scan)
    metrics: Tuple[str, ...] = ("l2", "ip")
    nprobes: Tuple[int, ...] = (8, 16)
    nq: int = 300
    tps: int = 0                   # option "ivf_tps" before the add (D > 128)
    first_centroids: bool = True   # centroids = the first nlist rows, else a seeded choice of rows
    scan_dtype: int = 0            # vdb_stats.scan_dtype after a list-major search

    @property
    def id(self):
        return self.name


SHAPES = (
    Shape("f16-d64", 20000, 64, 64),
    Shape("f16-d128", 20000, 128, 64),
    Shape("i8-d64-int", 20000, 64, 64, "bytes", "int", scan_dtype=1),
    Shape("i8-d128-int", 20000, 128, 64, "bytes", "int", scan_dtype=1),
    Shape("i8-d64-float", 20000, 64, 64, "bytes", "float"),
    Shape("kloop-d200", 30000, 200, 64, metrics=("l2",), nprobes=(8,), first_centroids=False),
    Shape("kloop-d256-tps64", 60000, 256, 16, metrics=("ip",), nprobes=(4,), nq=200, tps=64, first_centroids=False),
    Shape("kloop-d256-tps16", 60000, 256, 16, metrics=("ip",), nprobes=(16,), nq=200, tps=16, first_centroids=False),
)


def _bytes(rng, n, d):
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(F32)


@lru_cache(maxsize=3)
def data(s: Shape):
    """(X, C, Q), read-only"""
    rng = np.random.default_rng([53, s.n, s.d, s.kind == "bytes", s.qkind == "int"])
    if s.kind == "bytes":
        X, Q = _bytes(rng, s.n, s.d), _bytes(rng, s.nq, s.d)
        if s.qkind == "float":
            Q = Q + 3 * rng.standard_normal((s.nq, s.d)).astype(F32)
    else:
        X, Q = rng.standard_normal((s.n, s.d)).astype(F32), rng.standard_normal((s.nq, s.d)).astype(F32)
    C = X[:s.nlist].copy() if s.first_centroids else X[np.sort(rng.choice(s.n, s.nlist, replace=False))].copy()
    for a in (X, C, Q):
        a.flags.writeable = False
    return X, C, Q


def host_assign(C, X, metric):
    """nearest centroid in float64 (ties: the lower list) -- for the host tests only; GPU tests read the index's own assignment()"""
    C64, X64 = C.astype(np.float64), X.astype(np.float64)
    key = -(X64 @ C64.T) if metric == "ip" else (C64 * C64).sum(1)[None, :] - 2.0 * (X64 @ C64.T)
    return np.argmin(key, axis=1).astype(np.int32)


def nearest_lists(C, q, metric, m):
    """the m lists nearest to one query, float64"""
    C64, q64 = C.astype(np.float64), q.astype(np.float64)
    key = -(C64 @ q64) if metric == "ip" else ((C64 - q64) ** 2).sum(1)
    return np.argsort(key, kind="stable")[:m]


def list_order(lor):
    """(perm, offsets): perm[j] = insertion-order row of list-order row j (stable by list), offsets[l] = first list-order row of list l"""
    perm = np.argsort(lor, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(lor, minlength=int(lor.max()) + 1))])
    return perm, offsets


def masks(n: int, lor: np.ndarray, probed: np.ndarray):
    """name -> bool mask (n,) over rows in INSERTION order, read-only.  `probed`: three lists some query probes."""
    rng = np.random.default_rng([59, n])
    out = {}

    def put(name, rows=None, cleared=None):
        m = np.zeros(n, np.bool_) if cleared is None else np.ones(n, np.bool_)
        m[np.asarray(rows if cleared is None else cleared, np.int64)] = cleared is None
        m.flags.writeable = False
        out[name] = m

    put("all-ones", cleared=[])
    put("all-zeros", rows=[])
    for dens in (0.5, 0.1, 0.01):
        put(f"random-{dens}", rows=np.flatnonzero(rng.random(n) < dens))
    put("id-run", rows=np.arange(n // 3, n // 3 + n // 10))
    put("three-lists-cleared", cleared=np.flatnonzero(np.isin(lor, probed)))
    put("one-list-only", rows=np.flatnonzero(lor == probed[0]))
    put("single-row", rows=[int(np.flatnonzero(lor == probed[0])[0])])
    put("last-row", rows=[n - 1])
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


def reference(ivf_search, X, C, lor, Q, k: int, nprobe: int, metric: str, mask: np.ndarray, id_base: int = 0):
    """(D (nq, k) float32, I (nq, k) int64) of the contract; ivf_search is the oracle's (X, C, list_of_row, Q, k, nprobe, metric)"""
    rows = np.flatnonzero(mask).astype(np.int64)
    if len(rows) == 0:
        return np.full((len(Q), k), pad_value(metric), F32), np.full((len(Q), k), -1, np.int64)
    d, i = ivf_search(np.ascontiguousarray(X[rows]), C, np.ascontiguousarray(lor[rows]), Q, k, nprobe, metric)
    return np.ascontiguousarray(d, F32), np.where(i >= 0, rows[np.maximum(i, 0)] + id_base, -1).astype(np.int64)


def brute_reference(pair_keys, X, C, lor, Q, k: int, nprobe: int, metric: str, mask: np.ndarray, id_base: int = 0):
    """The definition stated directly: per query the nprobe nearest lists (float64, ties to the lower list), the oracle's pair_keys
    over the ADMITTED rows of those lists, lexsort by (key, id), cut to k, padded."""
    nq = len(Q)
    D = np.full((nq, k), pad_value(metric), F32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        lists = nearest_lists(C, Q[q], metric, nprobe)
        rows = np.flatnonzero(mask & np.isin(lor, lists)).astype(np.int64)
        if len(rows) == 0:
            continue
        keys = pair_keys(X, Q[q:q + 1], rows[None, :], metric)[0]
        order = np.lexsort((rows, keys))[:k]
        I[q, :len(order)] = rows[order] + id_base
        D[q, :len(order)] = (keys[order] if metric == "l2" else -keys[order]).astype(F32)
    return D, I


def rule_declines(n: int, nlist: int, nprobe: int, k: int, n_allowed: int) -> bool:
    """ivf_filter_declines (csrc/ivf_filter_plan.hpp) for a batch the unfiltered ivf_geometry admits (its bins per query are then
    >= 4 k already): fewer than 4 k admitted rows probed, unless every row is admitted"""
    return n_allowed < n and nprobe * n_allowed / nlist < 4.0 * k

"""Hash-table LSH on the MI355X with the surface of the reference's own `lsh` slot (src/algorithms/lsh.py).

  HipLSHTableIndexer    drop-in for LSHIndexer     (lsh.py:27-141)
  HipLSHTableSearcher   drop-in for LSHSearcher    (lsh.py:144-301)
  HipLSHTables          drop-in for the stand-alone LSH class (lsh.py:304-359)

The reference keeps T dictionaries of buckets, counts votes over the buckets a query hits (`Counter.most_common()`), caps the
candidates and scores them exactly.  Here the rows' table keys live on the device next to the float32 rows (vdb_lsht_*): a
query's candidates are its colliding rows under (votes descending, first colliding table, id) -- the order `most_common()`
gives over buckets filled in id order -- and the exact re-rank is vdb_rerank's.  Projections and offsets are drawn exactly
as the reference draws them (`make_tables`), so its results are reproduced id for id.
"""
from __future__ import annotations

import math
from typing import Any, Optional, Tuple

import numpy as np

from .algorithms import (_resolve_device, apply_engine_options, euclidean_or_negated, indexer_operands, query_batch,
                         reserve_workspace, resident_mb)
from .index import FlatIndex
from .plugin_api import (BaseAlgorithm, BaseIndexer, BaseSearcher, IndexArtifact, Metadata, SearchResult, register_algorithm,
                         register_indexer, register_searcher)

MAX_CANDIDATES = 65536      # ncand limit of vdb_lsht_candidates / vdb_lsht_search


def make_tables(dim: int, num_tables: int, hash_size: int, metric: str = "cosine", bucket_width: float = 4.0,
                seed: int = 42) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(P float32 (T, H, dim), b float32 (T, H) or None): LSHIndexer.build's draws in its order (lsh.py:70-76, 99-101) --
    `normal(size=(T, H, dim))`, then for L2 `uniform(0, w, size=(T, H))`, from one `np.random.RandomState(seed)`."""
    rng = np.random.RandomState(seed)
    p = rng.normal(size=(int(num_tables), int(hash_size), int(dim))).astype(np.float32)
    b = None
    if metric == "l2":
        b = rng.uniform(0.0, bucket_width, size=(int(num_tables), int(hash_size))).astype(np.float32)
    return p, b


def candidate_cap(k: int, multiplier: float, max_candidates: Optional[int]) -> int:
    """LSHSearcher._select_candidates' cap (lsh.py:237-239); a cap the device select cannot serve is a ValueError."""
    cap = max_candidates or max(k, int(math.ceil(multiplier * k)))
    if cap > MAX_CANDIDATES:
        raise ValueError(f"the LSH candidate cap is at most {MAX_CANDIDATES}, got {cap}")
    return int(cap)


def _normalize_queries(q: np.ndarray) -> np.ndarray:
    """Row by row as the reference's _normalize_vector (lsh.py:19-24): the 1-D norm, a zero query stays zero.  Not
    algorithms._safe_normalize: the 1-D norm sums in another order, and the two differ in the last bit on one row in five."""
    out = np.zeros_like(q)
    for i, row in enumerate(q):
        norm = np.linalg.norm(row)
        if norm != 0:
            out[i] = row / norm
    return out


def _check_parameters(what: str, metric: str, num_tables: int, hash_size: int, bucket_width: float) -> None:
    if metric not in HipLSHTableIndexer.SUPPORTED_METRICS:
        raise ValueError(f"{what} supports metrics {HipLSHTableIndexer.SUPPORTED_METRICS}, received '{metric}'")
    if hash_size <= 0:
        raise ValueError("hash_size must be positive")
    if num_tables <= 0:
        raise ValueError("num_tables must be positive")
    if metric == "l2" and bucket_width <= 0:
        raise ValueError("bucket_width must be positive for L2 LSH")


def _build_index(vectors: np.ndarray, dimension: int, metric: str, num_tables: int, hash_size: int, bucket_width: float,
                 seed: int, params: dict) -> FlatIndex:
    data, library_metric, _ = indexer_operands(vectors, metric)    # (cosine: the reference's _normalize_rows, call for call)
    p, b = make_tables(dimension, num_tables, hash_size, metric, bucket_width, seed)
    device = _resolve_device(params.get("device"), params.get("device_ids"))
    index = FlatIndex(dimension, library_metric, device)
    apply_engine_options(index, params)
    index.lsht_set_tables(p, b, bucket_width if b is not None else 0.0)
    index.add(data)
    reserve_workspace(index, params)
    return index


def _search(index: FlatIndex, metric: str, queries: np.ndarray, k: int, cap: int, fallback: bool) -> SearchResult:
    q = query_batch(queries)
    if metric == "cosine":
        q = _normalize_queries(q)
    d, i = index.lsht_search(q, int(k), cap, fallback)
    if metric == "l2":
        return euclidean_or_negated(d, i, metric)
    d = (np.float32(1.0) - d).astype(np.float32)         # the reference's cosine distance
    d[i < 0] = np.inf
    return d, i


class HipLSHTableIndexer(BaseIndexer):
    """Flat index + T table keys per row on one MI355X (LSHIndexer: sign keys for cosine, E2 bucket keys for L2)."""

    SUPPORTED_METRICS = {"cosine", "l2"}

    def __init__(self, name: str, dimension: int, metric: str = "cosine", num_tables: int = 8, hash_size: int = 16,
                 bucket_width: float = 4.0, seed: int = 42, **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, num_tables=num_tables, hash_size=hash_size, bucket_width=bucket_width, seed=seed,
                         **kwargs)
        _check_parameters("LSHIndexer", metric, num_tables, hash_size, bucket_width)
        self.num_tables, self.hash_size, self.bucket_width, self.seed = num_tables, hash_size, bucket_width, seed

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected vectors with dimension {self.dimension}, received {vectors.shape[1]}")
        index = _build_index(vectors, self.dimension, self.metric, self.num_tables, self.hash_size, self.bucket_width, self.seed,
                             self.params)
        meta = {"metric": self.metric, "num_tables": self.num_tables, "hash_size": self.hash_size}
        if self.metric == "cosine":
            meta["normalize_queries"] = True
        else:
            meta["bucket_width"] = self.bucket_width
        return IndexArtifact(kind="hip_lsh_tables", data=index, metadata=meta)


class HipLSHTableSearcher(BaseSearcher):
    """LSHSearcher over a HipLSHTableIndexer artifact: `candidate_multiplier` (4.0), `max_candidates` (None),
    `fallback_to_bruteforce` (True)."""

    def __init__(self, name: str, dimension: int, metric: str = "cosine", candidate_multiplier: float = 4.0,
                 max_candidates: Optional[int] = None, fallback_to_bruteforce: bool = True, **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, candidate_multiplier=candidate_multiplier, max_candidates=max_candidates,
                         fallback_to_bruteforce=fallback_to_bruteforce, **kwargs)
        if candidate_multiplier <= 0:
            raise ValueError("candidate_multiplier must be positive")
        self.candidate_multiplier = candidate_multiplier
        self.max_candidates = max_candidates
        self.fallback_to_bruteforce = fallback_to_bruteforce
        self.index: Optional[FlatIndex] = None

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        if artifact.kind != "hip_lsh_tables":
            raise ValueError("HipLSHTableSearcher can only attach to artifacts produced by HipLSHTableIndexer")
        self.index = artifact.data
        self.metric = (artifact.metadata or {}).get("metric", self.metric)
        self._prepared = True

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        d, i = self.batch_search(query, k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        if not self._prepared:
            raise RuntimeError("LSHSearcher not attached to an index")
        cap = candidate_cap(int(k), self.candidate_multiplier, self.max_candidates)
        return _search(self.index, self.metric, queries, k, cap, bool(self.fallback_to_bruteforce))

    def get_memory_usage(self) -> float:
        return resident_mb(self.index)


class HipLSHTables(BaseAlgorithm):
    """Stand-alone counterpart of the reference's LSH class, same constructor keys and defaults."""

    def __init__(self, name: str, dimension: int, metric: str = "cosine", num_tables: int = 8, hash_size: int = 16,
                 bucket_width: float = 4.0, candidate_multiplier: float = 4.0, max_candidates: Optional[int] = None,
                 fallback_to_bruteforce: bool = True, seed: int = 42, **kwargs: Any) -> None:
        super().__init__(name, dimension, metric=metric, num_tables=num_tables, hash_size=hash_size, bucket_width=bucket_width,
                         candidate_multiplier=candidate_multiplier, max_candidates=max_candidates,
                         fallback_to_bruteforce=fallback_to_bruteforce, seed=seed, **kwargs)
        _check_parameters("LSHIndexer", metric, num_tables, hash_size, bucket_width)
        if candidate_multiplier <= 0:
            raise ValueError("candidate_multiplier must be positive")
        self.metric = metric
        self.num_tables, self.hash_size, self.bucket_width, self.seed = num_tables, hash_size, bucket_width, seed
        self.candidate_multiplier, self.max_candidates = candidate_multiplier, max_candidates
        self.fallback_to_bruteforce = fallback_to_bruteforce
        self.index: Optional[FlatIndex] = None

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected vectors with dimension {self.dimension}, received {vectors.shape[1]}")
        self.index = _build_index(vectors, self.dimension, self.metric, self.num_tables, self.hash_size, self.bucket_width,
                                  self.seed, self.config)
        self.index_built = True

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        d, i = self.batch_search(query, k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        if not self.index_built:
            raise RuntimeError("Index has not been built for LSH algorithm")
        cap = candidate_cap(int(k), self.candidate_multiplier, self.max_candidates)
        return _search(self.index, self.metric, queries, k, cap, bool(self.fallback_to_bruteforce))

    def get_memory_usage(self) -> float:
        return resident_mb(self.index)


register_indexer("HipLSHTableIndexer", HipLSHTableIndexer)
register_searcher("HipLSHTableSearcher", HipLSHTableSearcher)
register_algorithm("HipLSHTables", HipLSHTables)

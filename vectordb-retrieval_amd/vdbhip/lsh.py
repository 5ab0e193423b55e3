"""Sign-LSH on the MI355X with the reference's `faiss_lsh` surface.

  HipLSHIndexer    drop-in for FaissLSHIndexer                      (src/algorithms/modular.py:182-221)
  HipLSHSearcher   drop-in for the LSH branch of FaissSearcher      (src/algorithms/modular.py:455-548)

`faiss.IndexLSH(d, nbits)` with its defaults is a random rotation, one sign bit per output and a Hamming search; the
searcher asks it for `candidate_k` ids and re-scores them against the float32 rows.  Here the whole chain runs on the
device (vdb_lsh_*: query -> code -> Hamming top-c -> exact top-k).  FAISS' random matrix and its order among equal
Hamming distances are not reproduced: the projection is `make_projection` (same construction, NumPy's generator) and
ties go to the smaller id, as everywhere in the library.
"""
from __future__ import annotations

from typing import Any, Optional

import numpy as np

from .algorithms import (FaissStyleSearcher, _resolve_device, apply_engine_options, euclidean_or_negated, indexer_operands,
                         reserve_workspace, warmup_rows)
from .index import FlatIndex
from .plugin_api import BaseIndexer, IndexArtifact, Metadata, SearchResult, register_indexer, register_searcher

MAX_CANDIDATES = 65536      # ncand limit of vdb_lsh_candidates / vdb_lsh_search


def make_projection(dim: int, nbits: int, seed: int = 0) -> np.ndarray:
    """float32 (nbits, dim): the top-left block of the Q factor of an m x m Gaussian matrix, m = max(nbits, dim) -- the
    construction of FAISS' RandomRotationMatrix (orthonormal columns when nbits >= dim, orthonormal rows otherwise)."""
    dim, nbits = int(dim), int(nbits)
    if dim < 1 or nbits < 1:
        raise ValueError("dim and nbits must be positive")
    m = max(nbits, dim)
    g = np.random.default_rng(seed).standard_normal((m, m))
    q, _ = np.linalg.qr(g)
    return np.ascontiguousarray(q[:nbits, :dim], dtype=np.float32)


def candidate_count(k: int, multiplier: float, max_candidates: Optional[int], ntotal: int) -> int:
    """candidate_k of FaissSearcher._batch_search_lsh_rerank (modular.py:463-468), statement by statement."""
    candidate_k = max(k, 1)
    if multiplier > 1.0:
        candidate_k = int(max(candidate_k, k * multiplier))
    if max_candidates is not None:
        candidate_k = min(candidate_k, max_candidates)
    return min(candidate_k, ntotal)


class HipLSHIndexer(BaseIndexer):
    """Flat index + sign-LSH codes on one MI355X (FaissLSHIndexer: `num_bits` random-hyperplane bits per row)."""

    SUPPORTED_METRICS = {"l2", "cosine", "ip"}

    def __init__(self, name: str, dimension: int, metric: str = "l2", num_bits: int = 256, seed: int = 0, **kwargs: Any) -> None:
        if metric not in self.SUPPORTED_METRICS:
            raise ValueError(f"FaissLSHIndexer supports metrics {self.SUPPORTED_METRICS}, received '{metric}'")
        if num_bits <= 0:
            raise ValueError("num_bits must be positive")
        if num_bits % 32 or num_bits > 1024:
            raise ValueError("num_bits must be a multiple of 32 in [32, 1024]")
        super().__init__(name, dimension, metric, num_bits=num_bits, seed=seed, **kwargs)
        self.num_bits = int(num_bits)
        self.seed = int(seed)

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected dimension {self.dimension}, got {vectors.shape[1]}")
        data, metric, _ = indexer_operands(vectors, self.metric)
        meta = {"metric": self.metric, "num_bits": self.num_bits, "faiss_index_kind": "lsh", "seed": self.seed}
        if self.metric == "cosine":                 # (FaissLSHIndexer's own entries, not the factory indexer's)
            meta["normalize_queries"] = True
        elif self.metric == "ip":
            meta["faiss_metric"] = "ip"
        device = _resolve_device(self.params.get("device"), self.params.get("device_ids"))
        index = FlatIndex(self.dimension, metric, device)
        apply_engine_options(index, self.params)
        index.lsh_set_projection(make_projection(self.dimension, self.num_bits, self.seed))
        index.add(data)
        reserve_workspace(index, self.params)
        meta["reserve_queries"] = self.params.get("reserve_queries")
        return IndexArtifact(kind="hip_lsh", data=index, metadata=meta)


class HipLSHSearcher(FaissStyleSearcher):
    """FaissSearcher's LSH branch over a HipLSHIndexer artifact: `lsh_rerank` (True), `lsh_candidate_multiplier` (8.0),
    `lsh_max_candidates` (None)."""

    _kind = "hip_lsh"

    def __init__(self, name: str, dimension: int, metric: str = "l2", **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, **kwargs)
        self._lsh_rerank = bool(self.params.get("lsh_rerank", True))
        self._lsh_candidate_multiplier = float(self.params.get("lsh_candidate_multiplier", 8.0))
        max_candidates = self.params.get("lsh_max_candidates")
        self._lsh_max_candidates = int(max_candidates) if max_candidates is not None else None

    def candidate_count(self, k: int, ntotal: int) -> int:
        return candidate_count(k, self._lsh_candidate_multiplier, self._lsh_max_candidates, ntotal)

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        meta = self._bind(artifact)
        self._prepared = True
        # size the LSH workspace now, as reserve_workspace does for the flat one (the harness times its first batch)
        n = warmup_rows(self.index, self.params.get("reserve_queries", meta.get("reserve_queries")))
        if n:
            c = self.candidate_count(10, self.index.ntotal)
            if 0 < c <= MAX_CANDIDATES:
                self.index.lsh_search(np.asarray(vectors[:n], dtype=np.float32), 10, c)

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        self._require_attached()
        q = self._prepare_query(queries)
        ntotal = self.index.ntotal
        if ntotal <= 0:
            raise RuntimeError("LSH index has no vectors to search")
        candidate_k = self.candidate_count(k, ntotal) if self._lsh_rerank else 0
        if candidate_k <= 0:                  # no re-rank (or the degenerate case of modular.py:470-475): raw Hamming order
            ham, ids = self.index.lsh_candidates(q, k)
            d = ham.astype(np.float32)
            if self.metric in {"cosine", "ip"}:
                d = -d
            d[ids < 0] = np.inf
            return d, ids
        return euclidean_or_negated(*self.index.lsh_search(q, k, candidate_k), self.metric)


register_indexer("HipLSHIndexer", HipLSHIndexer)
register_searcher("HipLSHSearcher", HipLSHSearcher)

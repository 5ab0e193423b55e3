"""MI355X-backed plugins with the reference's names, argument meaning and output conventions, and the conventions every
plugin module shares (one copy each: operands of an indexer, query batch, result convention, memory figure, warm-up sizing,
the FAISS-style searcher base and the raw-convention algorithm base).

  HipExactSearch         drop-in for ExactSearch            (src/algorithms/exact_search.py:6-78)
  HipBruteForceIndexer   drop-in for BruteForceIndexer      (src/algorithms/modular.py:121-133)
  HipLinearSearcher      drop-in for LinearSearcher         (src/algorithms/modular.py:312-390)

Convention matrix reproduced here; all return (float32 (Q,k), int64 (Q,k)), best first:
  ExactSearch     l2 -> squared L2          | cosine/ip -> raw inner product (NOT normalised), descending
                  k > N -> id -1, distance +FLT_MAX / -FLT_MAX   (faiss.IndexFlat padding)
  LinearSearcher  l2 -> sqrt(squared L2)    | cosine -> -(q^ . x^) | ip -> -(q . x), ascending
                  k > N -> id -1, distance +inf
  FaissSearcher   l2 -> squared L2          | cosine -> -(q^ . x^) | ip -> -(q . x), ascending; faiss.IndexFlat padding
The GPU work is done by libvdbhip through the index classes; nothing here computes distances on the CPU.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import _ffi
from .index import FlatIndex
from .plugin_api import (BaseAlgorithm, BaseIndexer, BaseSearcher, IndexArtifact, Metadata, SearchResult,
                         register_algorithm, register_indexer, register_searcher)


def _safe_normalize(matrix: np.ndarray) -> np.ndarray:
    """Rows scaled to unit length, zero rows stay zero -- same NumPy calls as modular.py:109-111 so the
    normalised float32 operands are bit-identical to the reference's."""
    norms = np.linalg.norm(matrix, axis=1, keepdims=True)
    return np.divide(matrix, norms, out=np.zeros_like(matrix), where=norms > 0)


def _resolve_device(device, device_ids):
    """GPU(s) of an index: `device` (an ordinal, or a list of them) wins over `device_ids`; more than one ordinal means ONE
    index row-sharded over those GPUs inside this process (vdb_create_multi) -- the reference's harness is a single process
    (experiment_runner.py:329-331, 428-434), so this is how a YAML entry `{type: HipExactSearch, device_ids: [0, .., 7]}`
    reaches eight MI355X.  Returns an int or a list of ints."""
    from .index import normalize_devices

    if device is not None:
        return normalize_devices(device)
    if device_ids is not None and not isinstance(device_ids, (int, np.integer)) and len(device_ids) > 0:
        return normalize_devices(list(device_ids))
    if isinstance(device_ids, (int, np.integer)):
        return int(device_ids)
    import os

    return int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("VDBHIP_DEVICE_FROM_RANK") else 0


DEFAULT_RESERVE_QUERIES = 10_000


def reserve_workspace(index, params: dict, k: int = 10) -> None:
    """Size the search workspace at build time for batches of `reserve_queries` queries (default 10 000, 0 = leave it to
    the first search).  The reference harness times its first batch_search with the allocations it triggers
    (experiment_runner.py:431-437; no warm-up, metrics_methodology.md:119-121); FAISS' GPU resources reserve their scratch
    memory at construction for the same reason."""
    n = int((params or {}).get("reserve_queries", DEFAULT_RESERVE_QUERIES))
    if n > 0 and index is not None and index.ntotal > 0:
        index.reserve(n, k)


def warmup_rows(index, reserve) -> int:
    """Rows of the one warm-up search that sizes a workspace `vdb_reserve` does not cover (sign-LSH, graph search):
    min(reserve, ntotal); `reserve` None = the default of reserve_workspace, 0 = no warm-up."""
    reserve = DEFAULT_RESERVE_QUERIES if reserve is None else int(reserve)
    return min(reserve, index.ntotal) if reserve > 0 and index.ntotal > 0 else 0


def apply_engine_options(index, params: dict) -> None:
    """`engine_options: {name: value}` of an algorithm / indexer / searcher config entry are handed to `vdb_set_option`
    before the corpus is added (include/vdbhip.h lists them; e.g. `stream_panels: 1` for a 768-dim corpus that should
    occupy ~1.2x instead of ~1.6x its float32 bytes).  An unknown name raises, as the C-ABI does."""
    for key, value in ((params or {}).get("engine_options") or {}).items():
        index.set_option(str(key), float(value))


def indexer_operands(vectors: np.ndarray, metric: str) -> Tuple[np.ndarray, str, Dict[str, Any]]:
    """(rows, library metric, metadata entries) of a FAISS-style indexer (modular.py:253-262): cosine = rows normalised +
    inner product, and the artifact tells the searcher to normalise its queries."""
    data = _ffi.as_f32_c(vectors)
    if metric == "cosine":
        return _safe_normalize(data), "ip", {"faiss_metric": "ip", "normalize_queries": True, "normalize_vectors": True}
    library = "ip" if metric == "ip" else "l2"
    return data, library, {"faiss_metric": library}


def query_batch(queries: np.ndarray, normalize: bool = False) -> np.ndarray:
    """A float32 (nq, dim) copy of the caller's queries (one query: a batch of one), rows normalised on request."""
    q = np.asarray(queries)
    if q.ndim == 1:
        q = q.reshape(1, -1)
    q = q.astype(np.float32, copy=True)
    return _safe_normalize(q) if normalize else q


def euclidean_or_negated(d: np.ndarray, i: np.ndarray, metric: str) -> SearchResult:
    """Library results -> LinearSearcher's convention: Euclidean distance for 'l2', negated score otherwise, +inf where
    the id is -1."""
    pad = i < 0
    d = np.sqrt(np.where(pad, np.float32(0), d), dtype=np.float32) if metric == "l2" else -d
    d[pad] = np.inf
    return d.astype(np.float32, copy=False), i


def resident_mb(index) -> float:
    """MB resident in HBM (picked up by experiment_runner.py:493-497); 0.0 without an index."""
    return index.stats()["bytes_resident"] / (1024.0 * 1024.0) if index else 0.0


class RawAlgorithm(BaseAlgorithm):
    """A stand-alone algorithm over one index (self.index) with the raw FAISS conventions of ApproximateSearch
    (approximate_search.py:53-87): no normalisation, no sign flip."""

    index = None

    def _require_built(self) -> None:
        if not self.index_built:
            raise RuntimeError("Index has not been built yet.")

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        self._require_built()
        d, i = self.index.search(np.array([query], dtype=np.float32), k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        self._require_built()
        return self.index.search(np.asarray(queries).astype(np.float32), k)

    def get_memory_usage(self) -> float:
        return resident_mb(self.index)


class FaissStyleSearcher(BaseSearcher):
    """FaissSearcher (modular.py:393-449, 536-548) over an artifact of kind `_kind` whose data is one of this library's
    indexes: queries normalised when the artifact says so, distances negated for cosine / ip, squared L2 as it is.  A
    subclass adds its own parameters in `attach` (after `_bind`) and, where it is not `index.search`, `_search_index`."""

    _kind = ""

    def __init__(self, name: str, dimension: int, metric: str = "l2", **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, **kwargs)
        self.index = None
        self.normalize_queries = False

    def _bind(self, artifact: IndexArtifact) -> dict:
        """The part of `attach` every subclass shares; returns the artifact's metadata."""
        if artifact.kind != self._kind:
            raise ValueError(f"{type(self).__name__} requires '{self._kind}' artifact")
        self.index = artifact.data
        meta = artifact.metadata or {}
        self.metric = meta.get("metric", self.metric)
        self.normalize_queries = meta.get("normalize_queries", False)
        return meta

    def _require_attached(self) -> None:
        if not self._prepared:
            raise RuntimeError("FaissSearcher not attached to an index")

    def _prepare_query(self, query: np.ndarray) -> np.ndarray:
        return query_batch(query, self.normalize_queries)

    def _search_index(self, queries: np.ndarray, k: int) -> SearchResult:
        return self.index.search(queries, k)

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        d, i = self.batch_search(self._prepare_query(query), k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        self._require_attached()
        d, i = self._search_index(self._prepare_query(queries), k)
        if self.metric in {"cosine", "ip"}:
            d = -d
        return d.astype(np.float32), i.astype(np.int64)

    def get_memory_usage(self) -> float:
        return resident_mb(self.index)


class HipExactSearch(RawAlgorithm):
    """Exact k-NN on one MI355X -- or, with `device_ids: [..]` of several, on ONE index row-sharded over them in this
    process; same constructor and results as ExactSearch (faiss.IndexFlat)."""

    def __init__(self, name: str, dimension: int, metric: str = "l2", device=None,
                 device_ids=None, **kwargs: Any) -> None:
        super().__init__(name, dimension, **kwargs)
        if device_ids is not None:
            self.config["device_ids"] = list(device_ids) if not isinstance(device_ids, (int, np.integer)) else int(device_ids)
        # exact_search.py:23 -- 'l2' -> METRIC_L2, anything else -> METRIC_INNER_PRODUCT (no normalisation)
        self.metric = "l2" if metric == "l2" else "ip"
        self.device = _resolve_device(device, device_ids)
        self.index: Optional[FlatIndex] = None

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        self.vectors = _ffi.as_f32_c(vectors)
        if self.vectors.ndim != 2 or self.vectors.shape[1] != self.dimension:
            raise ValueError(f"expected (n, {self.dimension}) vectors, got {self.vectors.shape}")
        self.index = FlatIndex(self.dimension, self.metric, self.device)
        apply_engine_options(self.index, self.config)
        self.index.add(self.vectors)
        reserve_workspace(self.index, self.config)
        self.index_built = True

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        self._require_built()
        d, i = self.index.search(np.asarray(query, dtype=np.float32).reshape(1, -1), k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10, allowed=None) -> SearchResult:
        """`allowed` (None: every row): a bool mask over the rows, an integer id array or anything else FlatIndex.set_filter
        takes -- the k nearest among those rows, same conventions and padding.  The same array object is installed once."""
        self._require_built()
        q = _ffi.as_f32_c(queries)
        if allowed is None:
            self.record_operation("ndis", float(q.shape[0]) * float(self.index.ntotal))
            return self.index.search(q, k)
        self.index.ensure_filter(allowed)
        self.record_operation("ndis", float(q.shape[0]) * float(self.index.filter_count))
        return self.index.search_filtered(q, k)

    def range_search(self, queries: np.ndarray, radius: float, sort: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """faiss.IndexFlat.range_search in the raw conventions: (lims, D, I) of the rows with squared L2 < radius / inner
        product > radius.  Per query the rows come in ascending id; `sort=True` orders them nearest first, by (D, id)."""
        self._require_built()
        q = _ffi.as_f32_queries(queries)
        self.record_operation("ndis", float(q.shape[0]) * float(self.index.ntotal))
        lims, d, i = self.index.range_search(q, radius)
        if sort and len(i):
            owner = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
            order = np.lexsort((i, d if self.metric == "l2" else -d, owner))
            d, i = d[order], i[order]
        return lims, d, i


def _flat_index(store: np.ndarray, dimension: int, metric: str, params: dict) -> FlatIndex:
    """The flat index of the brute-force pair: options, rows (normalised for cosine), workspace."""
    data, library_metric, _ = indexer_operands(store, metric)
    index = FlatIndex(dimension, library_metric, _resolve_device(params.get("device"), params.get("device_ids")))
    apply_engine_options(index, params)
    index.add(data)
    reserve_workspace(index, params)
    return index


class HipBruteForceIndexer(BaseIndexer):
    """Keeps the raw matrix (as the reference does) and uploads it to HBM once, at build time."""

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        store = _ffi.as_f32_c(vectors)
        if store.ndim != 2 or store.shape[1] != self.dimension:
            raise ValueError("Vector dimension mismatch in HipBruteForceIndexer")
        if self.metric not in ("l2", "cosine", "ip"):
            # same late failure as the reference: an unknown metric only breaks at search time
            return IndexArtifact(kind="raw_vectors", data=store,
                                 metadata={"metric": self.metric, "normalize_vectors": False})
        index = _flat_index(store, self.dimension, self.metric, self.params)
        return IndexArtifact(kind="raw_vectors", data=store,
                             metadata={"metric": self.metric, "normalize_vectors": self.metric == "cosine",
                                       "hip_index": index, "hip_index_metric": self.metric})


class HipLinearSearcher(BaseSearcher):
    """LinearSearcher semantics; the scan itself runs on the MI355X."""

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        if artifact.kind != "raw_vectors":
            raise ValueError("HipLinearSearcher requires 'raw_vectors' artifact")
        store = artifact.data
        if store.shape[1] != self.dimension:
            raise ValueError("Vector dimension mismatch in LinearSearcher")
        self._ntotal = int(store.shape[0])
        self._index: Optional[FlatIndex] = None
        meta = artifact.metadata or {}
        if self.metric in ("l2", "cosine", "ip"):
            if meta.get("hip_index") is not None and meta.get("hip_index_metric") == self.metric:
                self._index = meta["hip_index"]
            else:  # artifact from the reference's own BruteForceIndexer, or built for another metric
                self._index = _flat_index(store, self.dimension, self.metric, self.params)
        self._prepared = True

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        d, i = self.batch_search(query_batch(query), k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10, allowed=None) -> SearchResult:
        """`allowed` (None: every row): what FlatIndex.set_filter takes -- the k nearest among those rows, in this searcher's
        conventions (+inf / -1 where fewer than k rows are admitted).  The same array object is installed once."""
        if not self._prepared:
            raise RuntimeError("LinearSearcher not attached to an index")
        if self.metric not in ("l2", "cosine", "ip"):
            raise ValueError(f"Unsupported metric '{self.metric}' for LinearSearcher")
        if self._ntotal == 0:
            raise RuntimeError("LinearSearcher cannot operate on empty index")
        q = query_batch(queries, self.metric == "cosine")
        if allowed is None:
            d, i = self._index.search(q, k)
        else:
            self._index.ensure_filter(allowed)
            d, i = self._index.search_filtered(q, k)
        return euclidean_or_negated(d, i, self.metric)

    def range_search(self, queries: np.ndarray, radius: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(lims, distances, ids) in this searcher's conventions, ascending id per query.  'l2': the rows at Euclidean
        distance below `radius` (the library is asked for squared distances below float32(radius) * float32(radius)) with
        their Euclidean distances; 'cosine' / 'ip': `radius` is a similarity threshold -- the rows whose score (queries
        normalised for cosine) exceeds it, with the negated scores `batch_search` returns."""
        if not self._prepared:
            raise RuntimeError("LinearSearcher not attached to an index")
        if self.metric not in ("l2", "cosine", "ip"):
            raise ValueError(f"Unsupported metric '{self.metric}' for LinearSearcher")
        if self._ntotal == 0:
            raise RuntimeError("LinearSearcher cannot operate on empty index")
        r = np.float32(radius)
        lims, d, i = self._index.range_search(query_batch(queries, self.metric == "cosine"), r * r if self.metric == "l2" else r)
        return (lims,) + euclidean_or_negated(d, i, self.metric)

    def get_memory_usage(self) -> float:
        return resident_mb(getattr(self, "_index", None))


def rerank_candidates(index: FlatIndex, queries: np.ndarray, candidate_ids: np.ndarray, k: int, metric: str):
    """Candidate re-scoring with the conventions of FaissSearcher._batch_search_lsh_rerank (modular.py:455-534):
    per query the valid (>= 0) candidate ids are re-scored exactly and the best k returned -- Euclidean distance
    for 'l2', negated score for 'cosine' / 'ip' (queries and the indexed vectors already normalised for cosine),
    unused slots padded with +inf / -1.  One batched launch replaces the reference's per-query Python loop."""
    return euclidean_or_negated(*index.rerank(queries, candidate_ids, k), metric)


register_algorithm("HipExactSearch", HipExactSearch)
register_indexer("HipBruteForceIndexer", HipBruteForceIndexer)
register_searcher("HipLinearSearcher", HipLinearSearcher)

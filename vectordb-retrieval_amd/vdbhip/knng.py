"""k-NN graph index on the MI355X behind the reference's HNSW surface.

  KnnGraphIndex         FlatIndex + the vdb_knng_* calls (include/vdbhip.h)
  HipKnnGraphIndexer    stands in for HNSWIndexer                      (src/algorithms/modular.py:136-179)
  HipKnnGraphSearcher   FaissSearcher conventions over its artifact   (src/algorithms/modular.py:418-449, 536-548)
  HipKnnGraphSearch     stand-alone counterpart of the HNSW class      (src/algorithms/hnsw.py:6-141)

`faiss.IndexHNSWFlat` inserts rows one by one into a layered graph; here the graph is built at once -- the exact `ncand`
nearest neighbours of every row (the library's own scan, rows as queries), pruned to `degree = 2 M` by the HNSW neighbour
heuristic with the rejected candidates kept as fill -- and searched by a beam of width `efSearch` from evenly spaced entry
rows.  One layer, no level draw: FAISS' graph, its float32 distances and its tie order are not reproduced; the contract
is the library's own (deterministic, restated in NumPy by tests/knng_restatement.py).
"""
from __future__ import annotations

import ctypes
from typing import Any, Optional, Tuple

import numpy as np

from . import _ffi
from .algorithms import (DEFAULT_RESERVE_QUERIES, FaissStyleSearcher, _resolve_device, _safe_normalize, apply_engine_options,
                         indexer_operands, query_batch, reserve_workspace, resident_mb, warmup_rows)
from .index import FlatIndex, _pair
from .plugin_api import (BaseAlgorithm, BaseIndexer, IndexArtifact, Metadata, SearchResult, register_algorithm, register_indexer,
                         register_searcher)

MAX_EF = 512            # ef limit of vdb_knng_search (and so of k)
MAX_DEGREE = 64
MAX_NCAND = 128


def graph_parameters(M: int, ncand: Optional[int] = None) -> Tuple[int, int]:
    """(degree, ncand) of an HNSW `M`: degree = 2 M, HNSW's layer-0 degree; ncand defaults to min(2 degree, 128)."""
    M = int(M)
    if M < 2 or 2 * M > MAX_DEGREE:
        raise ValueError(f"M must be in [2, {MAX_DEGREE // 2}] (degree = 2 M in [4, {MAX_DEGREE}]), got {M}")
    degree = 2 * M
    ncand = min(2 * degree, MAX_NCAND) if ncand is None else int(ncand)
    if ncand < degree or ncand > MAX_NCAND:
        raise ValueError(f"ncand must be in [degree = {degree}, {MAX_NCAND}], got {ncand}")
    return degree, ncand


class KnnGraphIndex(FlatIndex):
    """A flat index that can carry a k-NN graph next to its float32 rows.  Its `search` stays the exact search."""

    def knng_build(self, degree: int = 32, ncand: Optional[int] = None) -> None:
        """Build the graph of the rows present (any later add, and reset, drop it)."""
        ncand = min(2 * int(degree), MAX_NCAND) if ncand is None else int(ncand)
        _ffi.check(self._lib.vdb_knng_build(self._handle(), int(degree), ncand), build_time=True)

    def knng_set(self, neighbours: np.ndarray) -> None:
        """Inject a graph: int32 (ntotal, degree) local row numbers, -1 only as a row's tail."""
        nb = np.ascontiguousarray(neighbours, dtype=np.int32)
        if nb.ndim != 2 or nb.shape[0] != self.ntotal:
            raise ValueError(f"expected ({self.ntotal}, degree) neighbours, got {nb.shape}")
        _ffi.check(self._lib.vdb_knng_set(self._handle(), int(nb.shape[1]), _ffi.ptr(nb)), build_time=True)

    @property
    def knng_degree(self) -> int:
        degree = ctypes.c_int(0)
        _ffi.check(self._lib.vdb_knng_get(self._handle(), ctypes.byref(degree), None))
        return int(degree.value)

    def knng_get(self) -> Optional[np.ndarray]:
        """int32 (ntotal, degree), or None when the handle carries no graph."""
        degree = ctypes.c_int(0)
        _ffi.check(self._lib.vdb_knng_get(self._handle(), ctypes.byref(degree), None))
        if degree.value == 0:
            return None
        nb = np.empty((self.ntotal, degree.value), np.int32)
        _ffi.check(self._lib.vdb_knng_get(self._handle(), ctypes.byref(degree), _ffi.ptr(nb)))
        return nb

    def knng_search(self, queries: np.ndarray, k: int, ef: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Beam search of width `ef` (default k): flat conventions and padding."""
        q = self._queries(queries)
        ef = int(k) if ef is None else int(ef)
        D, I = _pair(q.shape[0], int(k))
        _ffi.check(self._lib.vdb_knng_search(self._handle(), _ffi.ptr(q), q.shape[0], int(k), ef, _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def knng_search_device(self, q_ptr: int, nq: int, k: int, ef: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """All pointers are device memory on this index's GPU; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_knng_search_device(self._handle(), q_ptr, int(nq), int(k), int(ef), d_ptr, i_ptr, stream or None))


def _build_graph_index(data: np.ndarray, dim: int, metric: str, degree: int, ncand: int, params: dict) -> KnnGraphIndex:
    device = _resolve_device(params.get("device"), params.get("device_ids"))
    index = KnnGraphIndex(dim, metric, device)
    apply_engine_options(index, params)
    index.add(data)
    reserve_workspace(index, params)
    index.knng_build(degree, ncand)
    return index


def _reserve_search(index: KnnGraphIndex, vectors: np.ndarray, reserve, ef: int) -> None:
    """Size the graph search's workspace now (the harness times its first batch)."""
    n = warmup_rows(index, reserve)
    if n:
        index.knng_search(np.asarray(vectors[:n], dtype=np.float32), min(10, ef), ef)


class HipKnnGraphIndexer(BaseIndexer):
    """Flat index + pruned exact k-NN graph on one MI355X, with HNSWIndexer's constructor.

    `M`: degree = 2 M (HNSW's layer-0 degree).  `ncand`: nearest neighbours the prune chooses from (default min(2 degree,
    128)).  `efSearch`: default beam width of the searcher.  `efConstruction` is accepted and recorded in the artifact
    metadata, and is otherwise UNUSED: the candidates of every row are its exact nearest neighbours, there is no
    construction-time beam to widen."""

    SUPPORTED_METRICS = {"l2", "cosine", "ip"}

    def __init__(self, name: str, dimension: int, metric: str = "l2", M: int = 16, efConstruction: int = 200,
                 efSearch: int = 100, ncand: Optional[int] = None, **kwargs: Any) -> None:
        if metric not in self.SUPPORTED_METRICS:
            raise ValueError(f"HipKnnGraphIndexer supports metrics {self.SUPPORTED_METRICS}, received '{metric}'")
        self.degree, self.ncand = graph_parameters(M, ncand)
        if int(efSearch) < 1 or int(efSearch) > MAX_EF:
            raise ValueError(f"efSearch must be in [1, {MAX_EF}], got {efSearch}")
        super().__init__(name, dimension, metric, M=M, efConstruction=efConstruction, efSearch=efSearch, ncand=ncand, **kwargs)
        self.M, self.efConstruction, self.efSearch = int(M), int(efConstruction), int(efSearch)

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected dimension {self.dimension}, got {vectors.shape[1]}")
        data, metric, entries = indexer_operands(vectors, self.metric)
        meta = {"metric": self.metric, **entries, "efSearch": self.efSearch, "efConstruction": self.efConstruction,
                "M": self.M, "degree": self.degree, "ncand": self.ncand, "reserve_queries": self.params.get("reserve_queries")}
        index = _build_graph_index(data, self.dimension, metric, self.degree, self.ncand, self.params)
        return IndexArtifact(kind="hip_knng", data=index, metadata=meta)


class HipKnnGraphSearcher(FaissStyleSearcher):
    """FaissSearcher semantics over a HipKnnGraphIndexer artifact (as HipIVFSearcher applies them: squared L2 as it is, negated
    scores for cosine / ip).  The beam width is ef = max(efSearch, k); an `efSearch` given here overrides the artifact's."""

    _kind = "hip_knng"

    def __init__(self, name: str, dimension: int, metric: str = "l2", **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, **kwargs)
        self.efSearch = 100

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        meta = self._bind(artifact)
        ef = self.params.get("efSearch")
        if ef is None:
            ef = meta.get("efSearch", 100)
        self.efSearch = int(ef)
        if self.efSearch < 1 or self.efSearch > MAX_EF:
            raise ValueError(f"efSearch must be in [1, {MAX_EF}], got {self.efSearch}")
        self._prepared = True
        data = _safe_normalize(_ffi.as_f32_c(vectors[:DEFAULT_RESERVE_QUERIES]).copy()) if self.normalize_queries else vectors
        _reserve_search(self.index, data, self.params.get("reserve_queries", meta.get("reserve_queries")), self.efSearch)

    def _search_index(self, queries: np.ndarray, k: int) -> SearchResult:
        if int(k) > MAX_EF:
            raise RuntimeError(f"the k-NN graph search returns at most {MAX_EF} neighbours, got k = {k}")
        return self.index.knng_search(queries, int(k), max(self.efSearch, int(k)))


class HipKnnGraphSearch(BaseAlgorithm):
    """Stand-alone counterpart of the reference's HNSW class, same constructor keys: metric 'l2', 'cosine' (rows and queries
    normalised, inner product) or 'dot' (raw inner product); results in faiss conventions, as HNSW returns them (squared L2
    ascending / inner products descending).  `efConstruction` is accepted and unused (see HipKnnGraphIndexer)."""

    def __init__(self, name: str, dimension: int, M: int = 16, efConstruction: int = 200, efSearch: int = 100,
                 metric: str = "l2", ncand: Optional[int] = None, device=None, device_ids=None, **kwargs: Any) -> None:
        super().__init__(name, dimension, **kwargs)
        self.degree, self.ncand = graph_parameters(M, ncand)
        if int(efSearch) < 1 or int(efSearch) > MAX_EF:
            raise ValueError(f"efSearch must be in [1, {MAX_EF}], got {efSearch}")
        self.M, self.efConstruction, self.efSearch, self.metric = int(M), int(efConstruction), int(efSearch), metric
        self._device_params = {"device": device, "device_ids": device_ids}
        self.index: Optional[KnnGraphIndex] = None
        self.config.update({"M": self.M, "efConstruction": self.efConstruction, "efSearch": self.efSearch, "metric": self.metric})

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected vectors of dimension {self.dimension}, got {vectors.shape[1]}")
        self.vectors = vectors
        self.metadata = metadata
        data = _ffi.as_f32_c(vectors)
        if self.metric == "cosine":
            data = _safe_normalize(data)
        params = dict(self.config)
        params.update(self._device_params)
        self.index = _build_graph_index(data, self.dimension, "l2" if self.metric not in {"cosine", "dot"} else "ip",
                                        self.degree, self.ncand, params)
        _reserve_search(self.index, data, self.config.get("reserve_queries"), self.efSearch)
        self.index_built = True

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        d, i = self.batch_search(query, k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        if not self.index_built:
            raise RuntimeError("Index not built. Call build_index() first.")
        if int(k) > MAX_EF:
            raise RuntimeError(f"the k-NN graph search returns at most {MAX_EF} neighbours, got k = {k}")
        return self.index.knng_search(query_batch(queries, self.metric == "cosine"), int(k), max(self.efSearch, int(k)))

    def get_memory_usage(self) -> float:
        return resident_mb(self.index)


register_indexer("HipKnnGraphIndexer", HipKnnGraphIndexer)
register_searcher("HipKnnGraphSearcher", HipKnnGraphSearcher)
register_algorithm("HipKnnGraphSearch", HipKnnGraphSearch)

"""Flat product quantization on the MI355X behind the reference's `pq` entry points.

  HipPQIndexer    drop-in for FaissFactoryIndexer with a "PQ<M>" key         (src/algorithms/modular.py:224-309)
  HipPQSearcher   drop-in for the non-LSH branch of FaissSearcher on it     (src/algorithms/modular.py:393-449, 536-548)
  HipPQSearch     BaseAlgorithm form for `type:` entries (`index_type="PQ64"`), raw conventions of HipApproximateSearch

"PQ<M>" is `faiss.IndexPQ(d, M, 8)`: M sub-vectors of d / M dimensions, 256 centroids each, one byte per sub-vector.  The
index keeps the codes and the codebooks and no float32 rows; a search returns, bit for bit, the flat exact search of this
library over the reconstructed rows (include/vdbhip.h, vdb_pq_*).  FAISS' k-means, its float32 table sums and its order
among equal distances are not reproduced: the codebooks come from the library's own k-means (one run per sub-space, FAISS'
defaults: 25 iterations, at most 256 training points per centroid) and ties go to the smaller id.
"""
from __future__ import annotations

import ctypes
import re
from typing import Any, Optional, Tuple

import numpy as np

from . import _ffi
from .index import _Handle, normalize_devices
from .algorithms import _resolve_device, _safe_normalize, apply_engine_options, reserve_workspace
from .plugin_api import (BaseAlgorithm, BaseIndexer, BaseSearcher, IndexArtifact, Metadata, SearchResult,
                         register_algorithm, register_indexer, register_searcher)

_PQ_KEY = re.compile(r"^\s*PQ(\d+)(?:x8)?\s*$")


def parse_pq_key(key: str) -> int:
    """M of a "PQ<M>" / "PQ<M>x8" key; every other key (any other bit width included) raises ValueError."""
    m = _PQ_KEY.match(str(key))
    if not m or int(m.group(1)) < 1:
        raise ValueError(f"unsupported index key {key!r}: only 'PQ<M>' (8 bits per sub-vector) is implemented here")
    return int(m.group(1))


class PQIndex(_Handle):
    """Device-resident PQ<M> index (replaces faiss.IndexPQ(d, M, 8)).  One GPU only."""

    def __init__(self, dim: int, M: int, metric: str = "l2", device=0):
        if metric not in ("l2", "ip"):
            raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
        device = normalize_devices(device)
        if isinstance(device, list):
            raise ValueError("PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available")
        dim, M = int(dim), int(M)
        if M < 1 or M > min(dim, 256) or dim % M:
            raise ValueError(f"M must divide dim and lie in [1, min(dim, 256)]; got dim={dim}, M={M}")
        self.dim, self.M, self.dsub, self.metric, self.device = dim, M, dim // M, metric, device
        super().__init__(self.dim, 0 if metric == "l2" else 1, self.device)
        self.is_trained = False
        self.ntotal = 0

    def _sync_ntotal(self) -> None:
        self.ntotal = int(self.stats()["ntotal"])

    # -- codebooks ----------------------------------------------------------------------------------------
    def train(self, x: np.ndarray, niter: int = 25, seed: int = 1234, max_points_per_centroid: int = 256) -> None:
        x = _ffi.as_f32_c(x)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected (n, {self.dim}) vectors, got {x.shape}")
        _ffi.check(self._lib.vdb_pq_train(self._handle(), self.M, _ffi.ptr(x), x.shape[0], int(niter), int(seed),
                                          int(max_points_per_centroid)), build_time=True)
        self.is_trained = True

    def set_codebooks(self, codebooks: np.ndarray) -> None:
        c = _ffi.as_f32_c(codebooks)
        if c.shape != (self.M, 256, self.dsub):
            raise ValueError(f"expected ({self.M}, 256, {self.dsub}) codebooks, got {c.shape}")
        _ffi.check(self._lib.vdb_pq_set_codebooks(self._handle(), self.M, _ffi.ptr(c)), build_time=True)
        self.is_trained = True

    def codebooks(self) -> np.ndarray:
        m = ctypes.c_int(0)
        out = np.empty((self.M, 256, self.dsub), np.float32)
        _ffi.check(self._lib.vdb_pq_get_codebooks(self._handle(), ctypes.byref(m), None))
        if m.value != self.M:
            raise RuntimeError("no codebooks: train the index or set them first")
        _ffi.check(self._lib.vdb_pq_get_codebooks(self._handle(), ctypes.byref(m), _ffi.ptr(out)))
        return out

    # -- rows -----------------------------------------------------------------------------------------------
    def add(self, x: np.ndarray, id_base: int = 0) -> None:
        """Encode and append rows (faiss.Index.add; same `id_base` on every add of one index, `reset()` empties it)."""
        x = _ffi.as_f32_c(x)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected (n, {self.dim}) vectors, got {x.shape}")
        try:
            _ffi.check(self._lib.vdb_pq_add(self._handle(), _ffi.ptr(x), x.shape[0], int(id_base)), build_time=True)
        finally:
            self._sync_ntotal()

    def add_codes(self, codes: np.ndarray, id_base: int = 0) -> None:
        """Append rows given as codes, uint8 (n, M): what loading a persisted index does."""
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        if c.ndim != 2 or c.shape[1] != self.M:
            raise ValueError(f"expected (n, {self.M}) codes, got {c.shape}")
        try:
            _ffi.check(self._lib.vdb_pq_add_codes(self._handle(), _ffi.ptr(c), c.shape[0], int(id_base)), build_time=True)
        finally:
            self._sync_ntotal()

    def codes(self) -> np.ndarray:
        """uint8 (ntotal, M) codes in id (insertion) order."""
        out = np.empty((self.ntotal, self.M), np.uint8)
        _ffi.check(self._lib.vdb_pq_get_codes(self._handle(), _ffi.ptr(out)))
        return out

    def reconstruct(self, codes: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 (n, dim) rows x^ of `codes` (default: every indexed row): codebook[m][code[m]] side by side, a lookup."""
        c = self.codes() if codes is None else np.asarray(codes, dtype=np.uint8)
        cb = self.codebooks()
        return np.ascontiguousarray(np.concatenate([cb[m][c[:, m]] for m in range(self.M)], axis=1), dtype=np.float32)

    def reset(self) -> None:
        """Drop every row; the codebooks stay (faiss.IndexPQ.reset)."""
        _ffi.check(self._lib.vdb_reset(self._handle()), build_time=True)
        self.ntotal = 0

    # -- search ---------------------------------------------------------------------------------------------
    def search(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _ffi.as_f32_c(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise RuntimeError(f"expected (nq, {self.dim}) queries, got {q.shape}")
        D = np.empty((q.shape[0], k), np.float32)
        I = np.empty((q.shape[0], k), np.int64)
        _ffi.check(self._lib.vdb_search(self._handle(), _ffi.ptr(q), q.shape[0], int(k), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def search_device(self, q_ptr: int, nq: int, k: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """All pointers are device memory on this index's GPU; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_search_device(self._handle(), q_ptr, int(nq), int(k), d_ptr, i_ptr, stream or None))

    def search_partial_device(self, q_ptr: int, nq: int, k: int, keys_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        """Partial top-k (float64 order keys + ids, device pointers), as FlatIndex.search_partial_device."""
        _ffi.check(self._lib.vdb_search_partial_device(self._handle(), q_ptr, int(nq), int(k), keys_ptr, ids_ptr, stream or None))

    def rerank(self, queries: np.ndarray, candidate_ids: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _ffi.as_f32_c(queries)
        c = np.ascontiguousarray(candidate_ids, dtype=np.int64)
        D = np.empty((q.shape[0], k), np.float32)
        I = np.empty((q.shape[0], k), np.int64)
        _ffi.check(self._lib.vdb_rerank(self._handle(), _ffi.ptr(q), q.shape[0], _ffi.ptr(c), c.shape[1], int(k), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I


def _build_pq(vectors: np.ndarray, dim: int, key: str, metric: str, device, params: dict) -> PQIndex:
    index = PQIndex(dim, parse_pq_key(key), metric, device)
    apply_engine_options(index, params)
    index.train(vectors, niter=int(params.get("niter", 25)), seed=int(params.get("seed", 1234)),
                max_points_per_centroid=int(params.get("max_points_per_centroid", 256)))
    index.add(vectors)
    return index


class HipPQIndexer(BaseIndexer):
    """FaissFactoryIndexer semantics for a "PQ<M>" key: cosine = normalise + inner product, `seed` for the k-means."""

    def __init__(self, name: str, dimension: int, metric: str = "l2", index_type: Optional[str] = None,
                 index_key: Optional[str] = None, **kwargs: Any) -> None:
        key = index_key or index_type or "PQ8"
        params = dict(kwargs)
        params.setdefault("index_type", key)
        super().__init__(name, dimension, metric, **params)
        self.index_key = self.index_type = key
        m = parse_pq_key(key)
        if dimension % m or m > min(dimension, 256):
            raise ValueError(f"PQ{m} needs a dimension that is a multiple of {m} (and M <= 256); got {dimension}")

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected dimension {self.dimension}, got {vectors.shape[1]}")
        data = _ffi.as_f32_c(vectors)
        meta = {"metric": self.metric, "index_key": self.index_key, "faiss_metric": "l2"}
        metric = "l2"
        if self.metric == "cosine":
            data = _safe_normalize(data)
            metric = "ip"
            meta.update({"faiss_metric": "ip", "normalize_queries": True, "normalize_vectors": True})
        elif self.metric == "ip":
            metric = "ip"
            meta["faiss_metric"] = "ip"
        device = _resolve_device(self.params.get("device"), self.params.get("device_ids"))
        index = _build_pq(data, self.dimension, self.index_key, metric, device, self.params)
        reserve_workspace(index, self.params)
        return IndexArtifact(kind="hip_pq", data=index, metadata=meta)


class HipPQSearcher(BaseSearcher):
    """FaissSearcher semantics over a HipPQIndexer artifact (distances negated for cosine / ip, as HipIVFSearcher)."""

    def __init__(self, name: str, dimension: int, metric: str = "l2", **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, **kwargs)
        self.index: Optional[PQIndex] = None
        self.normalize_queries = False

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        if artifact.kind != "hip_pq":
            raise ValueError("HipPQSearcher requires 'hip_pq' artifact")
        self.index = artifact.data
        meta = artifact.metadata or {}
        self.metric = meta.get("metric", self.metric)
        self.normalize_queries = meta.get("normalize_queries", False)
        self._prepared = True

    def _prepare_query(self, query: np.ndarray) -> np.ndarray:
        query = np.asarray(query)
        if query.ndim == 1:
            query = query.reshape(1, -1)
        query = query.astype(np.float32, copy=True)
        return _safe_normalize(query) if self.normalize_queries else query

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        d, i = self.batch_search(self._prepare_query(query), k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        if not self._prepared:
            raise RuntimeError("FaissSearcher not attached to an index")
        d, i = self.index.search(self._prepare_query(queries), k)
        if self.metric in {"cosine", "ip"}:
            d = -d
        return d.astype(np.float32), i.astype(np.int64)

    def get_memory_usage(self) -> float:
        return self.index.stats()["bytes_resident"] / (1024.0 * 1024.0) if self.index else 0.0


class HipPQSearch(BaseAlgorithm):
    """ApproximateSearch semantics for `index_type="PQ<M>"`: train -> add; raw FAISS conventions (no normalisation, no sign
    flip: 'l2' -> squared L2, anything else -> raw inner product)."""

    _FORMAT = "vdbhip-pq-v1"

    def __init__(self, name: str, dimension: int, index_type: str = "PQ8", metric: str = "l2", device: Optional[int] = None,
                 **kwargs: Any) -> None:
        super().__init__(name, dimension, **kwargs)
        self.index_type = index_type
        self.metric = "l2" if metric == "l2" else "ip"
        self.device = _resolve_device(device, kwargs.get("device_ids"))
        self.index: Optional[PQIndex] = None
        m = parse_pq_key(index_type)                          # fail at construction, like a bad factory string
        if dimension % m or m > min(dimension, 256):
            raise ValueError(f"PQ{m} needs a dimension that is a multiple of {m} (and M <= 256); got {dimension}")
        if isinstance(self.device, list):
            raise ValueError("PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available")

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        data = np.asarray(vectors).astype(np.float32)
        self.index = _build_pq(data, self.dimension, self.index_type, self.metric, self.device, self.config)
        self.index_built = True
        reserve_workspace(self.index, self.config)

    def search(self, query: np.ndarray, k: int = 10) -> SearchResult:
        if not self.index_built:
            raise RuntimeError("Index has not been built yet.")
        d, i = self.index.search(np.array([query], dtype=np.float32), k)
        return d[0], i[0]

    def batch_search(self, queries: np.ndarray, k: int = 10) -> SearchResult:
        if not self.index_built:
            raise RuntimeError("Index has not been built yet.")
        return self.index.search(np.asarray(queries).astype(np.float32), k)

    def get_memory_usage(self) -> float:
        return self.index.stats()["bytes_resident"] / (1024.0 * 1024.0) if self.index else 0.0

    # ---- persistence (protocol of HipApproximateSearch: temp dir + manifest + WRITE_COMPLETE last + atomic rename) ----------
    # A PQ artifact is the index itself: codebooks, codes and id_base.  No corpus file -- the index holds no float32 rows.
    def save_index(self, artifact_dir: str, context=None):
        import hashlib
        import json
        import shutil
        import tempfile
        from pathlib import Path

        if not self.index_built or self.index is None:
            raise RuntimeError("Cannot persist HipPQSearch before build_index has completed.")
        context = context or {}
        target = Path(artifact_dir)
        target.parent.mkdir(parents=True, exist_ok=True)
        if target.exists():
            if not bool(context.get("force_rebuild", False)):
                raise FileExistsError(f"Artifact directory already exists: {target}. "
                                      "Set persistence.force_rebuild=true to overwrite.")
            shutil.rmtree(target)
        tmp = Path(tempfile.mkdtemp(prefix=f".{target.name}.tmp.", dir=str(target.parent)))
        try:
            codebooks, codes = self.index.codebooks(), self.index.codes()
            np.save(tmp / "codebooks.npy", codebooks, allow_pickle=False)
            np.save(tmp / "codes.npy", codes, allow_pickle=False)
            build_metrics = dict(context.get("build_metrics", {}))
            manifest = {"format": self._FORMAT, "algorithm": type(self).__name__, "dimension": self.dimension,
                        "index_type": self.index_type, "metric": self.metric, "M": self.index.M, "id_base": 0,
                        "n_vectors": int(self.index.ntotal), "config_hash": context.get("config_hash"),
                        "sha256": {"codebooks": hashlib.sha256(codebooks.tobytes()).hexdigest(),
                                   "codes": hashlib.sha256(codes.tobytes()).hexdigest()},
                        "files": {"codebooks": "codebooks.npy", "codes": "codes.npy"}}
            (tmp / "manifest.json").write_text(json.dumps(manifest, indent=2), encoding="utf-8")
            (tmp / "build_metrics.json").write_text(json.dumps(build_metrics, indent=2), encoding="utf-8")
            (tmp / "WRITE_COMPLETE").write_text("ok\n", encoding="utf-8")
            tmp.rename(target)
        except Exception:
            shutil.rmtree(tmp, ignore_errors=True)
            raise
        return {"artifact_dir": str(target), "manifest_path": str(target / "manifest.json"),
                "build_time_s": float(build_metrics.get("build_time_s", 0.0) or 0.0)}

    def load_index(self, artifact_dir: str, context=None):
        import hashlib
        import json
        from pathlib import Path

        path = Path(artifact_dir)
        if not path.is_dir():
            raise FileNotFoundError(f"Persisted HipPQSearch artifact directory not found: {path}")
        if not (path / "WRITE_COMPLETE").is_file():
            raise FileNotFoundError(f"Artifact is incomplete or corrupted (missing WRITE_COMPLETE): {path}")
        manifest = json.loads((path / "manifest.json").read_text(encoding="utf-8"))
        for key, want in (("format", self._FORMAT), ("dimension", self.dimension), ("index_type", self.index_type),
                          ("metric", self.metric)):
            if manifest.get(key) != want:
                raise ValueError(f"Persisted index mismatch for '{key}': artifact has {manifest.get(key)!r}, "
                                 f"this instance expects {want!r}")
        expected_hash = (context or {}).get("config_hash")
        if expected_hash and manifest.get("config_hash") and manifest["config_hash"] != expected_hash:
            raise ValueError("Persisted index was built with a different configuration (config_hash mismatch)")
        codebooks = np.load(path / manifest["files"]["codebooks"])
        codes = np.load(path / manifest["files"]["codes"])
        m = parse_pq_key(self.index_type)
        if codebooks.shape != (m, 256, self.dimension // m) or codes.ndim != 2 or codes.shape[1] != m or codes.dtype != np.uint8 \
                or codes.shape[0] != int(manifest.get("n_vectors", codes.shape[0])):
            raise ValueError("Persisted PQ files do not match the manifest")
        want = manifest.get("sha256") or {}
        for name, arr in (("codebooks", codebooks), ("codes", codes)):
            if want.get(name) and hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest() != want[name]:
                raise ValueError(f"Persisted index files do not belong together (fingerprint mismatch: {name})")
        self.index = PQIndex(self.dimension, m, self.metric, self.device)
        apply_engine_options(self.index, self.config)
        self.index.set_codebooks(codebooks)           # no k-means and no encoding pass: the stored index is reused
        self.index.add_codes(codes, id_base=int(manifest.get("id_base", 0)))
        self.index_built = True
        metrics = {}
        bm = path / "build_metrics.json"
        if bm.is_file():
            metrics = json.loads(bm.read_text(encoding="utf-8"))
        return {"artifact_dir": str(path), "manifest_path": str(path / "manifest.json"),
                "build_time_s": float(metrics.get("build_time_s", 0.0) or 0.0)}


register_algorithm("HipPQSearch", HipPQSearch)
register_indexer("HipPQIndexer", HipPQIndexer)
register_searcher("HipPQSearcher", HipPQSearcher)

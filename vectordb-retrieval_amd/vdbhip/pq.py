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
from typing import Any, Optional

import numpy as np

from . import _ffi, persist
from .index import _FlatSearch, metric_code, one_device
from .algorithms import (FaissStyleSearcher, RawAlgorithm, _resolve_device, apply_engine_options, indexer_operands,
                         reserve_workspace)
from .plugin_api import BaseIndexer, IndexArtifact, Metadata, register_algorithm, register_indexer, register_searcher

_PQ_KEY = re.compile(r"^\s*PQ(\d+)(?:x8)?\s*$")
_ONE_GPU = "PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available"


def parse_pq_key(key: str) -> int:
    """M of a "PQ<M>" / "PQ<M>x8" key; every other key (any other bit width included) raises ValueError."""
    m = _PQ_KEY.match(str(key))
    if not m or int(m.group(1)) < 1:
        raise ValueError(f"unsupported index key {key!r}: only 'PQ<M>' (8 bits per sub-vector) is implemented here")
    return int(m.group(1))


def check_m(dim: int, M: int) -> None:
    if M < 1 or M > min(dim, 256) or dim % M:
        raise ValueError(f"M must divide dim and lie in [1, min(dim, 256)]; got dim={dim}, M={M}")


def check_key_dimension(dimension: int, m: int) -> None:
    """A plugin's constructor-time refusal of a "PQ<m>" codec the dimension does not admit (as a bad factory string fails)."""
    if dimension % m or m > min(dimension, 256):
        raise ValueError(f"PQ{m} needs a dimension that is a multiple of {m} (and M <= 256); got {dimension}")


class PQCodec:
    """What PQIndex and ivf_pq.IVFPQIndex share: the codebooks and codes of a product quantizer (self.M, self.dsub) behind
    the entry points `_pq_prefix` + set_codebooks / get_codebooks / get_codes."""

    _pq_prefix = "vdb_pq_"

    def _pq_call(self, name: str):
        return getattr(self._lib, self._pq_prefix + name)

    def set_codebooks(self, codebooks: np.ndarray) -> None:
        c = _ffi.as_f32_c(codebooks)
        if c.shape != (self.M, 256, self.dsub):
            raise ValueError(f"expected ({self.M}, 256, {self.dsub}) codebooks, got {c.shape}")
        _ffi.check(self._pq_call("set_codebooks")(self._handle(), self.M, _ffi.ptr(c)), build_time=True)

    def codebooks(self) -> np.ndarray:
        m = ctypes.c_int(0)
        _ffi.check(self._pq_call("get_codebooks")(self._handle(), ctypes.byref(m), None))
        if m.value != self.M:
            raise RuntimeError("no codebooks: train the index or set them first")
        out = np.empty((self.M, 256, self.dsub), np.float32)
        _ffi.check(self._pq_call("get_codebooks")(self._handle(), ctypes.byref(m), _ffi.ptr(out)))
        return out

    def codes(self) -> np.ndarray:
        """uint8 (ntotal, M) codes in id (insertion) order."""
        out = np.empty((self.ntotal, self.M), np.uint8)
        _ffi.check(self._pq_call("get_codes")(self._handle(), _ffi.ptr(out)))
        return out

    def lookup(self, codes: np.ndarray) -> np.ndarray:
        """float32 (n, dim): codebook[m][code[m]] side by side -- what reconstruct() starts from."""
        cb = self.codebooks()
        return np.ascontiguousarray(np.concatenate([cb[m][codes[:, m]] for m in range(self.M)], axis=1), dtype=np.float32)


class PQIndex(PQCodec, _FlatSearch):
    """Device-resident PQ<M> index (replaces faiss.IndexPQ(d, M, 8)).  One GPU only.  `adc_max_batch`: option
    "pq_adc_max_batch" -- query batches up to that size (at most 512; 0 = off) take the lookup-table (ADC) scan of the codes."""

    def __init__(self, dim: int, M: int, metric: str = "l2", device=0, adc_max_batch: int = 0):
        code = metric_code(metric)
        device = one_device(device, _ONE_GPU)
        dim, M = int(dim), int(M)
        check_m(dim, M)
        self.dim, self.M, self.dsub, self.metric, self.device = dim, M, dim // M, metric, device
        super().__init__(self.dim, code, self.device)
        self.is_trained = False
        self.ntotal = 0
        self.adc_max_batch = int(adc_max_batch or 0)
        if self.adc_max_batch:
            self.set_option("pq_adc_max_batch", float(self.adc_max_batch))

    # -- codebooks ----------------------------------------------------------------------------------------
    def train(self, x: np.ndarray, niter: int = 25, seed: int = 1234, max_points_per_centroid: int = 256) -> None:
        x = self._rows(x)
        _ffi.check(self._lib.vdb_pq_train(self._handle(), self.M, _ffi.ptr(x), x.shape[0], int(niter), int(seed),
                                          int(max_points_per_centroid)), build_time=True)
        self.is_trained = True

    def set_codebooks(self, codebooks: np.ndarray) -> None:
        super().set_codebooks(codebooks)
        self.is_trained = True

    # -- rows -----------------------------------------------------------------------------------------------
    def add(self, x: np.ndarray, id_base: int = 0) -> None:
        """Encode and append rows (faiss.Index.add; same `id_base` on every add of one index, `reset()` empties it)."""
        x = self._rows(x)
        try:
            _ffi.check(self._lib.vdb_pq_add(self._handle(), _ffi.ptr(x), x.shape[0], int(id_base)), build_time=True)
        finally:
            self._sync_ntotal()

    def add_codes(self, codes: np.ndarray, id_base: int = 0) -> None:
        """Append rows given as codes, uint8 (n, M): what loading a persisted index does."""
        c = self._codes(codes)
        try:
            _ffi.check(self._lib.vdb_pq_add_codes(self._handle(), _ffi.ptr(c), c.shape[0], int(id_base)), build_time=True)
        finally:
            self._sync_ntotal()

    def reconstruct(self, codes: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 (n, dim) rows x^ of `codes` (default: every indexed row): codebook[m][code[m]] side by side, a lookup."""
        return self.lookup(self.codes() if codes is None else np.asarray(codes, dtype=np.uint8))

    def debug_adc_scores(self, queries: np.ndarray, row0: int, nrows: int):
        """(scores (nq, nrows), eps (nq), cs) of the lookup-table (ADC) scan: raw, unpacked scores, as FlatIndex.debug_scan_scores.
        Indexes with rows only."""
        return self._debug_scores(self._lib.vdb_debug_pq_adc_scores, queries, nrows, int(row0), int(nrows))


def _build_pq(vectors: np.ndarray, dim: int, key: str, metric: str, device, params: dict) -> PQIndex:
    index = PQIndex(dim, parse_pq_key(key), metric, device, adc_max_batch=int(params.get("adc_max_batch") or 0))
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
        check_key_dimension(dimension, parse_pq_key(key))

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected dimension {self.dimension}, got {vectors.shape[1]}")
        data, metric, entries = indexer_operands(vectors, self.metric)
        meta = {"metric": self.metric, "index_key": self.index_key, **entries}
        device = _resolve_device(self.params.get("device"), self.params.get("device_ids"))
        index = _build_pq(data, self.dimension, self.index_key, metric, device, self.params)
        reserve_workspace(index, self.params)
        return IndexArtifact(kind="hip_pq", data=index, metadata=meta)


class HipPQSearcher(FaissStyleSearcher):
    """FaissSearcher semantics over a HipPQIndexer artifact (distances negated for cosine / ip, as HipIVFSearcher).
    `adc_max_batch` (a config entry `adc_max_batch: 16`): option "pq_adc_max_batch" of the attached index."""

    _kind = "hip_pq"

    def __init__(self, name: str, dimension: int, metric: str = "l2", adc_max_batch: Optional[int] = None, **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, **kwargs)
        self.adc_max_batch = None if adc_max_batch is None else int(adc_max_batch)

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        self._bind(artifact)
        if self.adc_max_batch is not None:
            self.index.set_option("pq_adc_max_batch", float(self.adc_max_batch))
            self.index.adc_max_batch = self.adc_max_batch
        self._prepared = True


class HipPQSearch(RawAlgorithm):
    """ApproximateSearch semantics for `index_type="PQ<M>"`: train -> add; raw FAISS conventions (no normalisation, no sign
    flip: 'l2' -> squared L2, anything else -> raw inner product)."""

    _FORMAT = "vdbhip-pq-v1"

    def __init__(self, name: str, dimension: int, index_type: str = "PQ8", metric: str = "l2", device: Optional[int] = None,
                 adc_max_batch: int = 0, **kwargs: Any) -> None:
        super().__init__(name, dimension, **kwargs)
        self.index_type = index_type
        self.adc_max_batch = int(adc_max_batch or 0)      # option "pq_adc_max_batch": a constructor parameter, not part of the artifact
        self.metric = "l2" if metric == "l2" else "ip"
        self.device = _resolve_device(device, kwargs.get("device_ids"))
        self.index: Optional[PQIndex] = None
        check_key_dimension(dimension, parse_pq_key(index_type))       # fail at construction, like a bad factory string
        one_device(self.device, _ONE_GPU)

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        data = np.asarray(vectors).astype(np.float32)
        self.index = _build_pq(data, self.dimension, self.index_type, self.metric, self.device,
                               {**self.config, "adc_max_batch": self.adc_max_batch})
        self.index_built = True
        reserve_workspace(self.index, self.config)

    # ---- persistence (persist.py: temp dir + manifest + WRITE_COMPLETE last + atomic rename) ------------------------------------
    # A PQ artifact is the index itself: codebooks, codes and id_base.  No corpus file -- the index holds no float32 rows.
    def save_index(self, artifact_dir: str, context=None):
        if not self.index_built or self.index is None:
            raise RuntimeError("Cannot persist HipPQSearch before build_index has completed.")
        manifest = {"format": self._FORMAT, "algorithm": type(self).__name__, "dimension": self.dimension,
                    "index_type": self.index_type, "metric": self.metric, "M": self.index.M, "id_base": 0,
                    "n_vectors": int(self.index.ntotal)}
        return persist.write_artifact(artifact_dir, context, manifest,
                                      {"codebooks": self.index.codebooks(), "codes": self.index.codes()})

    def load_index(self, artifact_dir: str, context=None):
        manifest, load, result = persist.read_artifact(artifact_dir, context, "HipPQSearch", format=self._FORMAT,
                                                       dimension=self.dimension, index_type=self.index_type, metric=self.metric)
        codebooks, codes = load("codebooks"), load("codes")
        m = parse_pq_key(self.index_type)
        if codebooks.shape != (m, 256, self.dimension // m) or codes.ndim != 2 or codes.shape[1] != m or codes.dtype != np.uint8 \
                or codes.shape[0] != int(manifest.get("n_vectors", codes.shape[0])):
            raise ValueError("Persisted PQ files do not match the manifest")
        persist.check_sha256(manifest, {"codebooks": codebooks, "codes": codes})
        self.index = PQIndex(self.dimension, m, self.metric, self.device, adc_max_batch=self.adc_max_batch)
        apply_engine_options(self.index, self.config)
        self.index.set_codebooks(codebooks)           # no k-means and no encoding pass: the stored index is reused
        self.index.add_codes(codes, id_base=int(manifest.get("id_base", 0)))
        self.index_built = True
        return result


register_algorithm("HipPQSearch", HipPQSearch)
register_indexer("HipPQIndexer", HipPQIndexer)
register_searcher("HipPQSearcher", HipPQSearcher)

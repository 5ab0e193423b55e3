"""IVF<nlist>,PQ<M> on the MI355X behind the reference's `FaissFactoryIndexer index_key: IVF...,PQ...` entries.

  HipIVFPQIndexer   drop-in for FaissFactoryIndexer with an "IVF<nlist>,PQ<M>" key   (src/algorithms/modular.py:224-309);
                    its artifact is the 'hip_ivf' one HipIVFSearcher attaches to (searcher `nprobe` override, cosine =
                    normalise + inner product, distances negated for cosine / ip)
  HipIVFPQSearch    BaseAlgorithm form for `type:` entries (`index_type="IVF256,PQ64"`), raw conventions of
                    HipApproximateSearch, with save_index / load_index

The inverted lists hold 8-bit product codes of the residuals x - c_l: M bytes per row, no float32 rows.  A search returns,
bit for bit, the IVF-Flat result of this library over the decoded rows x^ = c_l + codebook entries under the same lists and
nprobe (include/vdbhip.h, vdb_ivfpq_*).  FAISS' k-means, its float32 table sums and its order among equal distances are not
reproduced: centroids and codebooks come from the library's own k-means (FAISS' defaults: 25 iterations, at most 256
training points per centroid) and ties go to the smaller id.

The IVF and flat-PQ parsers and classes (parse_index_key, parse_ivf_key, parse_pq_key, HipApproximateSearch, HipIVFIndexer,
HipPQSearch) keep refusing these keys: the codec lives behind the names of this module only.
"""
from __future__ import annotations

import re
from typing import Any, Optional, Tuple

import numpy as np

from . import _ffi, persist
from .index import one_device
from .algorithms import RawAlgorithm, _resolve_device, indexer_operands, reserve_workspace
from .ivf import IVFFlatIndex
from .pq import PQCodec, check_key_dimension, check_m
from .plugin_api import BaseIndexer, IndexArtifact, Metadata, register_algorithm, register_indexer

_IVFPQ_KEY = re.compile(r"^\s*IVF(\d+)\s*,\s*PQ(\d+)(?:x8)?\s*$")
_ONE_GPU = "IVF<nlist>,PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available"


def parse_ivfpq_key(key: str) -> Tuple[int, int]:
    """(nlist, M) of an "IVF<nlist>,PQ<M>" / "IVF<nlist>,PQ<M>x8" key; every other key (any other bit width, OPQ, a flat
    "PQ<M>", the Flat and SQ8 codecs) raises ValueError."""
    m = _IVFPQ_KEY.match(str(key))
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"unsupported index key {key!r}: only 'IVF<nlist>,PQ<M>' (8 bits per sub-vector) is implemented here")
    return int(m.group(1)), int(m.group(2))


class IVFPQIndex(PQCodec, IVFFlatIndex):
    """Device-resident IVF<nlist>,PQ<M> index (replaces faiss.index_factory(d, "IVFn,PQm", metric)).  `train` fits the
    centroids and then the codebooks of the residuals on the same rows; `set_centroids` + `train_codebooks` /
    `set_codebooks` inject them instead.  One GPU only.  `adc_max_batch`: option "ivfpq_adc_max_batch" -- query batches up to that
    size (at most 512; 0 = off) take the lookup-table (ADC) scan of the probed lists; same results."""

    _pq_prefix = "vdb_ivfpq_"

    def __init__(self, dim: int, nlist: int, M: int, metric: str = "l2", device=0, adc_max_batch: int = 0):
        one_device(device, _ONE_GPU)
        check_m(int(dim), int(M))
        super().__init__(dim, nlist, metric, device)
        self.M, self.dsub = int(M), int(dim) // int(M)
        _ffi.check(self._lib.vdb_ivf_set_codec(self._handle(), 2), build_time=True)
        self.adc_max_batch = int(adc_max_batch or 0)
        if self.adc_max_batch:
            self.set_option("ivfpq_adc_max_batch", float(self.adc_max_batch))

    def debug_adc_scores(self, queries: np.ndarray, probe_list: int, row0: int, nrows: int):
        """(scores (nq, nrows) float32, eps (nq,) float32, cs): the ADC scan's own scores of the list-order rows [row0, row0 + nrows)
        of list `probe_list` for a batch of these queries (test hook)."""
        return self._debug_scores(self._lib.vdb_debug_ivfpq_adc_scores, queries, nrows, int(probe_list), int(row0), int(nrows))

    def train(self, x: np.ndarray, niter: int = 25, seed: int = 1234, max_points_per_centroid: int = 256) -> None:
        super().train(x, niter=niter, seed=seed, max_points_per_centroid=max_points_per_centroid)
        self.train_codebooks(x, niter=niter, seed=seed, max_points_per_centroid=max_points_per_centroid)

    def train_codebooks(self, x: np.ndarray, niter: int = 25, seed: int = 1234, max_points_per_centroid: int = 256) -> None:
        """Codebooks from the residuals of a row sample of `x` against the installed centroids."""
        x = self._rows(x)
        _ffi.check(self._lib.vdb_ivfpq_train(self._handle(), self.M, _ffi.ptr(x), x.shape[0], int(niter), int(seed),
                                             int(max_points_per_centroid)), build_time=True)
        self.ntotal = 0             # (new codebooks: rows encoded under the old ones are dropped)

    def set_codebooks(self, codebooks: np.ndarray) -> None:
        super().set_codebooks(codebooks)
        self.ntotal = 0

    def add_codes(self, codes: np.ndarray, list_of_row: np.ndarray, id_base: int = 0) -> None:
        """Append rows given as codes, uint8 (n, M), under the given lists: what loading a persisted index does."""
        c = self._codes(codes)
        lor = self._list_ids(list_of_row, c.shape[0])
        try:
            _ffi.check(self._lib.vdb_ivfpq_add_codes(self._handle(), _ffi.ptr(c), c.shape[0], int(id_base), _ffi.ptr(lor)),
                       build_time=True)
        finally:
            self._sync_ntotal()

    def reconstruct(self) -> np.ndarray:
        """float32 (ntotal, dim) rows x^ in id order: centroid of the row's list + codebook entries, one float32 add."""
        return np.ascontiguousarray(self.centroids()[self.assignment()] + self.lookup(self.codes()), dtype=np.float32)


def _build_ivfpq(vectors: np.ndarray, dim: int, key: str, metric: str, device, params: dict) -> IVFPQIndex:
    nlist, M = parse_ivfpq_key(key)
    index = IVFPQIndex(dim, nlist, M, metric, device, adc_max_batch=int(params.get("adc_max_batch") or 0))
    index.train(vectors, niter=int(params.get("niter", 25)), seed=int(params.get("seed", 1234)),
                max_points_per_centroid=int(params.get("max_points_per_centroid", 256)))
    index.add(vectors)
    return index


def _check_key(dimension: int, key: str, device) -> Tuple[int, int]:
    nlist, m = parse_ivfpq_key(key)
    check_key_dimension(dimension, m)
    one_device(device, _ONE_GPU)
    return nlist, m


class HipIVFPQIndexer(BaseIndexer):
    """FaissFactoryIndexer semantics for an "IVF<nlist>,PQ<M>" key; the artifact is HipIVFSearcher's ('hip_ivf').
    `adc_max_batch` (a config entry `adc_max_batch: 16`): option "ivfpq_adc_max_batch" of the index it builds."""

    def __init__(self, name: str, dimension: int, metric: str = "l2", index_type: Optional[str] = None,
                 index_key: Optional[str] = None, adc_max_batch: int = 0, **kwargs: Any) -> None:
        key = index_key or index_type or "IVF100,PQ8"
        params = dict(kwargs)
        params.setdefault("index_type", key)
        params["adc_max_batch"] = int(adc_max_batch or 0)
        super().__init__(name, dimension, metric, **params)
        self.adc_max_batch = int(adc_max_batch or 0)
        self.index_key = self.index_type = key
        _check_key(dimension, key, _resolve_device(self.params.get("device"), self.params.get("device_ids")))

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        if vectors.shape[1] != self.dimension:
            raise ValueError(f"Expected dimension {self.dimension}, got {vectors.shape[1]}")
        data, metric, entries = indexer_operands(vectors, self.metric)
        meta = {"metric": self.metric, "index_key": self.index_key, **entries}
        device = _resolve_device(self.params.get("device"), self.params.get("device_ids"))
        index = _build_ivfpq(data, self.dimension, self.index_key, metric, device, self.params)
        if "nprobe" in self.params:                       # runtime attribute of the index (modular.py:269-275)
            index.set_nprobe(int(self.params["nprobe"]))
            meta["nprobe"] = self.params["nprobe"]
        reserve_workspace(index, self.params)
        return IndexArtifact(kind="hip_ivf", data=index, metadata=meta)


class HipIVFPQSearch(RawAlgorithm):
    """ApproximateSearch semantics for `index_type="IVF<nlist>,PQ<M>"`: train -> add -> nprobe from kwargs; raw FAISS
    conventions (no normalisation, no sign flip: 'l2' -> squared L2, anything else -> raw inner product)."""

    _FORMAT = "vdbhip-ivfpq-v1"

    def __init__(self, name: str, dimension: int, index_type: str = "IVF100,PQ8", metric: str = "l2",
                 device: Optional[int] = None, adc_max_batch: int = 0, **kwargs: Any) -> None:
        super().__init__(name, dimension, **kwargs)
        self.adc_max_batch = int(adc_max_batch or 0)      # option "ivfpq_adc_max_batch": a constructor parameter, not part of the artifact
        self.index_type = index_type
        self.metric = "l2" if metric == "l2" else "ip"
        self.device = _resolve_device(device, kwargs.get("device_ids"))
        self.index: Optional[IVFPQIndex] = None
        _check_key(dimension, index_type, self.device)        # fail at construction, like a bad factory string

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        data = np.asarray(vectors).astype(np.float32)
        self.index = _build_ivfpq(data, self.dimension, self.index_type, self.metric, self.device,
                                  {**self.config, "adc_max_batch": self.adc_max_batch})
        self.index_built = True
        if "nprobe" in self.config:
            self.index.set_nprobe(int(self.config["nprobe"]))
        reserve_workspace(self.index, self.config)

    # ---- persistence (persist.py: temp dir + manifest + WRITE_COMPLETE last + atomic rename) ------------------------------------
    # An IVF-PQ artifact is the index itself: centroids, codebooks, codes and the list of every row.  No corpus file -- the
    # index holds no float32 rows -- and loading neither clusters nor encodes.
    _FILES = ("centroids", "codebooks", "codes", "list_of_row")

    def save_index(self, artifact_dir: str, context=None):
        if not self.index_built or self.index is None:
            raise RuntimeError("Cannot persist HipIVFPQSearch before build_index has completed.")
        manifest = {"format": self._FORMAT, "algorithm": type(self).__name__, "dimension": self.dimension,
                    "index_type": self.index_type, "metric": self.metric, "nlist": self.index.nlist, "M": self.index.M,
                    "nprobe": self.index.nprobe, "id_base": 0, "n_vectors": int(self.index.ntotal)}
        arrays = {"centroids": self.index.centroids(), "codebooks": self.index.codebooks(), "codes": self.index.codes(),
                  "list_of_row": self.index.assignment()}
        return persist.write_artifact(artifact_dir, context, manifest, arrays)

    def load_index(self, artifact_dir: str, context=None):
        manifest, load, result = persist.read_artifact(artifact_dir, context, "HipIVFPQSearch", format=self._FORMAT,
                                                       dimension=self.dimension, index_type=self.index_type, metric=self.metric)
        nlist, m = parse_ivfpq_key(self.index_type)
        arrays = {name: load(name) for name in self._FILES}
        n = int(manifest.get("n_vectors", arrays["codes"].shape[0]))
        lists = arrays["list_of_row"]
        if arrays["centroids"].shape != (nlist, self.dimension) or arrays["codebooks"].shape != (m, 256, self.dimension // m) \
                or arrays["codes"].shape != (n, m) or arrays["codes"].dtype != np.uint8 or lists.shape != (n,) \
                or (n and (lists.min() < 0 or lists.max() >= nlist)):
            raise ValueError("Persisted IVF-PQ files do not match the manifest")
        persist.check_sha256(manifest, arrays)
        self.index = IVFPQIndex(self.dimension, nlist, m, self.metric, self.device, adc_max_batch=self.adc_max_batch)
        self.index.set_centroids(arrays["centroids"])      # no k-means, no assignment and no encoding pass: the stored
        self.index.set_codebooks(arrays["codebooks"])      # index is reused as it is
        self.index.add_codes(arrays["codes"], lists, id_base=int(manifest.get("id_base", 0)))
        self.index.set_nprobe(int(self.config.get("nprobe", manifest.get("nprobe", 1))))
        self.index_built = True
        return result


register_algorithm("HipIVFPQSearch", HipIVFPQSearch)
register_indexer("HipIVFPQIndexer", HipIVFPQIndexer)

"""IVF-Flat and IVF-SQ8 on the MI355X behind the reference's three IVF entry points.

  HipApproximateSearch   drop-in for ApproximateSearch        (src/algorithms/approximate_search.py:6-87)
                         -- `index_type` keys of the form "IVF<nlist>,Flat" or "IVF<nlist>,SQ8" (PQ codecs are out of
                         scope); 'l2' -> squared L2, anything else -> raw inner product; no sign flips.
  HipIVFIndexer          drop-in for FaissFactoryIndexer / FaissIVFIndexer (modular.py:224-309)
                         -- cosine = normalise + inner product (:253-262), runtime `nprobe` (:269-275)
  HipIVFSearcher         drop-in for FaissSearcher on IVF artifacts (modular.py:393-449, 536-548)
                         -- searcher `nprobe` overrides the indexer's (:437-441), queries normalised when the
                         artifact says so (:447-448), distances negated for cosine/ip (:545-546).

k-means is this library's own Lloyd iteration (FAISS's is not reproducible without FAISS), defaults mirroring
FAISS: 25 iterations, seed 1234, at most 256 training points per centroid.
"""
from __future__ import annotations

import ctypes
import re
from typing import Any, Optional, Tuple

import numpy as np

from . import _ffi, persist
from .index import _Handle, _pair, metric_code, normalize_devices, one_device
from .algorithms import FaissStyleSearcher, RawAlgorithm, _resolve_device, indexer_operands, reserve_workspace
from .plugin_api import BaseIndexer, IndexArtifact, Metadata, register_algorithm, register_indexer, register_searcher

_IVF_KEY = re.compile(r"^\s*IVF(\d+)\s*,\s*Flat\s*$")
_IVF_CODEC_KEY = re.compile(r"^\s*IVF(\d+)\s*,\s*(Flat|SQ8)\s*$")


def parse_ivf_key(key: str) -> int:
    """nlist of an "IVF<nlist>,Flat" key (the row-sharded HipShardedApproximateSearch serves Flat lists only)."""
    m = _IVF_KEY.match(str(key))
    if not m:
        raise ValueError(f"unsupported index key {key!r}: only 'IVF<nlist>,Flat' is implemented on the HIP backend")
    return int(m.group(1))


def parse_index_key(key: str) -> Tuple[int, str]:
    """(nlist, codec) of "IVF<nlist>,Flat" / "IVF<nlist>,SQ8" (codec "Flat" or "SQ8"); every other key raises ValueError."""
    m = _IVF_CODEC_KEY.match(str(key))
    if not m:
        raise ValueError(f"unsupported index key {key!r}: only 'IVF<nlist>,Flat' and 'IVF<nlist>,SQ8' are implemented "
                         "on the HIP backend")
    return int(m.group(1)), m.group(2)


class IVFFlatIndex(_Handle):
    """Device-resident IVF-Flat index (replaces faiss.index_factory(d, "IVFn,Flat", metric))."""

    def __init__(self, dim: int, nlist: int, metric: str = "l2", device=0):
        """`device`: one GPU ordinal or a list of them (rows of every list split over those GPUs, coarse quantizer
        replicated: vdb_create_multi)."""
        code = metric_code(metric)
        self.dim, self.nlist, self.metric, self.device = int(dim), int(nlist), metric, normalize_devices(device)
        super().__init__(self.dim, code, self.device)
        self.is_trained = False
        self.ntotal = 0
        self.nprobe = 1
        self.id_base = 0

    def train(self, x: np.ndarray, niter: int = 25, seed: int = 1234, max_points_per_centroid: int = 256) -> None:
        x = self._rows(x)
        self._filter_key = None
        _ffi.check(self._lib.vdb_ivf_train(self._handle(), self.nlist, _ffi.ptr(x), x.shape[0], int(niter), int(seed),
                                           int(max_points_per_centroid)), build_time=True)
        self.is_trained = True
        self.ntotal = 0             # (new centroids: rows filed under the old ones are dropped)

    def set_centroids(self, centroids: np.ndarray) -> None:
        c = _ffi.as_f32_c(centroids)
        if c.shape != (self.nlist, self.dim):
            raise ValueError(f"expected ({self.nlist}, {self.dim}) centroids, got {c.shape}")
        self._filter_key = None
        _ffi.check(self._lib.vdb_ivf_set_centroids(self._handle(), _ffi.ptr(c), self.nlist), build_time=True)
        self.is_trained = True
        self.ntotal = 0

    def centroids(self) -> np.ndarray:
        out = np.empty((self.nlist, self.dim), np.float32)
        _ffi.check(self._lib.vdb_ivf_get_centroids(self._handle(), _ffi.ptr(out)))
        return out

    def add(self, x: np.ndarray, id_base: int = 0, list_of_row: Optional[np.ndarray] = None) -> None:
        """File the rows under the centroids, appending to the lists (faiss.IndexIVF.add; same `id_base` on every add of
        one index, `reset()` empties it).  `list_of_row` (int32, one list id per row, as `assignment()` returned it
        for this corpus and these centroids) skips the nearest-centroid pass: what loading a persisted index does."""
        x = self._rows(x)
        lor = None if list_of_row is None else self._list_ids(list_of_row, x.shape[0])
        self._filter_key = None
        try:
            if lor is None:
                _ffi.check(self._lib.vdb_ivf_add(self._handle(), _ffi.ptr(x), x.shape[0], int(id_base)), build_time=True)
            else:
                _ffi.check(self._lib.vdb_ivf_add_assigned(self._handle(), _ffi.ptr(x), x.shape[0], int(id_base), _ffi.ptr(lor)),
                           build_time=True)
            self.id_base = int(id_base)
        finally:
            self._sync_ntotal()

    @staticmethod
    def _list_ids(list_of_row: np.ndarray, n: int) -> np.ndarray:
        lor = np.ascontiguousarray(list_of_row, dtype=np.int32)
        if lor.shape != (n,):
            raise ValueError(f"expected {n} list ids, got {lor.shape}")
        return lor

    def assignment(self) -> np.ndarray:
        out = np.empty((self.ntotal,), np.int32)
        _ffi.check(self._lib.vdb_ivf_get_assignment(self._handle(), _ffi.ptr(out)))
        return out

    def set_nprobe(self, nprobe: int) -> None:
        _ffi.check(self._lib.vdb_ivf_set_nprobe(self._handle(), int(nprobe)), build_time=True)
        self.nprobe = int(nprobe)

    def search(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        q = self._queries(queries)
        D, I = _pair(q.shape[0], k)
        _ffi.check(self._lib.vdb_ivf_search(self._handle(), _ffi.ptr(q), q.shape[0], int(k), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def search_device(self, q_ptr: int, nq: int, k: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        _ffi.check(self._lib.vdb_ivf_search_device(self._handle(), q_ptr, int(nq), int(k), d_ptr, i_ptr, stream or None))

    def search_partial_device(self, q_ptr: int, nq: int, k: int, keys_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        """Per-shard partial top-k (float64 order keys + global ids) among the probed lists; device pointers."""
        _ffi.check(self._lib.vdb_ivf_search_partial_device(self._handle(), q_ptr, int(nq), int(k), keys_ptr, ids_ptr,
                                                           stream or None))

    # -- filtered search (vdb_ivf_filter_*, vdb_ivf_search_filtered): the k nearest rows among the admitted rows of the probed lists.
    #    IVF-Flat on one GPU; the library refuses the coded subclasses and a multi-device index, and the error comes through ----
    _filter_key = None       # (object, ntotal) of the filter `ensure_filter` installed last; any call that drops the filter clears it

    def set_filter(self, allowed, nbits: Optional[int] = None) -> None:
        """Install the rows a filtered search may return: a bool array of length ntotal (row numbers in insertion order over
        all adds, NOT list order), an integer array of ids (id_base + row; duplicates allowed, out of range raises ValueError),
        or packed uint32 words with `nbits=` (_ffi.pack_allow_bits).  Any add, reset, set_option, train or set_centroids drops
        the filter; set_nprobe keeps it."""
        self._filter_key = None
        words = _ffi.pack_allow_bits(allowed, self.ntotal, self.id_base, nbits)
        _ffi.check(self._lib.vdb_ivf_filter_set(self._handle(), _ffi.ptr(words), self.ntotal), build_time=True)

    def set_filter_device(self, words_ptr: int, nbits: int, stream: int = 0) -> None:
        """Packed uint32 words in device memory of this index's GPU; runs on `stream` and waits for it once."""
        self._filter_key = None
        _ffi.check(self._lib.vdb_ivf_filter_set_device(self._handle(), words_ptr, int(nbits), stream or None), build_time=True)

    def ensure_filter(self, allowed) -> None:
        """`set_filter(allowed)` unless that very object was installed last on these rows (identity and ntotal, not content)."""
        key = self._filter_key
        if key is not None and key[0] is allowed and key[1] == self.ntotal:
            return
        self.set_filter(allowed)
        self._filter_key = (allowed, self.ntotal)

    def clear_filter(self) -> None:
        self._filter_key = None
        _ffi.check(self._lib.vdb_filter_clear(self._handle()))

    @property
    def filter_count(self) -> int:
        """Rows the installed filter admits."""
        n = ctypes.c_int64(0)
        _ffi.check(self._lib.vdb_ivf_filter_count(self._handle(), ctypes.byref(n)))
        return int(n.value)

    def search_filtered(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """`search` among the admitted rows of the probed lists: same keys, order and padding (fewer than k admitted rows pad)."""
        q = self._queries(queries)
        D, I = _pair(q.shape[0], k)
        _ffi.check(self._lib.vdb_ivf_search_filtered(self._handle(), _ffi.ptr(q), q.shape[0], int(k), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def search_filtered_device(self, q_ptr: int, nq: int, k: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """All pointers are device memory on this index's GPU; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_ivf_search_filtered_device(self._handle(), q_ptr, int(nq), int(k), d_ptr, i_ptr, stream or None))

    # -- range search (vdb_ivf_range_*): every row of the probed lists within a radius, in list order per query.  IVF-Flat on one
    #    GPU; the library refuses the coded subclasses and a multi-device index, and the error comes through ----
    def range_search(self, queries: np.ndarray, radius: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(lims int64 (nq + 1,), D float32, I int64): query q owns entries [lims[q], lims[q + 1]) -- the rows of its `nprobe`
        probed lists with squared L2 distance < radius / inner product > radius (faiss.IndexIVFFlat.range_search), exact, in
        ascending (list, id)."""
        q = self._queries(queries)
        lims = np.empty((q.shape[0] + 1,), np.int64)
        _ffi.check(self._lib.vdb_ivf_range_search(self._handle(), _ffi.ptr(q), q.shape[0], float(np.float32(radius)), _ffi.ptr(lims)))
        D, I = np.empty((int(lims[-1]),), np.float32), np.empty((int(lims[-1]),), np.int64)
        _ffi.check(self._lib.vdb_ivf_range_results(self._handle(), _ffi.ptr(D), _ffi.ptr(I)))
        return lims, D, I

    def range_search_device(self, q_ptr: int, nq: int, radius: float, lims_ptr: int, stream: int = 0) -> int:
        """Device pointers on this index's GPU; waits for `stream` (the result size must reach the host) and returns
        lims[nq], the number of entries `range_results_device` will write."""
        total = ctypes.c_int64(0)
        _ffi.check(self._lib.vdb_ivf_range_search_device(self._handle(), q_ptr, int(nq), float(np.float32(radius)), lims_ptr,
                                                         ctypes.byref(total), stream or None))
        return int(total.value)

    def range_results_device(self, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """The (D, I) of the last range search of this index into device memory; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_ivf_range_results_device(self._handle(), d_ptr, i_ptr, stream or None))


class IVFSQ8Index(IVFFlatIndex):
    """Device-resident IVF<nlist>,SQ8 index (replaces faiss.index_factory(d, "IVFn,SQ8", metric): IndexIVFScalarQuantizer
    with 8-bit codes of the residuals, per-dimension min / max ranges).  One byte per dimension and no float32 rows; the
    results are exact over the decoded rows (include/vdbhip.h).  `train` fits the centroids and then the ranges on the same
    rows; `set_centroids` + `train_ranges` / `set_ranges` inject them instead.  One GPU only."""

    def __init__(self, dim: int, nlist: int, metric: str = "l2", device=0):
        one_device(device, "IVF<nlist>,SQ8 runs on one GPU: a multi-device index (more than one device id) is not "
                           "available for the SQ8 codec")
        super().__init__(dim, nlist, metric, device)
        _ffi.check(self._lib.vdb_ivf_set_codec(self._handle(), 1), build_time=True)

    def train_ranges(self, x: np.ndarray) -> None:
        """vmin / vdiff from the residuals of `x` against the installed centroids (at most 100 000 rows are read)."""
        x = self._rows(x)
        _ffi.check(self._lib.vdb_ivf_sq8_train_ranges(self._handle(), _ffi.ptr(x), x.shape[0]), build_time=True)
        self.ntotal = 0

    def set_ranges(self, vmin: np.ndarray, vdiff: np.ndarray) -> None:
        vmin = np.ascontiguousarray(vmin, dtype=np.float32).reshape(-1)
        vdiff = np.ascontiguousarray(vdiff, dtype=np.float32).reshape(-1)
        if vmin.shape != (self.dim,) or vdiff.shape != (self.dim,):
            raise ValueError(f"expected two ({self.dim},) range vectors, got {vmin.shape} and {vdiff.shape}")
        _ffi.check(self._lib.vdb_ivf_sq8_set_ranges(self._handle(), _ffi.ptr(vmin), _ffi.ptr(vdiff)), build_time=True)
        self.ntotal = 0

    def ranges(self) -> Tuple[np.ndarray, np.ndarray]:
        vmin = np.empty((self.dim,), np.float32)
        vdiff = np.empty((self.dim,), np.float32)
        _ffi.check(self._lib.vdb_ivf_sq8_get_ranges(self._handle(), _ffi.ptr(vmin), _ffi.ptr(vdiff)))
        return vmin, vdiff

    def codes(self) -> np.ndarray:
        """uint8 (ntotal, dim) codes in id (insertion) order."""
        out = np.empty((self.ntotal, self.dim), np.uint8)
        _ffi.check(self._lib.vdb_ivf_get_codes(self._handle(), _ffi.ptr(out)))
        return out


class IVFI8Index(IVFFlatIndex):
    """Device-resident IVF<nlist>,I8 index: IVF-Flat over a byte-valued corpus (every value an integer in 0..255, or every value
    an integer in -128..127 -- `is_byte_valued`) that keeps the rows as int8 only, losslessly (x = byte + cx): about 0.6 x the
    float32 bytes where IVF-Flat holds 2.8 - 4 x, and the IVF-Flat results bit for bit (include/vdbhip.h).  dim <= 128.  An add
    of rows that are not byte-valued raises and changes nothing.  One GPU only; no filtered or range search."""

    def __init__(self, dim: int, nlist: int, metric: str = "l2", device=0):
        one_device(device, "IVF<nlist>,I8 runs on one GPU: a multi-device index (more than one device id) is not "
                           "available for the IVF-I8 codec")
        super().__init__(dim, nlist, metric, device)
        _ffi.check(self._lib.vdb_ivf_set_codec(self._handle(), 3), build_time=True)

    def rows(self) -> Tuple[np.ndarray, int]:
        """(int8 (ntotal, dim) rows in id (insertion) order, cx): the corpus is `rows.astype(int) + cx`, exactly."""
        out = np.empty((self.ntotal, self.dim), np.int8)
        cx = ctypes.c_int(0)
        _ffi.check(self._lib.vdb_ivf_i8_get_rows(self._handle(), _ffi.ptr(out) if self.ntotal else None, ctypes.byref(cx)))
        return out, int(cx.value)


def is_byte_valued(x: np.ndarray) -> bool:
    """The byte test of the library (corpus_stats_kernel) in NumPy: every value a finite integer, and all of them in 0..255 or
    all of them in -128..127.  An empty array passes."""
    x = np.asarray(x)
    if x.size == 0:
        return True
    if not np.isfinite(x).all() or (x != np.rint(x)).any():
        return False
    lo, hi = float(x.min()), float(x.max())
    return (lo >= 0 and hi <= 255) or (lo >= -128 and hi <= 127)


def _fingerprint(vectors: np.ndarray, centroids: np.ndarray, list_of_row: np.ndarray) -> dict:
    """What a persisted index records about its three files so that load_index can tell a vectors / centroids file that
    does not belong to list_of_row.npy (regenerated corpus, partial overwrite): SHA-256 of the centroids and of the lists
    in full, and of up to 4096 evenly spaced corpus rows (hashing a memory-mapped 38 GB shard in full is not cheap)."""
    import hashlib

    n = int(vectors.shape[0])
    pick = np.unique(np.linspace(0, max(n - 1, 0), num=min(n, 4096)).astype(np.int64)) if n else np.zeros(0, np.int64)
    rows = np.ascontiguousarray(np.asarray(vectors[pick], dtype=np.float32))
    return {"centroids": hashlib.sha256(np.ascontiguousarray(centroids, np.float32).tobytes()).hexdigest(),
            "list_of_row": hashlib.sha256(np.ascontiguousarray(list_of_row, np.int32).tobytes()).hexdigest(),
            "vectors_sample": hashlib.sha256(rows.tobytes()).hexdigest(), "vectors_sample_rows": int(len(pick)),
            "vectors_shape": [n, int(vectors.shape[1]) if vectors.ndim == 2 else 0]}


def _lists_match_sample(vectors, centroids, list_of_row, metric: str, rows: int = 512) -> bool:
    """Artifacts written before the fingerprint existed: re-assign a few hundred rows against the stored centroids
    (float64; a row within 1e-9 relative of a tie may sit in either list) and compare with the stored lists."""
    n = int(vectors.shape[0])
    if n == 0:
        return True
    pick = np.unique(np.linspace(0, n - 1, num=min(n, rows)).astype(np.int64))
    x = np.asarray(vectors[pick], dtype=np.float64)
    c = np.asarray(centroids, dtype=np.float64)
    score = -(x @ c.T) if metric == "ip" else (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)
    best = score.min(axis=1)
    stored = score[np.arange(len(pick)), np.asarray(list_of_row)[pick]]
    return bool(np.all(stored - best <= 1e-9 * np.maximum(1.0, np.abs(best))))


def _build_ivf(vectors: np.ndarray, dim: int, key: str, metric: str, device: int, params: dict) -> IVFFlatIndex:
    nlist, codec = parse_index_key(key)
    # `int8_lists: true` on a Flat key: the lossless int8 lists where the corpus (as handed over, normalised or not) is byte-valued
    # and the kind can hold it; the IVF-Flat index otherwise, silently
    i8 = codec == "Flat" and bool(params.get("int8_lists", False)) and dim <= 128 and is_byte_valued(vectors)
    index = (IVFSQ8Index if codec == "SQ8" else IVFI8Index if i8 else IVFFlatIndex)(dim, nlist, metric, device)
    index.train(vectors, niter=int(params.get("niter", 25)), seed=int(params.get("seed", 1234)),
                max_points_per_centroid=int(params.get("max_points_per_centroid", 256)))
    index.add(vectors)
    return index


class HipApproximateSearch(RawAlgorithm):
    """ApproximateSearch semantics for "IVF<nlist>,Flat" and "IVF<nlist>,SQ8": train -> add -> nprobe from kwargs; raw
    FAISS conventions (no normalisation, no sign flip)."""

    def __init__(self, name: str, dimension: int, index_type: str, metric: str = "l2", device: Optional[int] = None,
                 **kwargs: Any) -> None:
        super().__init__(name, dimension, **kwargs)
        self.index_type = index_type
        self.metric = "l2" if metric == "l2" else "ip"      # approximate_search.py:25
        self.device = _resolve_device(device, kwargs.get("device_ids"))
        self.index: Optional[IVFFlatIndex] = None
        parse_index_key(index_type)                          # fail at construction, like a bad factory string

    def batch_search(self, queries: np.ndarray, k: int = 10, allowed=None) -> Tuple[np.ndarray, np.ndarray]:
        """`allowed` (None: every row): a bool mask over the rows, an integer id array or anything else IVFFlatIndex.set_filter
        takes -- the k nearest among those rows of the probed lists, same conventions and padding.  The same array object is
        installed once.  "IVF<nlist>,Flat" only: the library refuses the call on an SQ8 index."""
        if allowed is None:
            return super().batch_search(queries, k)
        self._require_built()
        self.index.ensure_filter(allowed)
        return self.index.search_filtered(np.asarray(queries).astype(np.float32), k)

    def range_search(self, queries: np.ndarray, radius: float, sort: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """faiss.IndexIVFFlat.range_search in the raw conventions: (lims, D, I) of the rows of the probed lists with squared L2 <
        radius / inner product > radius.  Per query the rows come in ascending (list, id); `sort="id"` orders them by id,
        `sort="distance"` nearest first, by (D, id) -- both on the host.  "IVF<nlist>,Flat" only: the library refuses an SQ8 index."""
        if sort not in (None, "id", "distance"):
            raise ValueError(f"sort must be None, 'id' or 'distance', got {sort!r}")
        self._require_built()
        lims, d, i = self.index.range_search(_ffi.as_f32_queries(queries), radius)
        if sort is not None and len(i):
            owner = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
            order = np.lexsort((i, owner)) if sort == "id" else np.lexsort((i, d if self.metric == "l2" else -d, owner))
            d, i = d[order], i[order]
        return lims, d, i

    def build_index(self, vectors: np.ndarray, metadata: Metadata = None) -> None:
        self.vectors = np.asarray(vectors).astype(np.float32)
        self.index = _build_ivf(self.vectors, self.dimension, self.index_type, self.metric, self.device, self.config)
        self.index_built = True
        if "nprobe" in self.config:
            self.index.set_nprobe(int(self.config["nprobe"]))
        reserve_workspace(self.index, self.config)

    # ---- persistence through the BaseAlgorithm hook (base_algorithm.py:98-120), by the protocol of persist.py ---------------
    # An SQ8 artifact stores the corpus, centroids and lists like a Flat one plus the ranges (ranges.npy: vmin, vdiff), under
    # its own format string: it never reloads as IVF-Flat, and loading re-encodes the stored rows under the stored lists
    # (encoding is deterministic: the codes come back bit-identical).
    _FORMAT = "vdbhip-ivfflat-v1"
    _FORMAT_SQ8 = "vdbhip-ivfsq8-v1"

    def _format(self) -> str:
        return self._FORMAT_SQ8 if parse_index_key(self.index_type)[1] == "SQ8" else self._FORMAT

    def save_index(self, artifact_dir: str, context=None):
        if not self.index_built or self.index is None:
            raise RuntimeError("Cannot persist HipApproximateSearch before build_index has completed.")
        if isinstance(self.index, IVFI8Index):
            raise NotImplementedError("save_index of an IVF-I8 index (int8_lists) is not implemented: build without int8_lists to persist")
        manifest = {"format": self._format(), "algorithm": type(self).__name__, "dimension": self.dimension,
                    "index_type": self.index_type, "metric": self.metric, "nlist": self.index.nlist,
                    "nprobe": self.index.nprobe, "n_vectors": int(self.index.ntotal)}
        arrays = {"vectors": self.vectors, "centroids": self.index.centroids(), "list_of_row": self.index.assignment()}
        fingerprint = _fingerprint(*arrays.values())
        if isinstance(self.index, IVFSQ8Index):
            arrays["ranges"] = np.stack(self.index.ranges())
            fingerprint["ranges"] = persist.sha256(arrays["ranges"])
        return persist.write_artifact(artifact_dir, context, manifest, arrays, fingerprint)

    def load_index(self, artifact_dir: str, context=None):
        if self.config.get("int8_lists", False):
            raise NotImplementedError("load_index with int8_lists is not implemented: an IVF-I8 index is built, not loaded")
        manifest, load, result = persist.read_artifact(artifact_dir, context, "HipApproximateSearch", format=self._format(),
                                                       dimension=self.dimension, index_type=self.index_type, metric=self.metric)
        vectors = load("vectors", mmap_mode="r")
        centroids = load("centroids")
        self.vectors = vectors
        sq8 = manifest["format"] == self._FORMAT_SQ8
        self.index = (IVFSQ8Index if sq8 else IVFFlatIndex)(self.dimension, int(manifest["nlist"]), self.metric, self.device)
        self.index.set_centroids(centroids)       # no k-means: the stored quantizer is reused ...
        if sq8:                                   # ... and so are the stored ranges
            ranges = load("ranges")
            want_ranges = (manifest.get("sha256") or {}).get("ranges")
            if ranges.shape != (2, self.dimension) or (want_ranges and persist.sha256(np.asarray(ranges, np.float32)) != want_ranges):
                raise ValueError("Persisted SQ8 ranges do not belong to this artifact")
            self.index.set_ranges(ranges[0], ranges[1])
        stored = load("list_of_row")
        if stored.shape != (vectors.shape[0],) or (len(stored) and (stored.min() < 0 or stored.max() >= int(manifest["nlist"]))):
            raise ValueError("Persisted inverted lists do not match the persisted corpus")
        # the three files must be the ones that were written together: a corpus or quantizer that does not belong to the
        # stored lists would load silently and answer with degraded recall
        want = manifest.get("sha256")
        if want:
            have = _fingerprint(vectors, centroids, stored)
            bad = [key for key in ("vectors_shape", "vectors_sample", "centroids", "list_of_row") if have[key] != want.get(key)]
            if bad:
                raise ValueError("Persisted index files do not belong together (fingerprint mismatch: " + ", ".join(bad) + ")")
        elif not _lists_match_sample(vectors, centroids, stored, self.metric):
            raise ValueError("Persisted inverted lists do not match the persisted corpus and centroids")
        self.index.add(vectors, list_of_row=stored)   # ... and so are the stored lists: no assignment pass either
        self.index.set_nprobe(int(self.config.get("nprobe", manifest.get("nprobe", 1))))
        self.index_built = True
        return result


class HipIVFIndexer(BaseIndexer):
    """FaissFactoryIndexer / FaissIVFIndexer semantics for "IVF<nlist>,Flat" and "IVF<nlist>,SQ8" keys."""

    _RESERVED = {"index_key", "index_type", "device", "device_ids", "niter", "seed", "max_points_per_centroid", "int8_lists"}

    def __init__(self, name: str, dimension: int, metric: str = "l2", index_type: Optional[str] = None,
                 index_key: Optional[str] = None, **kwargs: Any) -> None:
        key = index_key or index_type or "IVF100,Flat"
        params = dict(kwargs)
        params.setdefault("index_type", key)
        super().__init__(name, dimension, metric, **params)
        self.index_key = self.index_type = key
        parse_index_key(key)

    def build(self, vectors: np.ndarray, metadata: Metadata = None) -> IndexArtifact:
        data, metric, entries = indexer_operands(vectors, self.metric)
        meta = {"metric": self.metric, "index_key": self.index_key, **entries}
        device = _resolve_device(self.params.get("device"), self.params.get("device_ids"))
        index = _build_ivf(data, self.dimension, self.index_key, metric, device, self.params)
        if "nprobe" in self.params:                       # runtime attribute of the index (modular.py:269-275)
            index.set_nprobe(int(self.params["nprobe"]))
            meta["nprobe"] = self.params["nprobe"]
        reserve_workspace(index, self.params)
        return IndexArtifact(kind="hip_ivf", data=index, metadata=meta)


class HipIVFSearcher(FaissStyleSearcher):
    """FaissSearcher semantics over a HipIVFIndexer artifact.  `adc_max_batch` (a config entry `adc_max_batch: 16`): option
    "ivfpq_adc_max_batch" of the attached index -- it has an effect on an IVF-PQ index only (HipIVFPQIndexer)."""

    _kind = "hip_ivf"

    def __init__(self, name: str, dimension: int, metric: str = "l2", adc_max_batch: Optional[int] = None, **kwargs: Any) -> None:
        super().__init__(name, dimension, metric, **kwargs)
        self.adc_max_batch = None if adc_max_batch is None else int(adc_max_batch)

    def attach(self, artifact: IndexArtifact, vectors: np.ndarray, metadata: Metadata = None) -> None:
        meta = self._bind(artifact)
        self._prepared = True
        nprobe = self.params.get("nprobe")
        if nprobe is None:
            nprobe = meta.get("nprobe")
        if nprobe is not None:
            self.index.set_nprobe(int(nprobe))
        if self.adc_max_batch is not None:
            self.index.set_option("ivfpq_adc_max_batch", float(self.adc_max_batch))
            self.index.adc_max_batch = self.adc_max_batch

    def batch_search(self, queries: np.ndarray, k: int = 10, allowed=None) -> Tuple[np.ndarray, np.ndarray]:
        """`allowed` (None: every row): what IVFFlatIndex.set_filter takes -- the k nearest among those rows of the probed lists,
        in this searcher's conventions (queries normalised for cosine, distances negated for cosine / ip).  The same array
        object is installed once.  An IVF-Flat artifact only: the library refuses the call on the coded indexes."""
        if allowed is None:
            return super().batch_search(queries, k)
        self._require_attached()
        self.index.ensure_filter(allowed)
        d, i = self.index.search_filtered(self._prepare_query(queries), k)
        if self.metric in {"cosine", "ip"}:
            d = -d
        return d.astype(np.float32), i.astype(np.int64)

    def range_search(self, queries: np.ndarray, radius: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(lims, distances, ids) over the probed lists, ascending (list, id) per query, with HipLinearSearcher.range_search's
        radius: 'l2': the rows at Euclidean distance below `radius` (the library is asked for squared distances below
        float32(radius) * float32(radius)); 'cosine' / 'ip': the rows whose score (queries normalised for cosine) exceeds
        `radius`.  The distances are what `batch_search` returns: squared L2, negated scores.  An IVF-Flat artifact only."""
        self._require_attached()
        r = np.float32(radius)
        lims, d, i = self.index.range_search(self._prepare_query(queries), r * r if self.metric == "l2" else r)
        if self.metric in {"cosine", "ip"}:
            d = -d
        return lims, d.astype(np.float32), i.astype(np.int64)


register_algorithm("HipApproximateSearch", HipApproximateSearch)
register_algorithm("HipIVFFlat", HipApproximateSearch)
register_indexer("HipIVFIndexer", HipIVFIndexer)
register_indexer("HipFactoryIndexer", HipIVFIndexer)
register_searcher("HipIVFSearcher", HipIVFSearcher)

"""Thin object wrappers over the libvdbhip C-ABI handles: what every kind of index shares, and the flat index.

The returned conventions are those of faiss.IndexFlat, i.e. of the reference's ExactSearch
(exact_search.py:62-78): squared L2 ascending / raw inner product descending, int64 ids,
-1 / +-FLT_MAX padding when k exceeds the number of indexed rows.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _ffi

_METRICS = {"l2": _ffi.METRIC_L2, "ip": _ffi.METRIC_IP}


def metric_code(metric: str) -> int:
    if metric not in _METRICS:
        raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
    return _METRICS[metric]


def normalize_devices(device):
    """int -> int; a sequence of GPU ordinals -> list (length one -> its only member)."""
    if isinstance(device, (list, tuple, np.ndarray)):
        devs = [int(d) for d in device]
        if not devs:
            raise ValueError("empty device list")
        return devs[0] if len(devs) == 1 else devs
    return int(device)


def one_device(device, message: str) -> int:
    """`normalize_devices` for the kinds of index that run on one GPU: more than one ordinal is refused with `message`."""
    device = normalize_devices(device)
    if isinstance(device, list):
        raise ValueError(message)
    return device


def _pair(nq: int, width, first=np.float32) -> Tuple[np.ndarray, np.ndarray]:
    """The (nq, width) output pair of a host call: float32 / int64 for results, int32 / int64 for candidates."""
    return np.empty((nq, width), first), np.empty((nq, width), np.int64)


class _Handle:
    """What every index object shares: the library, the C-ABI handle it owns (one GPU ordinal or a list of them, see
    _ffi.create_handle), the calls that are the same on every kind of index, and the marshalling of host arrays (self.dim)."""

    def __init__(self, dim: int, metric: int, device):
        self._lib = _ffi.load()
        self._h = _ffi.create_handle(dim, metric, device)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vdb_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not getattr(self, "_h", None):
            raise RuntimeError("index handle already destroyed")
        return self._h

    def stats(self) -> dict:
        s = _ffi.Stats()
        _ffi.check(self._lib.vdb_stats(self._handle(), ctypes.byref(s)))
        return s.as_dict()

    def _sync_ntotal(self) -> None:
        """The row count is the library's: an add may have replaced rows instead of appending (e.g. after a failed add)."""
        self.ntotal = int(self.stats()["ntotal"])

    def reserve(self, nq: int, k: int = 10) -> None:
        """Size the search workspace for batches of up to `nq` queries now (vdb_reserve): the reference harness times its
        very first batch_search, allocations included (experiment_runner.py:431-437)."""
        _ffi.check(self._lib.vdb_reserve(self._handle(), int(nq), int(k)), build_time=True)

    def set_option(self, key: str, value: float) -> None:
        self._filter_key = None              # (any option change drops an installed filter)
        _ffi.check(self._lib.vdb_set_option(self._handle(), key.encode(), float(value)), build_time=True)

    def reset(self) -> None:
        """Drop every row; what was trained or set (centroids, ranges, codebooks) stays (faiss.Index.reset)."""
        self._filter_key = None
        _ffi.check(self._lib.vdb_reset(self._handle()), build_time=True)
        self.ntotal = 0

    # -- host arrays -> what the C ABI reads -------------------------------------------------------------
    def _queries(self, queries: np.ndarray) -> np.ndarray:
        q = _ffi.as_f32_queries(queries)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise RuntimeError(f"expected (nq, {self.dim}) queries, got {q.shape}")
        return q

    def _rows(self, x: np.ndarray) -> np.ndarray:
        x = _ffi.as_f32_c(x)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected (n, {self.dim}) vectors, got {x.shape}")
        return x

    def _codes(self, codes: np.ndarray) -> np.ndarray:
        """uint8 (n, M) product codes (the PQ kinds: self.M)."""
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        if c.ndim != 2 or c.shape[1] != self.M:
            raise ValueError(f"expected (n, {self.M}) codes, got {c.shape}")
        return c

    def _debug_scores(self, entry, queries: np.ndarray, nrows: int, *where):
        """(scores (nq, nrows) float32, eps (nq,) float32, cs) of a scan's own raw, unpacked scores (test hooks)."""
        q = self._queries(queries)
        nq = q.shape[0]
        scores = np.empty((nq, int(nrows)), np.float32)
        eps = np.empty((nq,), np.float32)
        cs = ctypes.c_double(0.0)
        _ffi.check(entry(self._handle(), _ffi.ptr(q), nq, *where, _ffi.ptr(scores), _ffi.ptr(eps), ctypes.byref(cs)))
        return scores, eps, float(cs.value)


class _FlatSearch(_Handle):
    """The search calls of the handles vdb_search serves: the flat index and the flat PQ index."""

    def search(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        q = self._queries(queries)
        D, I = _pair(q.shape[0], k)
        _ffi.check(self._lib.vdb_search(self._handle(), _ffi.ptr(q), q.shape[0], int(k), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def search_device(self, q_ptr: int, nq: int, k: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """All pointers are device memory on this index's GPU; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_search_device(self._handle(), q_ptr, int(nq), int(k), d_ptr, i_ptr, stream or None))

    def search_partial_device(self, q_ptr: int, nq: int, k: int, keys_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        """Partial top-k (float64 order keys + ids, device pointers) for merge_partials_device."""
        _ffi.check(self._lib.vdb_search_partial_device(self._handle(), q_ptr, int(nq), int(k), keys_ptr, ids_ptr,
                                                       stream or None))

    # -- range search (vdb_range_*): every row within a radius, ascending id per query ---------------------------
    def range_search(self, queries: np.ndarray, radius: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(lims int64 (nq + 1,), D float32, I int64): query q owns entries [lims[q], lims[q + 1]) -- the rows with squared
        L2 distance < radius / inner product > radius (faiss.IndexFlat.range_search), exact, in ascending id."""
        q = self._queries(queries)
        lims = np.empty((q.shape[0] + 1,), np.int64)
        _ffi.check(self._lib.vdb_range_search(self._handle(), _ffi.ptr(q), q.shape[0], float(np.float32(radius)), _ffi.ptr(lims)))
        D, I = np.empty((int(lims[-1]),), np.float32), np.empty((int(lims[-1]),), np.int64)
        _ffi.check(self._lib.vdb_range_results(self._handle(), _ffi.ptr(D), _ffi.ptr(I)))
        return lims, D, I

    def range_search_device(self, q_ptr: int, nq: int, radius: float, lims_ptr: int, stream: int = 0) -> int:
        """Device pointers on this index's GPU; waits for `stream` (the result size must reach the host) and returns
        lims[nq], the number of entries `range_results_device` will write."""
        total = ctypes.c_int64(0)
        _ffi.check(self._lib.vdb_range_search_device(self._handle(), q_ptr, int(nq), float(np.float32(radius)), lims_ptr,
                                                     ctypes.byref(total), stream or None))
        return int(total.value)

    def range_results_device(self, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """The (D, I) of the last range search of this index into device memory; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_range_results_device(self._handle(), d_ptr, i_ptr, stream or None))

    # -- filtered search (vdb_filter_*, vdb_search_filtered): the k nearest rows among those an allow bitmap admits ----
    _filter_key = None       # (object, ntotal) of the filter `ensure_filter` installed last; any call that drops the filter clears it

    def set_filter(self, allowed, nbits: Optional[int] = None) -> None:
        """Install the rows a filtered search may return: a bool array of length ntotal, an integer array of ids (id_base +
        row; duplicates allowed, out of range raises ValueError), or packed uint32 words with `nbits=` (_ffi.pack_allow_bits).
        Any add, reset or set_option drops the filter."""
        self._filter_key = None
        words = _ffi.pack_allow_bits(allowed, self.ntotal, getattr(self, "id_base", 0), nbits)
        _ffi.check(self._lib.vdb_filter_set(self._handle(), _ffi.ptr(words), self.ntotal), build_time=True)

    def set_filter_device(self, words_ptr: int, nbits: int, stream: int = 0) -> None:
        """Packed uint32 words in device memory of this index's GPU; runs on `stream` and waits for it once."""
        self._filter_key = None
        _ffi.check(self._lib.vdb_filter_set_device(self._handle(), words_ptr, int(nbits), stream or None), build_time=True)

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
        _ffi.check(self._lib.vdb_filter_count(self._handle(), ctypes.byref(n)))
        return int(n.value)

    def search_filtered(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """`search` among the rows of the installed filter: same keys, order and padding (fewer than k admitted rows pad)."""
        q = self._queries(queries)
        D, I = _pair(q.shape[0], k)
        _ffi.check(self._lib.vdb_search_filtered(self._handle(), _ffi.ptr(q), q.shape[0], int(k), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def search_filtered_device(self, q_ptr: int, nq: int, k: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """All pointers are device memory on this index's GPU; asynchronous on `stream`."""
        _ffi.check(self._lib.vdb_search_filtered_device(self._handle(), q_ptr, int(nq), int(k), d_ptr, i_ptr, stream or None))

    def rerank(self, queries: np.ndarray, candidate_ids: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-k among explicit candidate ids per query (nq, ncand) int64, -1 = empty slot."""
        q = _ffi.as_f32_queries(queries)
        c = np.ascontiguousarray(candidate_ids, dtype=np.int64)
        if c.ndim != 2 or c.shape[0] != q.shape[0] or q.shape[1] != self.dim:
            raise RuntimeError(f"expected queries (nq, {self.dim}) and candidates (nq, ncand), got {q.shape}, {c.shape}")
        D, I = _pair(q.shape[0], k)
        _ffi.check(self._lib.vdb_rerank(self._handle(), _ffi.ptr(q), q.shape[0], _ffi.ptr(c), c.shape[1], int(k),
                                        _ffi.ptr(D), _ffi.ptr(I)))
        return D, I


class FlatIndex(_FlatSearch):
    """Device-resident brute-force index (replaces faiss.IndexFlat(d, metric)).  `device`: one GPU ordinal, or a list of
    them -- ONE index row-sharded over those MI355X inside this process (vdb_create_multi): same calls, same results."""

    def __init__(self, dim: int, metric: str = "l2", device=0):
        code = metric_code(metric)
        self.dim, self.metric, self.device = int(dim), metric, normalize_devices(device)
        super().__init__(self.dim, code, self.device)
        self.ntotal = 0
        self.id_base = 0

    @property
    def devices(self):
        return list(self.device) if isinstance(self.device, list) else [self.device]

    # -- build --------------------------------------------------------------------------------------
    def add(self, vectors: np.ndarray, id_base: int = 0) -> None:
        """Append rows (faiss.Index.add): row i of the index, counted over all adds, has id `id_base + i`; every add of
        one index passes the same `id_base`.  `reset()` empties the index."""
        x = self._rows(vectors)
        self._filter_key = None
        try:
            _ffi.check(self._lib.vdb_add(self._handle(), _ffi.ptr(x), x.shape[0], int(id_base)), build_time=True)
            self.id_base = int(id_base)
        finally:
            self._sync_ntotal()

    def add_device(self, dev_ptr: int, n: int, id_base: int = 0, stream: int = 0) -> None:
        self._filter_key = None
        try:
            _ffi.check(self._lib.vdb_add_device(self._handle(), dev_ptr, int(n), int(id_base), stream or None),
                       build_time=True)
            self.id_base = int(id_base)
        finally:
            self._sync_ntotal()

    def reset(self) -> None:
        """Drop every row (faiss.Index.reset)."""
        super().reset()
        self._sync_ntotal()

    # -- sign-LSH codes (vdb_lsh_*): Hamming candidates + exact re-rank -------------------------------
    def lsh_set_projection(self, projection: np.ndarray) -> None:
        """Install R (nbits, dim) float32; rows already indexed are encoded now, later adds encode what they append."""
        r = _ffi.as_f32_c(projection)
        if r.ndim != 2 or r.shape[1] != self.dim:
            raise ValueError(f"expected a (nbits, {self.dim}) projection, got {r.shape}")
        _ffi.check(self._lib.vdb_lsh_set_projection(self._handle(), int(r.shape[0]), _ffi.ptr(r)), build_time=True)

    def lsh_get_projection(self) -> Optional[np.ndarray]:
        nbits = ctypes.c_int(0)
        _ffi.check(self._lib.vdb_lsh_get_projection(self._handle(), ctypes.byref(nbits), None))
        if nbits.value == 0:
            return None
        r = np.empty((nbits.value, self.dim), np.float32)
        _ffi.check(self._lib.vdb_lsh_get_projection(self._handle(), ctypes.byref(nbits), _ffi.ptr(r)))
        return r

    def lsh_codes(self) -> np.ndarray:
        """Codes of the indexed rows, uint32 (ntotal, nbits / 32): bit j of a row is bit j % 32 of word j / 32."""
        nbits = ctypes.c_int(0)
        _ffi.check(self._lib.vdb_lsh_get_projection(self._handle(), ctypes.byref(nbits), None))
        codes = np.empty((self.ntotal, nbits.value // 32), np.uint32)
        _ffi.check(self._lib.vdb_lsh_get_codes(self._handle(), _ffi.ptr(codes)))
        return codes

    def lsh_candidates(self, queries: np.ndarray, ncand: int) -> Tuple[np.ndarray, np.ndarray]:
        """Per query the min(ncand, ntotal) rows smallest under (Hamming distance, id): (int32 (nq, ncand), int64 (nq, ncand)),
        padded with INT32_MAX / -1."""
        q = self._queries(queries)
        ham, ids = _pair(q.shape[0], int(ncand), np.int32)
        _ffi.check(self._lib.vdb_lsh_candidates(self._handle(), _ffi.ptr(q), q.shape[0], int(ncand), _ffi.ptr(ham), _ffi.ptr(ids)))
        return ham, ids

    def lsh_candidates_device(self, q_ptr: int, nq: int, ncand: int, ham_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        _ffi.check(self._lib.vdb_lsh_candidates_device(self._handle(), q_ptr, int(nq), int(ncand), ham_ptr, ids_ptr, stream or None))

    def lsh_search(self, queries: np.ndarray, k: int, ncand: int) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-k among the `ncand` Hamming candidates of every query (flat conventions and padding)."""
        q = self._queries(queries)
        D, I = _pair(q.shape[0], int(k))
        _ffi.check(self._lib.vdb_lsh_search(self._handle(), _ffi.ptr(q), q.shape[0], int(k), int(ncand), _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def lsh_search_device(self, q_ptr: int, nq: int, k: int, ncand: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        _ffi.check(self._lib.vdb_lsh_search_device(self._handle(), q_ptr, int(nq), int(k), int(ncand), d_ptr, i_ptr, stream or None))

    # -- hash-table LSH (vdb_lsht_*): table keys, collision votes, exact re-rank -------------------------
    def lsht_set_tables(self, projections: np.ndarray, offsets: Optional[np.ndarray] = None, bucket_width: float = 0.0) -> None:
        """Install T tables of H projections, P (T, H, dim) float32.  `offsets` None: sign keys (mode 0); else E2 bucket keys
        (mode 1) with offsets b (T, H) float32 and `bucket_width`.  Rows already indexed are keyed now, later adds key what
        they append."""
        p = _ffi.as_f32_c(projections)
        if p.ndim != 3 or p.shape[2] != self.dim:
            raise ValueError(f"expected (num_tables, hash_size, {self.dim}) projections, got {p.shape}")
        b = None
        if offsets is not None:
            b = _ffi.as_f32_c(offsets)
            if b.shape != p.shape[:2]:
                raise ValueError(f"expected {p.shape[:2]} offsets, got {b.shape}")
        _ffi.check(self._lib.vdb_lsht_set_tables(self._handle(), int(p.shape[0]), int(p.shape[1]), 0 if b is None else 1, _ffi.ptr(p),
                                                 _ffi.ptr(b), float(bucket_width)), build_time=True)

    def lsht_get_tables(self) -> Optional[dict]:
        """None without tables, else {num_tables, hash_size, mode, projections, offsets (None in sign mode), bucket_width}."""
        t, hs, mode, w = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_float(0.0)
        refs = (ctypes.byref(t), ctypes.byref(hs), ctypes.byref(mode))
        _ffi.check(self._lib.vdb_lsht_get_tables(self._handle(), *refs, None, None, ctypes.byref(w)))
        if t.value == 0:
            return None
        p = np.empty((t.value, hs.value, self.dim), np.float32)
        b = np.empty((t.value, hs.value), np.float32) if mode.value == 1 else None
        _ffi.check(self._lib.vdb_lsht_get_tables(self._handle(), *refs, _ffi.ptr(p), _ffi.ptr(b), ctypes.byref(w)))
        return {"num_tables": t.value, "hash_size": hs.value, "mode": mode.value, "projections": p, "offsets": b,
                "bucket_width": float(w.value)}

    def lsht_keys(self) -> np.ndarray:
        """Table keys of the indexed rows, uint32 (ntotal, T * W): W = ceil(H / 32) words per table in sign mode, H in E2 mode."""
        t, hs, mode = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _ffi.check(self._lib.vdb_lsht_get_tables(self._handle(), ctypes.byref(t), ctypes.byref(hs), ctypes.byref(mode), None, None, None))
        words = t.value * (hs.value if mode.value == 1 else (hs.value + 31) // 32)
        keys = np.empty((self.ntotal, words), np.uint32)
        _ffi.check(self._lib.vdb_lsht_get_keys(self._handle(), _ffi.ptr(keys)))
        return keys

    def lsht_candidates(self, queries: np.ndarray, ncand: int) -> Tuple[np.ndarray, np.ndarray]:
        """Per query its colliding rows under (votes descending, first table, id), at most `ncand`: (votes int32 (nq, ncand),
        ids int64 (nq, ncand)), padded with 0 / -1."""
        q = self._queries(queries)
        votes, ids = _pair(q.shape[0], int(ncand), np.int32)
        _ffi.check(self._lib.vdb_lsht_candidates(self._handle(), _ffi.ptr(q), q.shape[0], int(ncand), _ffi.ptr(votes), _ffi.ptr(ids)))
        return votes, ids

    def lsht_candidates_device(self, q_ptr: int, nq: int, ncand: int, votes_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        _ffi.check(self._lib.vdb_lsht_candidates_device(self._handle(), q_ptr, int(nq), int(ncand), votes_ptr, ids_ptr, stream or None))

    def lsht_search(self, queries: np.ndarray, k: int, ncand: int, fallback: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-k among the `ncand` vote candidates of every query (flat conventions and padding); `fallback`: a query
        without a colliding row gets the exact flat top-k instead."""
        q = self._queries(queries)
        D, I = _pair(q.shape[0], int(k))
        _ffi.check(self._lib.vdb_lsht_search(self._handle(), _ffi.ptr(q), q.shape[0], int(k), int(ncand), int(bool(fallback)),
                                             _ffi.ptr(D), _ffi.ptr(I)))
        return D, I

    def lsht_search_device(self, q_ptr: int, nq: int, k: int, ncand: int, fallback: bool, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        _ffi.check(self._lib.vdb_lsht_search_device(self._handle(), q_ptr, int(nq), int(k), int(ncand), int(bool(fallback)), d_ptr,
                                                    i_ptr, stream or None))

    def rerank_device(self, q_ptr: int, nq: int, cand_ptr: int, ncand: int, k: int, d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        _ffi.check(self._lib.vdb_rerank_device(self._handle(), q_ptr, int(nq), cand_ptr, int(ncand), int(k), d_ptr, i_ptr, stream or None))

    # -- introspection --------------------------------------------------------------------------------
    def debug_scan_scores(self, queries: np.ndarray, row0: int, nrows: int):
        return self._debug_scores(self._lib.vdb_debug_scan_scores, queries, nrows, int(row0), int(nrows))


def merge_partials_device(metric: str, device: int, keys_ptr: int, ids_ptr: int, nparts: int, nq: int, k: int,
                          d_ptr: int, i_ptr: int, stream: int = 0) -> None:
    """Merge (nparts, nq, k) per-shard partial lists (device memory) into the final (nq, k) result."""
    _ffi.check(_ffi.load().vdb_merge_partials_device(_METRICS[metric], int(device), keys_ptr, ids_ptr, int(nparts),
                                                     int(nq), int(k), d_ptr, i_ptr, stream or None))


def merge_packed_partials_device(metric: str, device: int, packed_ptr: int, nparts: int, nq: int, k: int, d_ptr: int,
                                 i_ptr: int, stream: int = 0) -> None:
    """Merge per-part packed buffers (nparts, 2, nq, k) of 8-byte words: keys then ids (one all-gather)."""
    _ffi.check(_ffi.load().vdb_merge_packed_partials_device(_METRICS[metric], int(device), packed_ptr, int(nparts),
                                                            int(nq), int(k), d_ptr, i_ptr, stream or None))

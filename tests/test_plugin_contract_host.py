"""The Python layer's contract, pinned on the CPU over a recording fake of libvdbhip: which entry point every index method and
every plugin class calls, with which scalars and which buffers, and what comes back -- dtypes, shapes, sign flips, padding,
metadata, messages.  `_ffi.load` and `_ffi.create_handle` are the only seam: the real index classes and the real plugin classes
run unmodified over the fake, so the file holds for any arrangement of the code above the C ABI.

Four behaviours differ on purpose between a tree whose `_Handle` has the shared `_queries` helper and one that has not (each
replaces a wrong-sized buffer handed to C): IVFFlatIndex.train checks its rows, PQIndex.rerank checks and reshapes as
FlatIndex.rerank does, the three debug hooks check their queries, and IVFFlatIndex.add re-reads ntotal after a failed add.  On a
tree without the helper those cases skip; with it they are asserted.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

F32 = np.float32
DIM, M, NLIST, N, NQ, K = 8, 4, 4, 5, 3, 4
H = 77                                   # the handle create_handle gives out
FLT_MAX = np.finfo(F32).max
RNG = np.random.default_rng(22)
X = RNG.standard_normal((N, DIM)).astype(F32)
Q = RNG.standard_normal((NQ, DIM)).astype(F32)
CODES = RNG.integers(0, 256, size=(N, M)).astype(np.uint8)
LISTS = np.array([0, 1, 2, 3, 0], np.int32)

# entry point -> (position of a float32 (rows, DIM) matrix pointer, position of its row count)
_MATRIX = {name: (1, 2) for name in (
    "vdb_add", "vdb_ivf_add", "vdb_ivf_add_assigned", "vdb_pq_add", "vdb_search", "vdb_ivf_search", "vdb_rerank",
    "vdb_lsh_candidates", "vdb_lsh_search", "vdb_lsht_candidates", "vdb_lsht_search", "vdb_knng_search",
    "vdb_ivf_sq8_train_ranges", "vdb_debug_scan_scores", "vdb_debug_pq_adc_scores", "vdb_debug_ivfpq_adc_scores")}
_MATRIX.update({name: (2, 3) for name in ("vdb_ivf_train", "vdb_pq_train", "vdb_ivfpq_train")})
# host entry points that fill an (nq, width) pair at their last two pointers: (position of width, dtype of the first array)
_OUTPUT = {"vdb_search": (3, F32), "vdb_ivf_search": (3, F32), "vdb_lsh_search": (3, F32), "vdb_lsht_search": (3, F32),
           "vdb_knng_search": (3, F32), "vdb_rerank": (5, F32), "vdb_lsh_candidates": (3, np.int32),
           "vdb_lsht_candidates": (3, np.int32)}
_DEBUG = {"vdb_debug_scan_scores": 4, "vdb_debug_pq_adc_scores": 4, "vdb_debug_ivfpq_adc_scores": 5}    # position of nrows


def canned(nq, width, first=F32):
    """What the fake answers: row i, slot j; the last slot of every row is a padded one (id -1)."""
    i, j = np.arange(nq)[:, None], np.arange(width)[None, :]
    a = (0.5 + i + 0.3 * j).astype(F32) if first is F32 else (i + j).astype(np.int32)
    ids = (i + 2 * j).astype(np.int64)
    a[:, -1] = FLT_MAX if first is F32 else np.iinfo(np.int32).max
    ids[:, -1] = -1
    return a, ids


def _fill(ptr, values):
    ctype = np.ctypeslib.as_ctypes_type(values.dtype)
    np.ctypeslib.as_array((ctype * values.size).from_address(ptr))[:] = values.ravel()


class FakeLib:
    def __init__(self):
        self.log, self.seen, self.fail = [], {}, {}
        self.ntotal, self.bytes_resident = N, 3 << 20

    def __getattr__(self, name):
        if not name.startswith("vdb_"):
            raise AttributeError(name)

        def call(*args):
            if name == "vdb_destroy":              # whenever the collector gets to an index: not part of any sequence
                return 0
            self.log.append((name, args))
            return self._serve(name, args)
        return call

    def _serve(self, name, args):
        from vdbhip import _ffi

        if name == "vdb_last_error":
            return None
        if name in self.fail:
            return self.fail[name]
        if name in _MATRIX:
            p, n = _MATRIX[name]
            rows = np.ctypeslib.as_array((ctypes.c_float * (args[n] * DIM)).from_address(args[p])).reshape(args[n], DIM)
            self.seen.setdefault(name, []).append((args[p], rows.copy()))
        if name == "vdb_stats":
            args[1]._obj.ntotal, args[1]._obj.bytes_resident = self.ntotal, self.bytes_resident
        if name in _OUTPUT:
            w, first = _OUTPUT[name]
            a, ids = canned(args[2], args[w], first)
            _fill(args[-2], a)
            _fill(args[-1], ids)
        if name in _DEBUG:
            nq, nrows = args[2], args[_DEBUG[name]]
            _fill(args[-3], np.arange(nq * nrows, dtype=F32))
            _fill(args[-2], np.arange(nq, dtype=F32))
            args[-1]._obj.value = 2.5
        return _ffi.VDB_OK

    # -- reading the log ------------------------------------------------------------------------------------------------------
    def names(self):
        return [n for n, _ in self.log]

    def calls(self, name):
        return [a for n, a in self.log if n == name]

    def matrix(self, name):
        return self.seen[name][-1]

    def clear(self):
        self.log.clear()
        self.seen.clear()


@pytest.fixture
def fake(monkeypatch):
    from vdbhip import _ffi

    lib = FakeLib()

    def create_handle(dim, metric, device):
        lib.log.append(("create", (dim, metric, device)))
        return H
    monkeypatch.setattr(_ffi, "load", lambda: lib)
    monkeypatch.setattr(_ffi, "create_handle", create_handle)
    monkeypatch.delenv("VDBHIP_DEVICE_FROM_RANK", raising=False)
    return lib


def permitted_difference():
    from vdbhip.index import _Handle

    if not hasattr(_Handle, "_queries"):
        pytest.skip("this tree hands a wrong-sized buffer to the library here")


def make_index(kind, metric="l2", device=0):
    import vdbhip

    return {"flat": lambda: vdbhip.FlatIndex(DIM, metric, device), "knng": lambda: vdbhip.KnnGraphIndex(DIM, metric, device),
            "ivf": lambda: vdbhip.IVFFlatIndex(DIM, NLIST, metric, device), "sq8": lambda: vdbhip.IVFSQ8Index(DIM, NLIST, metric, device),
            "pq": lambda: vdbhip.PQIndex(DIM, M, metric, device), "ivfpq": lambda: vdbhip.IVFPQIndex(DIM, NLIST, M, metric, device)}[kind]()


KINDS = ("flat", "knng", "ivf", "sq8", "pq", "ivfpq")
GOOD = {"f32c": Q, "f64": Q.astype(np.float64), "fortran": np.asfortranarray(Q), "1d": Q[0]}
BAD = {"wrong_dim": Q[:, :7], "wrong_ndim": Q.reshape(1, NQ, DIM)}
INPUTS = tuple(GOOD) + tuple(BAD)


def as_matrix(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1, DIM)


# ---- index classes: construction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_index_construction(fake, kind):
    for metric, code in (("l2", 0), ("ip", 1)):
        fake.clear()
        idx = make_index(kind, metric)
        assert fake.calls("create") == [(DIM, code, 0)] and idx.ntotal == 0 and idx.metric == metric
        want = {"sq8": [("vdb_ivf_set_codec", (H, 1))], "ivfpq": [("vdb_ivf_set_codec", (H, 2))]}.get(kind, [])
        assert fake.log[1:] == want
    with pytest.raises(ValueError) as e:
        make_index(kind, "cosine")
    assert str(e.value) == "metric must be 'l2' or 'ip', got 'cosine'"


def test_index_constructor_options_and_refusals(fake):
    import vdbhip

    vdbhip.PQIndex(DIM, M, adc_max_batch=16)
    assert fake.calls("vdb_set_option") == [(H, b"pq_adc_max_batch", 16.0)]
    fake.clear()
    vdbhip.IVFPQIndex(DIM, NLIST, M, adc_max_batch=8)
    assert fake.names() == ["create", "vdb_ivf_set_codec", "vdb_set_option"]
    assert fake.calls("vdb_set_option") == [(H, b"ivfpq_adc_max_batch", 8.0)]
    one_gpu = {"sq8": "IVF<nlist>,SQ8 runs on one GPU: a multi-device index (more than one device id) is not available for the SQ8 codec",
               "pq": "PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available",
               "ivfpq": "IVF<nlist>,PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available"}
    for kind, message in one_gpu.items():
        fake.clear()
        with pytest.raises(ValueError) as e:
            make_index(kind, device=[0, 1])
        assert str(e.value) == message and fake.log == []
    assert make_index("flat", device=[0, 1]).device == [0, 1] and make_index("ivf", device=[3]).device == 3
    with pytest.raises(ValueError, match=r"M must divide dim and lie in \[1, min\(dim, 256\)\]; got dim=8, M=3"):
        vdbhip.PQIndex(DIM, 3)
    with pytest.raises(ValueError, match=r"M must divide dim"):
        vdbhip.IVFPQIndex(DIM, NLIST, 3)


# ---- index classes: methods that take queries -----------------------------------------------------------------------------------
# (kind, method, arguments after the queries, entry point, scalars between nq and the two output pointers, dtype of the first output)
QUERY_METHODS = [
    ("flat", "search", (K,), "vdb_search", (K,), F32), ("knng", "search", (K,), "vdb_search", (K,), F32),
    ("pq", "search", (K,), "vdb_search", (K,), F32), ("ivf", "search", (K,), "vdb_ivf_search", (K,), F32),
    ("sq8", "search", (K,), "vdb_ivf_search", (K,), F32), ("ivfpq", "search", (K,), "vdb_ivf_search", (K,), F32),
    ("flat", "lsh_candidates", (6,), "vdb_lsh_candidates", (6,), np.int32), ("flat", "lsh_search", (K, 6), "vdb_lsh_search", (K, 6), F32),
    ("flat", "lsht_candidates", (6,), "vdb_lsht_candidates", (6,), np.int32),
    ("flat", "lsht_search", (K, 6, True), "vdb_lsht_search", (K, 6, 1), F32), ("flat", "lsht_search", (K, 6), "vdb_lsht_search", (K, 6, 0), F32),
    ("knng", "knng_search", (K, 7), "vdb_knng_search", (K, 7), F32), ("knng", "knng_search", (K,), "vdb_knng_search", (K, K), F32),
    ("knng", "lsh_search", (K, 6), "vdb_lsh_search", (K, 6), F32),
]


@pytest.mark.parametrize("which", INPUTS)
@pytest.mark.parametrize("kind,method,args,entry,scalars,first", QUERY_METHODS)
def test_query_methods(fake, kind, method, args, entry, scalars, first, which):
    idx = make_index(kind)
    fake.clear()
    if which in BAD:
        with pytest.raises(RuntimeError) as e:
            getattr(idx, method)(BAD[which], *args)
        assert type(e.value) is RuntimeError and str(e.value) == f"expected (nq, {DIM}) queries, got {BAD[which].shape}"
        assert fake.log == []
        return
    q = GOOD[which]
    a, ids = getattr(idx, method)(q, *args)
    nq = 1 if which == "1d" else NQ
    (got,) = fake.calls(entry)
    assert fake.names() == [entry]
    assert got[0] == H and got[2:-2] == (nq,) + scalars and got[-2:] == (a.ctypes.data, ids.ctypes.data)
    assert a.dtype == first and ids.dtype == np.int64 and a.shape == ids.shape == (nq, args[0])
    assert a.flags["C_CONTIGUOUS"] and ids.flags["C_CONTIGUOUS"]
    want_a, want_ids = canned(nq, args[0], first)
    assert np.array_equal(a, want_a) and np.array_equal(ids, want_ids)
    ptr, seen = fake.matrix(entry)
    assert np.array_equal(seen, as_matrix(q)) and got[1] == ptr
    if which == "f32c":
        assert ptr == q.ctypes.data


CAND = np.array([[0, 1, 2, 3, 4, -1]] * NQ, np.int64)
RERANK_CASES = {"f32c": (Q, CAND), "f64": (Q.astype(np.float64), CAND), "fortran": (np.asfortranarray(Q), CAND), "1d": (Q[0], CAND[:1]),
                "int32_candidates": (Q, CAND.astype(np.int32)), "wrong_dim": (Q[:, :7], CAND), "wrong_ndim": (Q.reshape(1, NQ, DIM), CAND),
                "flat_candidates": (Q, CAND[0]), "fewer_candidate_rows": (Q, CAND[:2])}


@pytest.mark.parametrize("which", list(RERANK_CASES))
@pytest.mark.parametrize("kind", ["flat", "knng", "pq"])
def test_rerank(fake, kind, which):
    idx = make_index(kind)
    fake.clear()
    q, c = RERANK_CASES[which]
    bad = which in ("wrong_dim", "wrong_ndim", "flat_candidates", "fewer_candidate_rows")
    if kind == "pq" and (bad or which == "1d"):
        permitted_difference()
    if bad:
        with pytest.raises(RuntimeError) as e:
            idx.rerank(q, c, K)
        assert type(e.value) is RuntimeError
        assert str(e.value) == f"expected queries (nq, {DIM}) and candidates (nq, ncand), got {q.shape}, {c.shape}"
        assert fake.log == []
        return
    d, i = idx.rerank(q, c, K)
    nq = c.shape[0]
    (got,) = fake.calls("vdb_rerank")
    assert fake.names() == ["vdb_rerank"] and got[0] == H and got[2] == nq and got[4:6] == (6, K)
    assert got[-2:] == (d.ctypes.data, i.ctypes.data) and d.dtype == F32 and i.dtype == np.int64 and d.shape == i.shape == (nq, K)
    assert np.array_equal(d, canned(nq, K)[0]) and np.array_equal(i, canned(nq, K)[1])
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_int64 * (nq * 6)).from_address(got[3])).reshape(nq, 6), c)
    ptr, seen = fake.matrix("vdb_rerank")
    assert np.array_equal(seen, as_matrix(q))
    if which == "f32c":
        assert ptr == q.ctypes.data and got[3] == c.ctypes.data


# (kind, method, arguments after the queries, entry point, scalars after nq)
DEBUG_HOOKS = [("flat", "debug_scan_scores", (1, 2), "vdb_debug_scan_scores", (1, 2)),
               ("pq", "debug_adc_scores", (1, 2), "vdb_debug_pq_adc_scores", (1, 2)),
               ("ivfpq", "debug_adc_scores", (3, 1, 2), "vdb_debug_ivfpq_adc_scores", (3, 1, 2))]


@pytest.mark.parametrize("which", INPUTS)
@pytest.mark.parametrize("kind,method,args,entry,scalars", DEBUG_HOOKS)
def test_debug_hooks(fake, kind, method, args, entry, scalars, which):
    idx = make_index(kind)
    fake.clear()
    if which in BAD or which == "1d":
        permitted_difference()
    if which in BAD:
        with pytest.raises(RuntimeError) as e:
            getattr(idx, method)(BAD[which], *args)
        assert str(e.value) == f"expected (nq, {DIM}) queries, got {BAD[which].shape}" and fake.log == []
        return
    q = GOOD[which]
    scores, eps, cs = getattr(idx, method)(q, *args)
    nq = 1 if which == "1d" else NQ
    (got,) = fake.calls(entry)
    assert fake.names() == [entry] and got[0] == H and got[2:-3] == (nq,) + scalars
    assert got[-3:-1] == (scores.ctypes.data, eps.ctypes.data)
    assert scores.dtype == eps.dtype == F32 and scores.shape == (nq, 2) and eps.shape == (nq,) and type(cs) is float and cs == 2.5
    assert np.array_equal(scores.ravel(), np.arange(nq * 2)) and np.array_equal(eps, np.arange(nq))
    ptr, seen = fake.matrix(entry)
    assert np.array_equal(seen, as_matrix(q))
    if which == "f32c":
        assert ptr == q.ctypes.data


# ---- index classes: methods that take rows or codes -----------------------------------------------------------------------------
TRAIN = dict(niter=2, seed=7, max_points_per_centroid=9)
# (kind, method, positional arguments after the rows, keyword arguments, [(entry point, scalars before the pointer, after it)], re-reads ntotal)
ROW_METHODS = [
    ("flat", "add", (3,), {}, [("vdb_add", (), (N, 3))], True), ("knng", "add", (3,), {}, [("vdb_add", (), (N, 3))], True),
    ("ivf", "add", (3,), {}, [("vdb_ivf_add", (), (N, 3))], True), ("sq8", "add", (3,), {}, [("vdb_ivf_add", (), (N, 3))], True),
    ("ivfpq", "add", (3,), {}, [("vdb_ivf_add", (), (N, 3))], True), ("pq", "add", (3,), {}, [("vdb_pq_add", (), (N, 3))], True),
    ("ivf", "add", (3, LISTS), {}, [("vdb_ivf_add_assigned", (), (N, 3, LISTS.ctypes.data))], True),
    ("ivf", "train", (), TRAIN, [("vdb_ivf_train", (NLIST,), (N, 2, 7, 9))], False),
    ("sq8", "train", (), TRAIN, [("vdb_ivf_train", (NLIST,), (N, 2, 7, 9))], False),
    ("ivfpq", "train", (), TRAIN, [("vdb_ivf_train", (NLIST,), (N, 2, 7, 9)), ("vdb_ivfpq_train", (M,), (N, 2, 7, 9))], False),
    ("ivfpq", "train_codebooks", (), TRAIN, [("vdb_ivfpq_train", (M,), (N, 2, 7, 9))], False),
    ("pq", "train", (), TRAIN, [("vdb_pq_train", (M,), (N, 2, 7, 9))], False),
    ("sq8", "train_ranges", (), {}, [("vdb_ivf_sq8_train_ranges", (), (N,))], False),
]
ROWS_GOOD = {"f32c": X, "f64": X.astype(np.float64), "fortran": np.asfortranarray(X)}
ROWS_BAD = {"wrong_dim": X[:, :7], "wrong_ndim": X[0]}


@pytest.mark.parametrize("which", list(ROWS_GOOD) + list(ROWS_BAD))
@pytest.mark.parametrize("kind,method,args,kwargs,entries,syncs", ROW_METHODS)
def test_row_methods(fake, kind, method, args, kwargs, entries, syncs, which):
    idx = make_index(kind)
    fake.clear()
    if which in ROWS_BAD:
        if method == "train" and kind != "pq":
            permitted_difference()
        with pytest.raises(ValueError) as e:
            getattr(idx, method)(ROWS_BAD[which], *args, **kwargs)
        assert type(e.value) is ValueError and str(e.value) == f"expected (n, {DIM}) vectors, got {ROWS_BAD[which].shape}"
        assert fake.log == []
        return
    x = ROWS_GOOD[which]
    idx.ntotal = 99
    assert getattr(idx, method)(x, *args, **kwargs) is None
    assert fake.names() == [e for e, _, _ in entries] + (["vdb_stats"] if syncs else [])
    for entry, before, after in entries:
        (got,) = fake.calls(entry)
        ptr, seen = fake.matrix(entry)
        assert got == (H,) + before + (ptr,) + after and np.array_equal(seen, x)
        if which == "f32c":
            assert ptr == x.ctypes.data
    assert idx.ntotal == (N if syncs else 99 if (kind, method) == ("pq", "train") else 0)
    if method == "train":
        assert idx.is_trained


CODE_METHODS = [("pq", (3,), "vdb_pq_add_codes", (N, 3)), ("ivfpq", (LISTS, 3), "vdb_ivfpq_add_codes", (N, 3, LISTS.ctypes.data))]


@pytest.mark.parametrize("which", ["uint8", "int64", "fortran", "wrong_width", "wrong_ndim"])
@pytest.mark.parametrize("kind,args,entry,after", CODE_METHODS)
def test_code_methods(fake, kind, args, entry, after, which):
    idx = make_index(kind)
    fake.clear()
    c = {"uint8": CODES, "int64": CODES.astype(np.int64), "fortran": np.asfortranarray(CODES), "wrong_width": CODES[:, :3],
         "wrong_ndim": CODES[0]}[which]
    if which.startswith("wrong"):
        with pytest.raises(ValueError) as e:
            idx.add_codes(c, *args)
        assert str(e.value) == f"expected (n, {M}) codes, got {c.shape}" and fake.log == []
        return
    idx.add_codes(c, *args)
    assert fake.names() == [entry, "vdb_stats"] and idx.ntotal == N
    (got,) = fake.calls(entry)
    assert got[0] == H and got[2:] == after
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_uint8 * (N * M)).from_address(got[1])).reshape(N, M), CODES)
    if which == "uint8":
        assert got[1] == c.ctypes.data


def test_list_ids_of_an_assigned_add_are_checked(fake):
    for kind, call in (("ivf", lambda i, lor: i.add(X, 0, lor)), ("ivfpq", lambda i, lor: i.add_codes(CODES, lor))):
        idx = make_index(kind)
        fake.clear()
        with pytest.raises(ValueError) as e:
            call(idx, LISTS[:4])
        assert str(e.value) == f"expected {N} list ids, got (4,)" and fake.log == []
        call(idx, LISTS.astype(np.int64))                      # converted to int32
        lor = fake.log[0][1][-1]
        assert np.array_equal(np.ctypeslib.as_array((ctypes.c_int32 * N).from_address(lor)), LISTS)


# (kind, the failing call, entry point that fails, a permitted difference)
FAILING_ADDS = [("flat", lambda i: i.add(X), "vdb_add", False), ("knng", lambda i: i.add(X), "vdb_add", False),
                ("pq", lambda i: i.add(X), "vdb_pq_add", False), ("pq", lambda i: i.add_codes(CODES), "vdb_pq_add_codes", False),
                ("ivfpq", lambda i: i.add_codes(CODES, LISTS), "vdb_ivfpq_add_codes", False),
                ("ivf", lambda i: i.add(X), "vdb_ivf_add", True), ("sq8", lambda i: i.add(X), "vdb_ivf_add", True),
                ("ivfpq", lambda i: i.add(X), "vdb_ivf_add", True), ("ivf", lambda i: i.add(X, 0, LISTS), "vdb_ivf_add_assigned", True)]


@pytest.mark.parametrize("kind,call,entry,permitted", FAILING_ADDS)
def test_a_failed_add_re_reads_ntotal(fake, kind, call, entry, permitted):
    from vdbhip import _ffi

    if permitted:
        permitted_difference()
    idx = make_index(kind)
    idx.ntotal = 99
    fake.clear()
    fake.fail[entry] = _ffi.VDB_ERR_INVALID
    fake.ntotal = 2
    with pytest.raises(ValueError) as e:              # an argument error of a build-time call
        call(idx)
    assert str(e.value) == "libvdbhip status 1"
    assert idx.ntotal == 2 and fake.names() == [entry, "vdb_last_error", "vdb_stats"]
    fake.fail[entry] = _ffi.VDB_ERR_HIP
    with pytest.raises(_ffi.VdbError):
        call(idx)


@pytest.mark.parametrize("kind", KINDS)
def test_reset(fake, kind):
    idx = make_index(kind)
    idx.ntotal = 99
    fake.clear()
    idx.reset()
    assert fake.calls("vdb_reset") == [(H,)]
    # the flat kinds re-read the library's count, the IVF and PQ kinds set 0
    assert (idx.ntotal, fake.names()) == ((N, ["vdb_reset", "vdb_stats"]) if kind in ("flat", "knng") else (0, ["vdb_reset"]))


def test_search_time_failures_are_runtime_errors(fake):
    from vdbhip import _ffi

    for kind, entry in (("flat", "vdb_search"), ("ivf", "vdb_ivf_search"), ("pq", "vdb_search")):
        idx = make_index(kind)
        fake.fail[entry] = _ffi.VDB_ERR_INVALID
        with pytest.raises(_ffi.VdbError):
            idx.search(Q, K)


# ---- plugin classes ---------------------------------------------------------------------------------------------------------------
def normalized(a):
    """algorithms._safe_normalize, restated."""
    a = np.array(a, dtype=F32)
    norms = np.linalg.norm(a, axis=1, keepdims=True)
    return np.divide(a, norms, out=np.zeros_like(a), where=norms > 0)


def normalized_by_row(a):
    out = np.zeros_like(np.asarray(a, dtype=F32))
    for i, row in enumerate(np.asarray(a, dtype=F32)):
        out[i] = row / np.linalg.norm(row)
    return out


def euclidean(d, i, metric):
    pad = i < 0
    d = np.sqrt(np.where(pad, F32(0), d)).astype(F32) if metric == "l2" else -d
    d[pad] = np.inf
    return d


def faiss_style(d, i, metric):
    return -d if metric in ("cosine", "ip") else d


def hamming(d, i, metric):
    d = d.astype(F32)
    d = -d if metric in ("cosine", "ip") else d
    d[i < 0] = np.inf
    return d


def one_minus(d, i, metric):
    if metric == "l2":
        return euclidean(d, i, metric)
    d = (F32(1.0) - d).astype(F32)
    d[i < 0] = np.inf
    return d


def _plugins():
    import vdbhip as v

    # name -> (indexer, its parameters, searcher, its parameters, metrics, entry point of a search, scalars after nq, width, first dtype,
    #          result convention, query normalisation for cosine, not-attached message, wrong-kind message)
    faiss = "FaissSearcher not attached to an index"
    return {
        "linear": (v.HipBruteForceIndexer, {}, v.HipLinearSearcher, {}, ("l2", "cosine", "ip"), "vdb_search", (K,), F32, euclidean,
                   normalized, "LinearSearcher not attached to an index", "HipLinearSearcher requires 'raw_vectors' artifact"),
        "ivf": (v.HipIVFIndexer, {"index_key": "IVF4,Flat"}, v.HipIVFSearcher, {}, ("l2", "cosine", "ip"), "vdb_ivf_search", (K,), F32,
                faiss_style, normalized, faiss, "HipIVFSearcher requires 'hip_ivf' artifact"),
        "ivfpq": (v.HipIVFPQIndexer, {"index_key": "IVF4,PQ4"}, v.HipIVFSearcher, {}, ("l2", "cosine", "ip"), "vdb_ivf_search", (K,), F32,
                  faiss_style, normalized, faiss, "HipIVFSearcher requires 'hip_ivf' artifact"),
        "pq": (v.HipPQIndexer, {"index_key": "PQ4"}, v.HipPQSearcher, {}, ("l2", "cosine", "ip"), "vdb_search", (K,), F32, faiss_style,
               normalized, faiss, "HipPQSearcher requires 'hip_pq' artifact"),
        "knng": (v.HipKnnGraphIndexer, {"M": 2}, v.HipKnnGraphSearcher, {}, ("l2", "cosine", "ip"), "vdb_knng_search", (K, 100), F32,
                 faiss_style, normalized, faiss, "HipKnnGraphSearcher requires 'hip_knng' artifact"),
        "lsh": (v.HipLSHIndexer, {"num_bits": 32}, v.HipLSHSearcher, {}, ("l2", "cosine", "ip"), "vdb_lsh_search", (K, N), F32, euclidean,
                normalized, faiss, "HipLSHSearcher requires 'hip_lsh' artifact"),
        "lsh_raw": (v.HipLSHIndexer, {"num_bits": 32}, v.HipLSHSearcher, {"lsh_rerank": False}, ("l2", "cosine", "ip"), "vdb_lsh_candidates",
                    (K,), np.int32, hamming, normalized, faiss, "HipLSHSearcher requires 'hip_lsh' artifact"),
        "lsh_tables": (v.HipLSHTableIndexer, {"num_tables": 2, "hash_size": 3}, v.HipLSHTableSearcher, {}, ("l2", "cosine"), "vdb_lsht_search",
                       (K, 16, 1), F32, one_minus, normalized_by_row, "LSHSearcher not attached to an index",
                       "HipLSHTableSearcher can only attach to artifacts produced by HipLSHTableIndexer"),
    }


PLUGINS = ("linear", "ivf", "ivfpq", "pq", "knng", "lsh", "lsh_raw", "lsh_tables")


@pytest.mark.parametrize("metric", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("plugin", PLUGINS)
def test_searchers(fake, plugin, metric):
    from vdbhip import IndexArtifact

    indexer, iparams, searcher, sparams, metrics, entry, scalars, first, convention, normalize, detached, wrong_kind = _plugins()[plugin]
    if metric not in metrics:
        with pytest.raises(ValueError, match="LSHIndexer supports metrics"):
            indexer("ix", DIM, metric, **iparams)
        return
    s = searcher("s", DIM, metric, **sparams)
    assert s.get_memory_usage() == 0.0
    for call in (lambda: s.batch_search(Q, K), lambda: s.search(Q[0], K)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert type(e.value) is RuntimeError and str(e.value) == detached
    with pytest.raises(ValueError) as e:
        s.attach(IndexArtifact(kind="something_else", data=None), X)
    assert str(e.value) == wrong_kind
    s.attach(indexer("ix", DIM, metric, **iparams).build(X), X)
    assert s.get_memory_usage() == 3.0
    fake.bytes_resident = 5 << 19
    assert s.get_memory_usage() == 2.5

    for queries in (Q, Q.astype(np.float64), np.asfortranarray(Q), Q[0]):
        fake.clear()
        before = queries.copy()
        single = queries.ndim == 1
        d, i = (s.search if single else s.batch_search)(queries, K)
        nq = 1 if single else NQ
        (got,) = fake.calls(entry)
        assert fake.names() == [entry] and got[0] == H and got[2:-2] == (nq,) + scalars
        ptr, seen = fake.matrix(entry)
        reach = np.array(queries, dtype=F32).reshape(nq, DIM)
        if metric == "cosine":
            reach = normalize(reach)
            if single and searcher is not _plugins()["linear"][2] and plugin != "lsh_tables":
                reach = normalize(reach)           # FaissSearcher.search prepares the query and hands it to batch_search, which prepares it again
        assert seen.dtype == F32 and np.array_equal(seen, reach)
        assert ptr != queries.ctypes.data and np.array_equal(queries, before)
        a, ids = canned(nq, K, first)
        want = convention(a, ids, metric)
        if single:
            want, ids = want[0], ids[0]
        assert d.dtype == F32 and i.dtype == np.int64 and d.shape == i.shape == ((K,) if single else (NQ, K))
        assert np.array_equal(d, want) and np.array_equal(np.signbit(d), np.signbit(want)) and np.array_equal(i, ids)


def _attach(fake, plugin, metric="l2", iextra=None, **sparams):
    indexer, iparams, searcher = _plugins()[plugin][:3]
    artifact = indexer("ix", DIM, metric, **dict(iparams, **(iextra or {}))).build(X)
    fake.clear()
    s = searcher("s", DIM, metric, **sparams)
    s.attach(artifact, X)
    return s, artifact


def test_attach_of_the_ivf_searcher(fake):
    for plugin in ("ivf", "ivfpq"):
        s, art = _attach(fake, plugin)
        assert fake.log == [] and s.index is art.data
        _attach(fake, plugin, nprobe=3)
        assert fake.log == [("vdb_ivf_set_nprobe", (H, 3))]
        s, art = _attach(fake, plugin, iextra={"nprobe": 2})
        assert fake.log == [("vdb_ivf_set_nprobe", (H, 2))] and art.data.nprobe == 2
        _attach(fake, plugin, iextra={"nprobe": 2}, nprobe=3)
        assert fake.log == [("vdb_ivf_set_nprobe", (H, 3))]
        s, art = _attach(fake, plugin, nprobe=3, adc_max_batch=16)
        assert sorted(fake.log) == [("vdb_ivf_set_nprobe", (H, 3)), ("vdb_set_option", (H, b"ivfpq_adc_max_batch", 16.0))]
        assert art.data.adc_max_batch == 16 and s.adc_max_batch == 16


def test_attach_of_the_pq_searcher(fake):
    s, art = _attach(fake, "pq")
    assert fake.log == [] and s.index is art.data and art.data.adc_max_batch == 0
    s, art = _attach(fake, "pq", adc_max_batch=16)
    assert fake.log == [("vdb_set_option", (H, b"pq_adc_max_batch", 16.0))] and art.data.adc_max_batch == 16
    s, art = _attach(fake, "pq", adc_max_batch=0)
    assert fake.log == [("vdb_set_option", (H, b"pq_adc_max_batch", 0.0))]


def _warm_up(fake, entry):
    (got,) = fake.calls(entry)
    assert fake.names() == [entry]
    return got[2:-2], fake.matrix(entry)[1]


def test_attach_of_the_graph_searcher(fake):
    for metric in ("l2", "cosine", "ip"):
        rows = normalized(X) if metric == "cosine" else X
        _attach(fake, "knng", metric)
        scalars, seen = _warm_up(fake, "vdb_knng_search")
        assert scalars == (N, 10, 100) and np.array_equal(seen, rows)
        s, _ = _attach(fake, "knng", metric, efSearch=7, reserve_queries=2)
        scalars, seen = _warm_up(fake, "vdb_knng_search")
        assert scalars == (2, 7, 7) and np.array_equal(seen, rows[:2]) and s.efSearch == 7
    s, _ = _attach(fake, "knng", iextra={"efSearch": 9, "reserve_queries": 3})
    assert _warm_up(fake, "vdb_knng_search")[0] == (3, 9, 9) and s.efSearch == 9
    _attach(fake, "knng", reserve_queries=0)
    assert fake.log == []
    with pytest.raises(ValueError) as e:
        _attach(fake, "knng", efSearch=600)
    assert str(e.value) == "efSearch must be in [1, 512], got 600"
    s, _ = _attach(fake, "knng", efSearch=7)
    fake.clear()
    s.batch_search(Q, 9)
    assert fake.calls("vdb_knng_search")[0][2:5] == (NQ, 9, 9)          # ef = max(efSearch, k)
    with pytest.raises(RuntimeError) as e:
        s.batch_search(Q, 513)
    assert str(e.value) == "the k-NN graph search returns at most 512 neighbours, got k = 513"


def test_attach_of_the_lsh_searcher(fake):
    for metric in ("l2", "cosine", "ip"):
        _attach(fake, "lsh", metric)
        scalars, seen = _warm_up(fake, "vdb_lsh_search")
        assert scalars == (N, 10, N) and np.array_equal(seen, X)           # the rows as given, for every metric
        _attach(fake, "lsh", metric, reserve_queries=2, lsh_max_candidates=3)
        scalars, seen = _warm_up(fake, "vdb_lsh_search")
        assert scalars == (2, 10, 3) and np.array_equal(seen, X[:2])
    _attach(fake, "lsh", iextra={"reserve_queries": 3})
    assert _warm_up(fake, "vdb_lsh_search")[0] == (3, 10, N)
    _attach(fake, "lsh", reserve_queries=0)
    assert fake.log == []
    _attach(fake, "lsh", lsh_max_candidates=0)
    assert fake.log == []
    s, _ = _attach(fake, "lsh", lsh_candidate_multiplier=1.0)
    fake.clear()
    s.batch_search(Q, 2)
    assert fake.calls("vdb_lsh_search")[0][2:5] == (NQ, 2, 2)
    fake.ntotal = 0
    s.index._sync_ntotal()
    with pytest.raises(RuntimeError) as e:
        s.batch_search(Q, 2)
    assert str(e.value) == "LSH index has no vectors to search"


def test_attach_of_the_linear_and_table_searchers(fake):
    import vdbhip
    from vdbhip import IndexArtifact

    for plugin in ("linear", "lsh_tables"):
        s, art = _attach(fake, plugin)
        assert fake.log == []
    for metric, code in (("l2", 0), ("cosine", 1), ("ip", 1)):
        fake.clear()
        s = vdbhip.HipLinearSearcher("s", DIM, metric, engine_options={"stream_panels": 1}, reserve_queries=64)
        s.attach(IndexArtifact(kind="raw_vectors", data=X.astype(np.float64), metadata={"metric": metric}), X)   # the reference's artifact
        assert fake.log[0] == ("create", (DIM, code, 0))
        assert fake.names() == ["create", "vdb_set_option", "vdb_add", "vdb_stats", "vdb_reserve"]
        assert fake.calls("vdb_set_option") == [(H, b"stream_panels", 1.0)] and fake.calls("vdb_reserve") == [(H, 64, 10)]
        assert np.array_equal(fake.matrix("vdb_add")[1], normalized(X) if metric == "cosine" else X)
    with pytest.raises(ValueError, match="Vector dimension mismatch in LinearSearcher"):
        vdbhip.HipLinearSearcher("s", DIM + 1).attach(IndexArtifact(kind="raw_vectors", data=X), X)
    s = vdbhip.HipLinearSearcher("s", DIM, "hamming")
    s.attach(IndexArtifact(kind="raw_vectors", data=X), X)
    with pytest.raises(ValueError, match="Unsupported metric 'hamming' for LinearSearcher"):
        s.batch_search(Q, K)
    s = vdbhip.HipLinearSearcher("s", DIM)
    s.attach(vdbhip.HipBruteForceIndexer("ix", DIM).build(X[:0]), X[:0])
    with pytest.raises(RuntimeError, match="LinearSearcher cannot operate on empty index"):
        s.batch_search(Q, K)
    with pytest.raises(ValueError, match="the LSH candidate cap is at most 65536, got 65537"):
        _attach(fake, "lsh_tables", max_candidates=65537)[0].batch_search(Q, K)


# ---- indexers: calls of a build, rows handed to the add, artifact -----------------------------------------------------------------
FAISS_META = {"l2": {"faiss_metric": "l2"}, "ip": {"faiss_metric": "ip"},
              "cosine": {"faiss_metric": "ip", "normalize_queries": True, "normalize_vectors": True}}
OPTS = {"engine_options": {"stream_panels": 1}}
OPT_CALL = ("vdb_set_option", (H, b"stream_panels", 1.0))
TRAIN_KW = {"niter": 2, "seed": 7, "max_points_per_centroid": 9}


def _indexers():
    import vdbhip as v

    # name -> (class, parameters, metrics, artifact kind, add entry point, calls of a build after `create` as (name, arguments or None),
    #          metadata(metric))
    reserve = ("vdb_reserve", (H, 10_000, 10))
    stats = ("vdb_stats", None)
    return {
        "brute": (v.HipBruteForceIndexer, OPTS, ("l2", "cosine", "ip"), "raw_vectors", "vdb_add",
                  [OPT_CALL, ("vdb_add", None), stats, reserve],
                  lambda m: {"metric": m, "normalize_vectors": m == "cosine", "hip_index_metric": m}),
        "ivf_flat": (v.HipIVFIndexer, dict(OPTS, index_key="IVF4,Flat", nprobe=3, adc_max_batch=16, **TRAIN_KW), ("l2", "cosine", "ip"), "hip_ivf",
                     "vdb_ivf_add", [("vdb_ivf_train", None), ("vdb_ivf_add", None), stats, ("vdb_ivf_set_nprobe", (H, 3)), reserve],
                     lambda m: dict({"metric": m, "index_key": "IVF4,Flat", "nprobe": 3}, **FAISS_META[m])),
        "ivf_sq8": (v.HipIVFIndexer, dict(index_type="IVF4,SQ8", reserve_queries=0), ("l2", "cosine", "ip"), "hip_ivf", "vdb_ivf_add",
                    [("vdb_ivf_set_codec", (H, 1)), ("vdb_ivf_train", None), ("vdb_ivf_add", None), stats],
                    lambda m: dict({"metric": m, "index_key": "IVF4,SQ8"}, **FAISS_META[m])),
        "pq": (v.HipPQIndexer, dict(OPTS, index_key="PQ4", adc_max_batch=16, **TRAIN_KW), ("l2", "cosine", "ip"), "hip_pq", "vdb_pq_add",
               [("vdb_set_option", (H, b"pq_adc_max_batch", 16.0)), OPT_CALL, ("vdb_pq_train", None), ("vdb_pq_add", None), stats, reserve],
               lambda m: dict({"metric": m, "index_key": "PQ4"}, **FAISS_META[m])),
        "ivfpq": (v.HipIVFPQIndexer, dict(OPTS, index_key="IVF4,PQ4", adc_max_batch=16, nprobe=3, reserve_queries=64, **TRAIN_KW),
                  ("l2", "cosine", "ip"), "hip_ivf", "vdb_ivf_add",
                  [("vdb_ivf_set_codec", (H, 2)), ("vdb_set_option", (H, b"ivfpq_adc_max_batch", 16.0)), ("vdb_ivf_train", None),
                   ("vdb_ivfpq_train", None), ("vdb_ivf_add", None), stats, ("vdb_ivf_set_nprobe", (H, 3)), ("vdb_reserve", (H, 64, 10))],
                  lambda m: dict({"metric": m, "index_key": "IVF4,PQ4", "nprobe": 3}, **FAISS_META[m])),
        "knng": (v.HipKnnGraphIndexer, dict(OPTS, M=2, efSearch=9, efConstruction=50, reserve_queries=64), ("l2", "cosine", "ip"), "hip_knng",
                 "vdb_add", [OPT_CALL, ("vdb_add", None), stats, ("vdb_reserve", (H, 64, 10)), ("vdb_knng_build", (H, 4, 8))],
                 lambda m: dict({"metric": m, "efSearch": 9, "efConstruction": 50, "M": 2, "degree": 4, "ncand": 8, "reserve_queries": 64},
                                **FAISS_META[m])),
        "lsh": (v.HipLSHIndexer, dict(OPTS, num_bits=32, seed=5), ("l2", "cosine", "ip"), "hip_lsh", "vdb_add",
                [OPT_CALL, ("vdb_lsh_set_projection", None), ("vdb_add", None), stats, reserve],
                lambda m: dict({"metric": m, "num_bits": 32, "faiss_index_kind": "lsh", "seed": 5, "reserve_queries": None},
                               **{"l2": {}, "cosine": {"normalize_queries": True}, "ip": {"faiss_metric": "ip"}}[m])),
        "lsh_tables": (v.HipLSHTableIndexer, dict(OPTS, num_tables=2, hash_size=3, bucket_width=2.0), ("l2", "cosine"), "hip_lsh_tables", "vdb_add",
                       [OPT_CALL, ("vdb_lsht_set_tables", None), ("vdb_add", None), stats, reserve],
                       lambda m: dict({"metric": m, "num_tables": 2, "hash_size": 3},
                                      **({"normalize_queries": True} if m == "cosine" else {"bucket_width": 2.0}))),
    }


INDEXERS = ("brute", "ivf_flat", "ivf_sq8", "pq", "ivfpq", "knng", "lsh", "lsh_tables")
TRAIN_ARGS = {"vdb_ivf_train": (NLIST,), "vdb_pq_train": (M,), "vdb_ivfpq_train": (M,)}


def check_build(fake, metric, add_entry, calls, params):
    """The log of one build: create with the library metric, then `calls` in order; rows normalised for cosine only."""
    kmeans = (2, 7, 9) if "niter" in params else (25, 1234, 256)
    assert fake.log[0] == ("create", (DIM, 0 if metric == "l2" else 1, 0))
    log = fake.log[1:]
    assert [n for n, _ in log] == [n for n, _ in calls]
    for (name, got), (_, want) in zip(log, calls):
        if want is not None:
            assert got == want, name
    rows = normalized(X) if metric == "cosine" else X
    for name, got in log:
        if name in TRAIN_ARGS:                     # trained on the rows that are added, with the configured k-means parameters
            assert got[1:2] + got[3:] == TRAIN_ARGS[name] + (N,) + kmeans
            assert np.array_equal(fake.matrix(name)[1], rows)
    (added,) = fake.calls(add_entry)
    assert added[2:] == (N, 0) and np.array_equal(fake.matrix(add_entry)[1], rows)
    return rows


@pytest.mark.parametrize("metric", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("name", INDEXERS)
def test_indexers(fake, name, metric):
    import vdbhip

    cls, params, metrics, kind, add_entry, calls, metadata = _indexers()[name]
    if metric not in metrics:
        return
    art = cls("ix", DIM, metric, **params).build(X)
    check_build(fake, metric, add_entry, calls, params)
    meta = dict(art.metadata)
    if name == "brute":
        assert type(meta.pop("hip_index")) is vdbhip.FlatIndex and art.data is X          # the raw store, not a copy
    else:
        assert art.data.ntotal == N
    assert art.kind == kind and meta == metadata(metric)
    for key, value in metadata(metric).items():
        assert type(meta[key]) is type(value), key
    if name == "lsh":
        got = fake.calls("vdb_lsh_set_projection")[0]
        assert got[:2] == (H, 32)
    if name == "lsh_tables":
        got = fake.calls("vdb_lsht_set_tables")[0]
        assert got[:4] == (H, 2, 3, 1 if metric == "l2" else 0) and (got[5] is None) == (metric != "l2")
        assert got[6] == (2.0 if metric == "l2" else 0.0)


def test_indexer_refusals(fake):
    import vdbhip as v

    def refused(make, message, exact=True):
        fake.clear()
        with pytest.raises(ValueError) as e:
            make()
        assert (str(e.value) == message) if exact else (message in str(e.value)), str(e.value)
        assert fake.log == []

    pq3 = "PQ3 needs a dimension that is a multiple of 3 (and M <= 256); got 8"
    ivf_key = "unsupported index key {!r}: only 'IVF<nlist>,Flat' and 'IVF<nlist>,SQ8' are implemented on the HIP backend"
    pq_key = "unsupported index key {!r}: only 'PQ<M>' (8 bits per sub-vector) is implemented here"
    ivfpq_key = "unsupported index key {!r}: only 'IVF<nlist>,PQ<M>' (8 bits per sub-vector) is implemented here"
    one_gpu_pq = "PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available"
    one_gpu_ivfpq = "IVF<nlist>,PQ<M> runs on one GPU: a multi-device index (more than one device id) is not available"
    refused(lambda: v.HipIVFIndexer("ix", DIM, index_key="PQ4"), ivf_key.format("PQ4"))
    refused(lambda: v.HipIVFIndexer("ix", DIM, index_type="IVF4,PQ4"), ivf_key.format("IVF4,PQ4"))
    refused(lambda: v.HipApproximateSearch("a", DIM, index_type="IVF4,PQ4"), ivf_key.format("IVF4,PQ4"))
    refused(lambda: v.HipPQIndexer("ix", DIM, index_key="PQ3"), pq3)
    refused(lambda: v.HipPQIndexer("ix", DIM, index_key="IVF4,Flat"), pq_key.format("IVF4,Flat"))
    refused(lambda: v.HipPQSearch("a", DIM, index_type="PQ3"), pq3)
    refused(lambda: v.HipPQSearch("a", DIM, index_type="PQ4x4"), pq_key.format("PQ4x4"))
    refused(lambda: v.HipPQSearch("a", DIM, index_type="PQ4", device_ids=[0, 1]), one_gpu_pq)
    refused(lambda: v.HipIVFPQIndexer("ix", DIM, index_key="IVF4,PQ3"), pq3)
    refused(lambda: v.HipIVFPQIndexer("ix", DIM, index_key="IVF4,Flat"), ivfpq_key.format("IVF4,Flat"))
    refused(lambda: v.HipIVFPQIndexer("ix", DIM, index_key="IVF4,PQ4", device_ids=[0, 1]), one_gpu_ivfpq)
    refused(lambda: v.HipIVFPQSearch("a", DIM, index_type="IVF4,PQ3"), pq3)
    refused(lambda: v.HipIVFPQSearch("a", DIM, index_type="IVF4,PQ4", device=[0, 1]), one_gpu_ivfpq)
    refused(lambda: v.HipPQIndexer("ix", DIM, index_key="PQ4", device_ids=[0, 1]).build(X), one_gpu_pq)
    refused(lambda: v.HipIVFIndexer("ix", DIM, index_key="IVF4,SQ8", device_ids=[0, 1]).build(X),
            "IVF<nlist>,SQ8 runs on one GPU: a multi-device index (more than one device id) is not available for the SQ8 codec")
    refused(lambda: v.HipKnnGraphIndexer("ix", DIM, "dot"), "HipKnnGraphIndexer supports metrics {", exact=False)
    refused(lambda: v.HipKnnGraphIndexer("ix", DIM, "dot"), "}, received 'dot'", exact=False)
    for cls in (v.HipKnnGraphIndexer, v.HipKnnGraphSearch):
        refused(lambda: cls("ix", DIM, M=1), "M must be in [2, 32] (degree = 2 M in [4, 64]), got 1")
        refused(lambda: cls("ix", DIM, M=2, ncand=3), "ncand must be in [degree = 4, 128], got 3")
        refused(lambda: cls("ix", DIM, efSearch=0), "efSearch must be in [1, 512], got 0")
    refused(lambda: v.HipLSHIndexer("ix", DIM, "dot"), "FaissLSHIndexer supports metrics {", exact=False)
    refused(lambda: v.HipLSHIndexer("ix", DIM, num_bits=0), "num_bits must be positive")
    refused(lambda: v.HipLSHIndexer("ix", DIM, num_bits=48), "num_bits must be a multiple of 32 in [32, 1024]")
    for cls in (v.HipLSHTableIndexer, v.HipLSHTables):
        refused(lambda: cls("ix", DIM, "ip"), "LSHIndexer supports metrics {", exact=False)
        refused(lambda: cls("ix", DIM, hash_size=0), "hash_size must be positive")
        refused(lambda: cls("ix", DIM, num_tables=0), "num_tables must be positive")
        refused(lambda: cls("ix", DIM, "l2", bucket_width=0.0), "bucket_width must be positive for L2 LSH")
    for cls in (v.HipLSHTableSearcher, v.HipLSHTables):
        refused(lambda: cls("s", DIM, candidate_multiplier=0), "candidate_multiplier must be positive")
    # build-time shape refusals
    refused(lambda: v.HipBruteForceIndexer("ix", DIM).build(X[:, :7]), "Vector dimension mismatch in HipBruteForceIndexer")
    for cls, params in ((v.HipPQIndexer, {"index_key": "PQ4"}), (v.HipIVFPQIndexer, {"index_key": "IVF4,PQ4"}), (v.HipKnnGraphIndexer, {}),
                        (v.HipLSHIndexer, {"num_bits": 32})):
        refused(lambda: cls("ix", DIM + 8, **params).build(X), f"Expected dimension {DIM + 8}, got {DIM}")
    refused(lambda: v.HipLSHTableIndexer("ix", DIM + 8).build(X), f"Expected vectors with dimension {DIM + 8}, received {DIM}")
    refused(lambda: v.HipLSHTables("a", DIM + 8).build_index(X), f"Expected vectors with dimension {DIM + 8}, received {DIM}")
    refused(lambda: v.HipKnnGraphSearch("a", DIM + 8).build_index(X), f"Expected vectors of dimension {DIM + 8}, got {DIM}")
    refused(lambda: v.HipExactSearch("a", DIM + 8).build_index(X), f"expected (n, {DIM + 8}) vectors, got ({N}, {DIM})")
    art = v.HipBruteForceIndexer("ix", DIM, "hamming").build(X)             # an unknown metric only breaks at search time
    assert art.metadata == {"metric": "hamming", "normalize_vectors": False} and art.data is X


# ---- stand-alone algorithms ---------------------------------------------------------------------------------------------------------
def _algorithms():
    import vdbhip as v

    reserve, stats = ("vdb_reserve", (H, 10_000, 10)), ("vdb_stats", None)
    # name -> (class, parameters, {constructor metric: library metric}, normalises for, add entry point, calls of a build, search entry point,
    #          scalars of a search after nq, not-built message)
    built = "Index has not been built yet."
    return {
        "exact": (v.HipExactSearch, OPTS, {"l2": "l2", "cosine": "ip", "ip": "ip"}, (), "vdb_add",
                  [OPT_CALL, ("vdb_add", None), stats, reserve], "vdb_search", (K,), built),
        "ivf": (v.HipApproximateSearch, dict(OPTS, index_type="IVF4,Flat", nprobe=3, adc_max_batch=16, **TRAIN_KW),
                {"l2": "l2", "cosine": "ip", "ip": "ip"}, (), "vdb_ivf_add",
                [("vdb_ivf_train", None), ("vdb_ivf_add", None), stats, ("vdb_ivf_set_nprobe", (H, 3)), reserve], "vdb_ivf_search", (K,), built),
        "sq8": (v.HipApproximateSearch, dict(index_type="IVF4,SQ8", reserve_queries=0), {"l2": "l2", "ip": "ip"}, (), "vdb_ivf_add",
                [("vdb_ivf_set_codec", (H, 1)), ("vdb_ivf_train", None), ("vdb_ivf_add", None), stats], "vdb_ivf_search", (K,), built),
        "pq": (v.HipPQSearch, dict(OPTS, index_type="PQ4", adc_max_batch=16, **TRAIN_KW), {"l2": "l2", "cosine": "ip", "ip": "ip"}, (), "vdb_pq_add",
               [("vdb_set_option", (H, b"pq_adc_max_batch", 16.0)), OPT_CALL, ("vdb_pq_train", None), ("vdb_pq_add", None), stats, reserve],
               "vdb_search", (K,), built),
        "pq_plain": (v.HipPQSearch, dict(index_type="PQ4"), {"l2": "l2"}, (), "vdb_pq_add",
                     [("vdb_pq_train", None), ("vdb_pq_add", None), stats, reserve], "vdb_search", (K,), built),
        "ivfpq": (v.HipIVFPQSearch, dict(OPTS, index_type="IVF4,PQ4", adc_max_batch=16, nprobe=3, **TRAIN_KW),
                  {"l2": "l2", "cosine": "ip", "ip": "ip"}, (), "vdb_ivf_add",
                  [("vdb_ivf_set_codec", (H, 2)), ("vdb_set_option", (H, b"ivfpq_adc_max_batch", 16.0)), ("vdb_ivf_train", None),
                   ("vdb_ivfpq_train", None), ("vdb_ivf_add", None), stats, ("vdb_ivf_set_nprobe", (H, 3)), reserve], "vdb_ivf_search", (K,), built),
        "knng": (v.HipKnnGraphSearch, dict(OPTS, M=2, efSearch=9), {"l2": "l2", "cosine": "ip", "dot": "ip", "ip": "l2"}, ("cosine",), "vdb_add",
                 [OPT_CALL, ("vdb_add", None), stats, reserve, ("vdb_knng_build", (H, 4, 8)), ("vdb_knng_search", None)], "vdb_knng_search",
                 (K, 9), "Index not built. Call build_index() first."),
        "lsh_tables": (v.HipLSHTables, dict(OPTS, num_tables=2, hash_size=3), {"l2": "l2", "cosine": "ip"}, ("cosine",), "vdb_add",
                       [OPT_CALL, ("vdb_lsht_set_tables", None), ("vdb_add", None), stats, reserve], "vdb_lsht_search", (K, 16, 1),
                       "Index has not been built for LSH algorithm"),
    }


ALGORITHMS = ("exact", "ivf", "sq8", "pq", "pq_plain", "ivfpq", "knng", "lsh_tables")


@pytest.mark.parametrize("metric", ["l2", "cosine", "ip", "dot"])
@pytest.mark.parametrize("name", ALGORITHMS)
def test_algorithms(fake, name, metric):
    cls, params, metrics, normalizes, add_entry, calls, entry, scalars, not_built = _algorithms()[name]
    if metric not in metrics:
        return
    a = cls("a", DIM, metric=metric, **params)
    assert fake.log == [] and a.get_memory_usage() == 0.0
    for call in (lambda: a.batch_search(Q, K), lambda: a.search(Q[0], K)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert type(e.value) is RuntimeError and str(e.value) == not_built
    a.build_index(X)
    rows = check_build(fake, "cosine" if metric in normalizes else metrics[metric], add_entry, calls, params)
    if metric not in normalizes:
        assert np.array_equal(rows, X)
    if name == "knng":                             # the warm-up search: the rows of the index as queries
        assert fake.calls("vdb_knng_search")[0][2:5] == (N, 9, 9) and np.array_equal(fake.matrix("vdb_knng_search")[1], rows)
    assert a.index_built and a.get_memory_usage() == 3.0 and a.index.ntotal == N
    norm = normalized_by_row if name == "lsh_tables" else normalized
    for queries in (Q, Q.astype(np.float64), np.asfortranarray(Q), Q[0]):
        fake.clear()
        single = queries.ndim == 1
        d, i = (a.search if single else a.batch_search)(queries, K)
        nq = 1 if single else NQ
        (got,) = fake.calls(entry)
        assert fake.names() == [entry] and got[0] == H and got[2:-2] == (nq,) + scalars
        reach = np.array(queries, dtype=F32).reshape(nq, DIM)
        assert np.array_equal(fake.matrix(entry)[1], norm(reach) if metric in normalizes else reach)
        want, ids = canned(nq, K)
        if name == "lsh_tables":
            want = one_minus(want, ids, metric)
        if single:
            want, ids = want[0], ids[0]
        assert d.dtype == F32 and i.dtype == np.int64 and np.array_equal(d, want) and np.array_equal(i, ids)
    if name == "exact":
        assert a.get_operations() == {"ndis": float(3 * NQ * N)}        # batch_search counts, search does not

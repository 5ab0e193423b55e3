"""Which entry point each kind of handle accepts (test infrastructure only; tests/test_gpu_admission.py asserts it cell for
cell against tests/golden/admission_matrix.json, which tests/golden/make_admission_matrix.py recorded).

`STATES`      name -> builder of a fresh single-purpose handle, the smallest shapes that reach the state.
`entries(c)`  every vdb_* function of include/vdbhip.h that takes a handle, with ONE set of valid arguments each (non-null, in
              range, M = 8, k = 5, 5 queries); vdb_ivf_set_codec and vdb_set_option appear once per listed argument.
`run_state`   calls every entry on a handle of the state and returns {entry: rc}.  A refused call must leave the handle as it
              was, so the handle is reused across cells and rebuilt only after a cell that returned VDB_OK.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np

F32 = np.float32
NQ, K, M, NLIST, NCAND, EF, NBITS = 5, 5, 8, 8, 16, 16, 64
SENTINEL = "null pointer"        # what vdb_device_count(NULL) leaves in vdb_last_error: set in front of every cell


class Ctx:
    """The arguments of one state: `n` rows of `d` dimensions (host and device), 5 queries, and the output buffers, all sized
    for the state's own row count plus one more add."""

    def __init__(self, d, n, byte_valued=False):
        import torch

        rng = np.random.default_rng(1000 * d + n)
        self.d, self.n = d, n
        if byte_valued:
            self.X = rng.integers(0, 200, size=(n, d)).astype(F32)
            self.Q = rng.integers(0, 200, size=(NQ, d)).astype(F32)
        else:
            self.X = rng.standard_normal((n, d)).astype(F32)
            self.Q = rng.standard_normal((NQ, d)).astype(F32)
        self.C = self.X[:NLIST].copy()
        self.lists = (np.arange(n) % NLIST).astype(np.int32)
        self.cb = (rng.standard_normal((M, 256, d // M)) * (40 if byte_valued else 1)).astype(F32)
        self.R = rng.standard_normal((NBITS, d)).astype(F32)
        self.ring = np.full((n, 4), -1, np.int32)                # the graph of test_gpu_knng.test_refusals_in_both_orders
        self.ring[:, 0] = (np.arange(n) + 1) % n
        self.codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
        self.vmin, self.vdiff = np.full(d, -4, F32), np.full(d, 8, F32)
        self.cand = np.tile(np.arange(4, dtype=np.int64), (NQ, 1))
        rows = 2 * n + 4096                                      # no getter of this module writes more rows than that
        self.D, self.I = np.empty((NQ, NCAND), F32), np.empty((NQ, NCAND), np.int64)
        self.ham = np.empty((NQ, NCAND), np.int32)
        self.bytes_out = np.empty((rows, max(d, M)), np.uint8)
        self.words_out = np.empty((rows, 64), np.int32)
        self.floats_out = np.empty(max(256 * d, NBITS * d, NQ * 16), F32)
        self.floats_out2 = np.empty(max(d, NQ), F32)
        self.cscale = ctypes.c_double(0)
        self.int_out = ctypes.c_int(0)
        self.tX, self.tQ, self.tcand = (torch.from_numpy(a).cuda() for a in (self.X, self.Q, self.cand))
        self.tD = torch.empty((NQ, NCAND), dtype=torch.float32, device="cuda")
        self.tI = torch.empty((NQ, NCAND), dtype=torch.int64, device="cuda")
        self.tkeys = torch.empty((NQ, NCAND), dtype=torch.float64, device="cuda")
        self.tham = torch.empty((NQ, NCAND), dtype=torch.int32, device="cuda")


@lru_cache(maxsize=4)
def ctx(d, n, byte_valued=False):
    return Ctx(d, n, byte_valued)


def entries(c):
    """[(name, function name, arguments behind the handle)]"""
    from vdbhip._ffi import Stats, ptr

    X, Q, n = ptr(c.X), ptr(c.Q), c.n
    D, I = ptr(c.D), ptr(c.I)
    tX, tQ, tD, tI = c.tX.data_ptr(), c.tQ.data_ptr(), c.tD.data_ptr(), c.tI.data_ptr()
    out = [
        ("vdb_add", "vdb_add", (X, n, 0)),
        ("vdb_add_device", "vdb_add_device", (tX, n, 0, None)),
        ("vdb_search", "vdb_search", (Q, NQ, K, D, I)),
        ("vdb_search_device", "vdb_search_device", (tQ, NQ, K, tD, tI, None)),
        ("vdb_search_partial_device", "vdb_search_partial_device", (tQ, NQ, K, c.tkeys.data_ptr(), tI, None)),
        ("vdb_rerank", "vdb_rerank", (Q, NQ, ptr(c.cand), 4, 2, D, I)),
        ("vdb_rerank_device", "vdb_rerank_device", (tQ, NQ, c.tcand.data_ptr(), 4, 2, tD, tI, None)),
        ("vdb_ivf_train", "vdb_ivf_train", (NLIST, X, n, 2, 1, 256)),
        ("vdb_ivf_set_centroids", "vdb_ivf_set_centroids", (ptr(c.C), NLIST)),
        ("vdb_ivf_get_centroids", "vdb_ivf_get_centroids", (ptr(c.floats_out),)),
        ("vdb_ivf_add", "vdb_ivf_add", (X, n, 0)),
        ("vdb_ivf_add_assigned", "vdb_ivf_add_assigned", (X, n, 0, ptr(c.lists))),
        ("vdb_ivf_set_nprobe", "vdb_ivf_set_nprobe", (4,)),
        ("vdb_ivf_get_assignment", "vdb_ivf_get_assignment", (ptr(c.words_out),)),
        ("vdb_ivf_search", "vdb_ivf_search", (Q, NQ, K, D, I)),
        ("vdb_ivf_search_device", "vdb_ivf_search_device", (tQ, NQ, K, tD, tI, None)),
        ("vdb_ivf_search_partial_device", "vdb_ivf_search_partial_device", (tQ, NQ, K, c.tkeys.data_ptr(), tI, None)),
        ("vdb_ivf_set_codec(0)", "vdb_ivf_set_codec", (0,)),
        ("vdb_ivf_set_codec(1)", "vdb_ivf_set_codec", (1,)),
        ("vdb_ivf_set_codec(2)", "vdb_ivf_set_codec", (2,)),
        ("vdb_ivf_sq8_train_ranges", "vdb_ivf_sq8_train_ranges", (X, n)),
        ("vdb_ivf_sq8_set_ranges", "vdb_ivf_sq8_set_ranges", (ptr(c.vmin), ptr(c.vdiff))),
        ("vdb_ivf_sq8_get_ranges", "vdb_ivf_sq8_get_ranges", (ptr(c.floats_out), ptr(c.floats_out2))),
        ("vdb_ivf_get_codes", "vdb_ivf_get_codes", (ptr(c.bytes_out),)),
        ("vdb_ivfpq_train", "vdb_ivfpq_train", (M, X, n, 2, 1, 256)),
        ("vdb_ivfpq_set_codebooks", "vdb_ivfpq_set_codebooks", (M, ptr(c.cb))),
        ("vdb_ivfpq_get_codebooks", "vdb_ivfpq_get_codebooks", (ctypes.byref(c.int_out), ptr(c.floats_out))),
        ("vdb_ivfpq_add_codes", "vdb_ivfpq_add_codes", (ptr(c.codes), n, 0, ptr(c.lists))),
        ("vdb_ivfpq_get_codes", "vdb_ivfpq_get_codes", (ptr(c.bytes_out),)),
        ("vdb_lsh_set_projection", "vdb_lsh_set_projection", (NBITS, ptr(c.R))),
        ("vdb_lsh_get_projection", "vdb_lsh_get_projection", (ctypes.byref(c.int_out), ptr(c.floats_out))),
        ("vdb_lsh_get_codes", "vdb_lsh_get_codes", (ptr(c.words_out),)),
        ("vdb_lsh_candidates", "vdb_lsh_candidates", (Q, NQ, NCAND, ptr(c.ham), I)),
        ("vdb_lsh_candidates_device", "vdb_lsh_candidates_device", (tQ, NQ, NCAND, c.tham.data_ptr(), tI, None)),
        ("vdb_lsh_search", "vdb_lsh_search", (Q, NQ, K, NCAND, D, I)),
        ("vdb_lsh_search_device", "vdb_lsh_search_device", (tQ, NQ, K, NCAND, tD, tI, None)),
        ("vdb_pq_train", "vdb_pq_train", (M, X, n, 2, 1, 256)),
        ("vdb_pq_set_codebooks", "vdb_pq_set_codebooks", (M, ptr(c.cb))),
        ("vdb_pq_get_codebooks", "vdb_pq_get_codebooks", (ctypes.byref(c.int_out), ptr(c.floats_out))),
        ("vdb_pq_add", "vdb_pq_add", (X, n, 0)),
        ("vdb_pq_add_codes", "vdb_pq_add_codes", (ptr(c.codes), n, 0)),
        ("vdb_pq_get_codes", "vdb_pq_get_codes", (ptr(c.bytes_out),)),
        ("vdb_knng_build", "vdb_knng_build", (8, 16)),
        ("vdb_knng_set", "vdb_knng_set", (4, ptr(c.ring))),
        ("vdb_knng_get", "vdb_knng_get", (ctypes.byref(c.int_out), ptr(c.words_out))),
        ("vdb_knng_search", "vdb_knng_search", (Q, NQ, K, EF, D, I)),
        ("vdb_knng_search_device", "vdb_knng_search_device", (tQ, NQ, K, EF, tD, tI, None)),
        ("vdb_reserve", "vdb_reserve", (NQ, K)),
        ("vdb_stats", "vdb_stats", (ctypes.byref(Stats()),)),
        ("vdb_debug_scan_scores", "vdb_debug_scan_scores",
         (Q, NQ, 0, 16, ptr(c.floats_out), ptr(c.floats_out2), ctypes.byref(c.cscale))),
        ("vdb_reset", "vdb_reset", ()),
    ]
    for name, value in (("int8_only", 1), ("stream_panels", 1), ("graph", 1), ("flat_shape", 32), ("f16_group", 4), ("i8_group", 4),
                        ("ivf_bt", 4)):
        out.append((f"vdb_set_option({name}={value})", "vdb_set_option", (name.encode(), float(value))))
    return out


# ---- states ------------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, d, n, steps, search=None, devices=0, byte_valued=False):
        self.d, self.n, self.steps, self.search, self.devices, self.byte_valued = d, n, steps, search, devices, byte_valued


def _opt(name, value):
    return lambda c: ("vdb_set_option", (name.encode(), float(value)))


def _call(fn, *names):
    from vdbhip._ffi import ptr

    return lambda c: (fn, tuple(ptr(getattr(c, a)) if isinstance(a, str) else (c.n if a is None else a) for a in names))


_ADD = _call("vdb_add", "X", None, 0)
_CENTROIDS = _call("vdb_ivf_set_centroids", "C", NLIST)
_IVF_ADD = _call("vdb_ivf_add", "X", None, 0)


def _codec(i):
    return lambda c: ("vdb_ivf_set_codec", (i,))


STATES = {
    "01_flat_empty": State(32, 2000, ()),
    "02_flat_rows": State(32, 2000, (_ADD,), "vdb_search"),
    "03_flat_graph_option": State(32, 2000, (_opt("graph", 1), _ADD), "vdb_search"),
    "04_flat_int8_only_option": State(32, 2000, (_opt("int8_only", 1), _ADD), "vdb_search"),
    # the option took effect (more than 32 768 byte-valued rows, D <= 128) and was then set back: only h->int8_only says so
    "05_flat_int8_only_effect": State(16, 40000, (_opt("int8_only", 1), _ADD, _opt("int8_only", 0)), "vdb_search", byte_valued=True),
    # the fp16 panels of a D > 128 index are streamed above the 2048 rows the dense path serves
    "06_flat_panels_streamed": State(136, 2560, (_opt("stream_panels", 1), _ADD), "vdb_search"),
    "07_lsh": State(32, 2000, (_call("vdb_lsh_set_projection", NBITS, "R"), _ADD), "vdb_lsh_search"),
    "08_knng": State(32, 2000, (_ADD, _call("vdb_knng_set", 4, "ring")), "vdb_knng_search"),
    "09_ivf_flat_centroids": State(32, 2000, (_CENTROIDS,)),
    "10_ivf_flat_built": State(32, 2000, (_CENTROIDS, _IVF_ADD), "vdb_ivf_search"),
    "11_sq8_codec_only": State(32, 2000, (_codec(1),)),
    "12_sq8_built": State(32, 2000, (_codec(1), _CENTROIDS, _call("vdb_ivf_sq8_train_ranges", "X", None), _IVF_ADD), "vdb_ivf_search"),
    "13_ivfpq_codec_only": State(32, 2000, (_codec(2),)),
    "14_ivfpq_built": State(32, 2000, (_codec(2), _CENTROIDS, _call("vdb_ivfpq_set_codebooks", M, "cb"), _IVF_ADD), "vdb_ivf_search"),
    "15_pq_codebooks": State(32, 2000, (_call("vdb_pq_set_codebooks", M, "cb"),)),
    "16_pq_rows": State(32, 2000, (_call("vdb_pq_set_codebooks", M, "cb"), _call("vdb_pq_add", "X", None, 0)), "vdb_search"),
    "17_multi_flat_rows": State(32, 2000, (_ADD,), "vdb_search", devices=2),
    "18_multi_ivf_built": State(32, 2000, (_CENTROIDS, _IVF_ADD), "vdb_ivf_search", devices=2),
}


def build(lib, s, c):
    from vdbhip import _ffi

    h = _ffi.create_handle(c.d, _ffi.METRIC_L2, [0] * s.devices if s.devices else 0)
    for step in s.steps:
        fn, args = step(c)
        rc = getattr(lib, fn)(h, *args)
        if rc != _ffi.VDB_OK:
            lib.vdb_destroy(h)
            raise RuntimeError(f"state builder: {fn} returned {rc}: {_ffi.last_error()}")
    return h


def own_search(lib, s, c, h):
    """(D, I) of the kind's own search of the 5 queries, as bytes"""
    from vdbhip import _ffi

    D, I = np.zeros((NQ, K), F32), np.zeros((NQ, K), np.int64)
    extra = {"vdb_lsh_search": (K, NCAND), "vdb_knng_search": (K, EF)}.get(s.search, (K,))
    rc = getattr(lib, s.search)(h, _ffi.ptr(c.Q), NQ, *extra, _ffi.ptr(D), _ffi.ptr(I))
    if rc != _ffi.VDB_OK:
        raise RuntimeError(f"{s.search} of the state returned {rc}: {_ffi.last_error()}")
    return D.tobytes() + I.tobytes()


def run_state(vdb, state, report=None):
    """{entry: rc} of every entry on a handle of `state`.  `report` (a dict) also receives `no_message`, the refused entries that
    left vdb_last_error empty or stale, and `changed`, the refused entries after which the state's own search differed."""
    import torch
    from vdbhip import _ffi

    lib = _ffi.load()
    s = STATES[state]
    c = ctx(s.d, s.n, s.byte_valued)
    cells, no_message, changed = {}, [], []
    h = build(lib, s, c)
    try:
        want = own_search(lib, s, c, h) if s.search else None
        for name, fn, args in entries(c):
            lib.vdb_device_count(None)                           # leaves SENTINEL in vdb_last_error
            rc = getattr(lib, fn)(h, *args)
            torch.cuda.synchronize()
            cells[name] = rc
            if rc == _ffi.VDB_OK:                                # the handle may be another one now
                lib.vdb_destroy(h)
                h = None
                h = build(lib, s, c)
                continue
            if _ffi.last_error() in ("", SENTINEL):
                no_message.append(name)
            if want is not None and own_search(lib, s, c, h) != want:
                changed.append(name)
    finally:
        if h is not None:
            lib.vdb_destroy(h)
    if report is not None:
        report.update(no_message=no_message, changed=changed)
    return cells

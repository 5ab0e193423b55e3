"""vdb_set_option: which values every option accepts, which kinds of index refuse which options, what a multi-device
handle forwards, and the polarity of the four options the library reads as "not off" (panel_dtype, small_batch,
fused_stats, scan_pair).

The table below restates the ranges of include/vdbhip.h; it is this file's own, not read from the library.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# option -> (accepted values, default): a value outside the list is VDB_ERR_INVALID, a non-integer too
ONE_OF = {
    "lsh_force_fallback": ((0, 1), 0),
    "graph": ((0, 1), 0),
    "force_path": ((0, 1, 2, 3), 0),
    "stream_panels": ((0, 1), 0),
    "fused_stats": ((0, 1), 1),
    "panel_dtype": ((0, 1), 0),
    "ivf_bt": ((0, 4, 16), 0),
    "ivf_tps": ((0, 16, 64), 0),
    "ivf_tile": ((0, 1, 2), 0),
    "ivf_i8_group": ((4, 8), 4),
    "ivf_group": ((0, 1, 2, 4), 0),
    "ivf_nw": ((0, 2, 4, 8), 0),
    "small_batch": ((0, 1), 1),
    "i8_group": ((4, 8), 8),
    "flat_shape": ((0, 16, 32), 0),
    "i8_shape": ((0, 16, 32), 0),          # alias of flat_shape
    "int8_only": ((0, 1), 0),
    "f16_group": ((4, 8), 8),
    "i8_nt": ((0, 1, 2), 0),
    "i8_ring": ((0, 2, 4, 8), 0),
    "f16_wide": ((0, 1), 0),
    "f16_stage_tiles": ((0, 4, 8), 0),
    "scan_pair": ((0, 1), 1),
}
# option -> (lo, hi, default): lo <= value <= hi (hi None: no upper bound); non-integers inside are accepted (truncated)
RANGE = {
    "pq_slab_chunks": (0, 4096, 0),
    "pq_scan_min_batch": (0, 10 ** 9, 0),
    "stream_slab_rows": (0, None, 0),
    "upload_block_mb": (0, 4096, 0),
    "ivf_part": (0, 1024, 0),
    "ivf_min_batch": (1, 10 ** 9, 1),
    "int8_block_rows": (0, 2 ** 31 - 1, 0),
    "int8_slab_chunks": (0, 1024, 0),
    "i8_variant": (0, 7, 3),
    "kloop_qgroup": (0, 1024, 0),
    "scan_prio": (0, 2, 0),
    "spans_per_chunk": (0, 4096, 0),
    "select_variant": (0, 2, 0),
    "list_cap": (0, 65536, 0),
}
ANY = ("timing", "graph_recapture_at_once")      # every value is accepted (stored as value != 0)


def _refused(idx, name, value):
    with pytest.raises(ValueError, match="flat_shape|i8_shape" if name == "i8_shape" else name):     # (the text names the option)
        idx.set_option(name, value)


@pytest.fixture(scope="module")
def empty_flat(vdb):
    idx = vdb.FlatIndex(16, "l2")
    yield idx
    idx.close()


@pytest.mark.parametrize("name", sorted(ONE_OF))
def test_list_option_accepts_its_values_only(empty_flat, name):
    values, default = ONE_OF[name]
    try:
        for v in values:
            empty_flat.set_option(name, v)
        outside = sorted({v + s for v in values for s in (-1, 1)} - set(values))
        assert outside[0] == min(values) - 1 and outside[-1] == max(values) + 1
        for v in outside:
            _refused(empty_flat, name, v)
        _refused(empty_flat, name, min(values) + 0.5)
    finally:
        empty_flat.set_option(name, default)


@pytest.mark.parametrize("name", sorted(RANGE))
def test_range_option_accepts_its_range_only(empty_flat, name):
    lo, hi, default = RANGE[name]
    try:
        for v in (lo, lo + 1, lo + 0.5, 2 ** 40 if hi is None else hi):
            empty_flat.set_option(name, v)
        _refused(empty_flat, name, lo - 1)
        if hi is not None:
            _refused(empty_flat, name, hi + 1)
    finally:
        empty_flat.set_option(name, default)


def test_examples_of_the_issue_and_unknown_names(empty_flat):
    _refused(empty_flat, "ivf_bt", 8)
    _refused(empty_flat, "i8_variant", 8)
    _refused(empty_flat, "i8_variant", -1)
    _refused(empty_flat, "ivf_min_batch", 0)
    _refused(empty_flat, "ivf_bt", 0.5)              # a list option: integers only
    empty_flat.set_option("scan_prio", 0.5)          # a range option: truncated toward zero
    empty_flat.set_option("scan_prio", 0)
    for name in ANY:
        for v in (1, -3, 0.5, 1e12, 0):
            empty_flat.set_option(name, v)
    for v in (0, 1):
        with pytest.raises(ValueError, match="unknown option 'no_such_option'"):
            empty_flat.set_option("no_such_option", v)
        with pytest.raises(ValueError, match="unknown option 'multi_stage_all'"):      # a key of multi-device handles only
            empty_flat.set_option("multi_stage_all", v)


def _gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _refuses(idx, vdb, refused, accepted, match):
    """`refused`: (option, value) pairs that are VDB_ERR_UNSUPPORTED on this index; `accepted`: pairs that are not."""
    from vdbhip import _ffi

    for name, v in refused:
        with pytest.raises(_ffi.VdbError, match=match) as e:
            idx.set_option(name, v)
        assert name in str(e.value) and not isinstance(e.value, ValueError)
    for name, v in accepted:
        idx.set_option(name, v)


def test_sq8_index_refuses(vdb):
    X = _gauss(300, 16, 1)
    idx = vdb.IVFSQ8Index(16, 4, "l2", 0)
    idx.set_centroids(X[:4].copy())
    idx.train_ranges(X)
    idx.add(X)
    names = ("graph", "int8_only", "stream_panels")
    _refuses(idx, vdb, [(n, 1) for n in names], [(n, 0) for n in names], "SQ8")
    _refused(idx, "ivf_bt", 8)                       # every other option as on any index
    idx.close()


def test_lsh_index_refuses(vdb):
    idx = vdb.FlatIndex(16, "l2", 0)
    idx.lsh_set_projection(vdb.make_projection(16, 32, 0))
    names = ("int8_only", "stream_panels")
    _refuses(idx, vdb, [(n, 1) for n in names], [(n, 0) for n in names] + [("graph", 1), ("graph", 0)], "sign-LSH")
    idx.close()


def test_pq_index_refuses(vdb):
    idx = vdb.PQIndex(16, 4, "l2", 0)
    idx.set_codebooks(_gauss(4 * 256, 4, 2).reshape(4, 256, 4))
    idx.add(_gauss(300, 16, 3))
    names = ("graph", "int8_only", "stream_panels")
    _refuses(idx, vdb, [(n, 1) for n in names], [(n, 0) for n in names], "PQ index")
    _refuses(idx, vdb, [("flat_shape", 32), ("i8_shape", 32), ("f16_group", 4), ("i8_group", 4)],
             [("flat_shape", 0), ("flat_shape", 16), ("i8_shape", 0), ("i8_shape", 16), ("f16_group", 8), ("i8_group", 8)], "x16")
    _refused(idx, "flat_shape", 8)
    _refused(idx, "f16_group", 0)
    idx.close()


def test_multi_handle_forwards(vdb):
    X, Q = _gauss(40000, 16, 4), _gauss(256, 16, 5)
    m = vdb.FlatIndex(16, "l2", [0, 0])
    m.add(X)
    m.search(Q, 3)
    assert m.stats()["last_path_name"] == "mfma_scan"
    m.set_option("force_path", 1)                    # forwarded to every shard
    m.search(Q, 3)
    assert m.stats()["last_path_name"] == "exact_scan"
    _refused(m, "ivf_bt", 8)                         # ... with the shards' checks
    with pytest.raises(RuntimeError, match="multi-device"):
        m.set_option("graph", 1)
    m.set_option("graph", 0)
    m.set_option("multi_stage_all", 1)
    m.set_option("multi_stage_all", 0)
    m.close()


@pytest.fixture(scope="module")
def byte_index(vdb):
    """A byte-valued corpus just above the rows of the dense path (15 360): layout "x16", an int8 copy next to the fp16 one.
    8 queries are too few for the scan to be chosen (search_batch), so it is forced; the scan is what these options shape."""
    rng = np.random.default_rng(6)
    X = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(20000, 32))), 0, 255).astype(np.float32)
    Q = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(8, 32))), 0, 255).astype(np.float32)
    idx = vdb.FlatIndex(32, "l2", 0)
    idx.add(X)
    idx.set_option("force_path", 2)
    yield idx, Q
    idx.close()


def test_panel_dtype_polarity(byte_index):
    idx, Q = byte_index
    got = {}
    for v, dtype in ((0, 1), (1, 0), (0, 1)):
        idx.set_option("panel_dtype", v)
        D, I = idx.search(Q, 10)
        st = idx.stats()
        print("panel_dtype", v, st["last_path_name"], st["scan_dtype"], st["scan_shape"], st["has_i8_copy"])
        assert st["last_path_name"] == "mfma_scan" and st["has_i8_copy"] == 1
        assert st["scan_dtype"] == dtype, (v, st)
        got[v] = I
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("name", ["small_batch", "fused_stats", "scan_pair"])
def test_same_results_at_0_and_1(byte_index, name):
    idx, Q = byte_index
    out = []
    try:
        for v in (1, 0):
            idx.set_option(name, v)
            D, I = idx.search(Q, 10)
            assert idx.stats()["last_path_name"] == "mfma_scan"
            out.append((D, I))
    finally:
        idx.set_option(name, 1)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])

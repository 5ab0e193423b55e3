"""One long-lived handle under interleaved calls of every kind: seeded random sequences and short directed ones, each step
compared byte for byte with what the host model of tests/sequence_cases.py expects -- the references are the ones the per-feature tests
use (oracle.knn / ivf_search / pair_keys, range_cases, filter_cases, ivf_filter_cases, ivf_range_cases).  The per-feature files test a
feature on a fresh handle; these test what a handle remembers between calls: the range result and its buffers, the installed filter,
the coarse search's query statistics, who clears the small workspace arrays, the workspace sized to the largest batch so far.

tests/test_sequence_host.py proves on fake indexes that the driver, the model and the committed seeds detect stale state.  With
VDBHIP_SEQUENCE_TRACE naming a file, the driver appends every step's line to it before the step runs."""
from __future__ import annotations

import ctypes
from dataclasses import replace

import numpy as np
import pytest

from tests import sequence_cases as sc
from tests.sequence_cases import Step as S

pytestmark = pytest.mark.gpu

CASES = [(kind, shape.name, seed) for kind in ("flat", "ivf") for shape, seed in sc.committed(kind)]
FLAT, FLAT_I8, IVF, IVF_I8 = (sc.shape_of("flat", "x16-f16"), sc.shape_of("flat", "x16-i8"), sc.shape_of("ivf", "f16-d64"),
                              sc.shape_of("ivf", "i8-d64-int"))
BOTH = [(FLAT, "l2"), (FLAT, "ip"), (IVF, "l2"), (IVF, "ip")]
BOTH_IDS = [f"{s.kind}-{m}" for s, m in BOTH]


def _fill(shape, id_base=0):
    """the steps that bring a fresh handle to all rows of the shape"""
    return [S("add", (id_base,))] + [S("append")] * (len(shape.blocks) - 1)


def _run(vdb, oracle, shape, metric, steps, label, each=None):
    """run `steps` on a fresh handle; `each(index, model, i, step)` after every step"""
    index = sc.open_index(vdb, shape, metric)
    try:
        model = sc.model_for(shape, metric, oracle)
        if each is None:
            sc.run(index, steps, model, label=f"{label} {shape.name} {metric}")
        else:
            for i, step in enumerate(steps):
                sc.run(index, [step], model, label=f"{label} {shape.name} {metric}", first=i)
                each(index, model, i, step)
    finally:
        index.close()


# ---- random sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name,seed", CASES, ids=[f"{k}-{n}-s{s}" for k, n, s in CASES])
def test_random_sequence(kind, name, seed, vdb, oracle):
    shape = sc.shape_of(kind, name)
    metric = sc.metric_of(shape, seed)
    index = sc.open_index(vdb, shape, metric)
    try:
        sc.run(index, sc.sequence(kind, name, seed), sc.model_for(shape, metric, oracle), label=f"{kind} {name} seed {seed} {metric}")
    finally:
        index.close()


# ---- directed sequences: one piece of cached state each -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,metric", BOTH, ids=BOTH_IDS)
def test_regrow_under_filter(shape, metric, vdb, oracle):
    """the Workspace buffers grow under an installed filter: the masked copies and the list must not depend on the old sizes"""
    steps = _fill(shape) + [S("set_filter", ("random-0.5", "bool")), S("search_filtered", (5, 10, 0)), S("search", (130, 10, 0)),
                            S("search_filtered", (130, 10, 1)), S("search_filtered", (5, 10, 1)),
                            S("set_filter", ("hundred", "ids")), S("search_filtered", (5, 10, 0)),
                            S("reserve", (130, 100)) if shape.kind == "flat" else S("search", (130, 100, 0)),
                            S("search_filtered", (130, 100, 0))]
    _run(vdb, oracle, shape, metric, steps, "regrow-under-filter")


@pytest.mark.parametrize("shape,metric", [(IVF, "l2"), (IVF, "ip"), (IVF_I8, "l2")], ids=["f16-l2", "f16-ip", "i8-l2"])
def test_same_size_new_queries(shape, metric, vdb, oracle):
    """info_valid_nq: the coarse search's query statistics are taken over on a match of the batch size alone -- every order of the three
    calls that run a coarse search, each followed by the same calls with other queries of the same count"""
    import itertools

    calls = {"search": lambda q: S("search", (64, 10, q)), "range": lambda q: S("range_search", (64, "10", q)),
             "filtered": lambda q: S("search_filtered", (64, 10, q))}
    steps = _fill(shape) + [S("set_nprobe", (8,)), S("set_filter", ("random-0.5", "bool"))]
    for order in itertools.permutations(calls):
        for qset in (0, 1):
            steps += [calls[c](qset) for c in order]
    _run(vdb, oracle, shape, metric, steps, "same-size-new-queries")


@pytest.mark.parametrize("shape,metric", BOTH, ids=BOTH_IDS)
def test_range_result_survives(shape, metric, vdb, oracle):
    """range_valid / RangeBufs: unrelated calls leave the last result alone, an option change drops it"""
    flat = shape.kind == "flat"
    steps = _fill(shape) + [S("range_search", (17, "10", 0)), S("search", (64, 10, 1)), S("set_filter", ("random-0.1", "words")),
                            S("search_filtered", (130, 10, 0))]
    steps += [S("rerank", (16, 40, 10, 0)), S("reserve", (64, 10))] if flat else [S("set_nprobe", (16,)), S("search", (16, 100, 0))]
    steps += [S("range_results_again"), S("filter_count"), S("set_option", ("timing", 1.0)), S("range_results_again"), S("filter_count"),
              S("search_filtered", (5, 10, 0))]
    _run(vdb, oracle, shape, metric, steps, "range-result-survives")


@pytest.mark.parametrize("shape,metric", BOTH, ids=BOTH_IDS)
def test_range_buffers_shrink_and_grow(shape, metric, vdb, oracle):
    """RangeBufs grow per slab: a large result, a tiny one, several slabs ("range_bitmap_mb" 1), a large one again"""
    steps = _fill(shape) + ([S("set_nprobe", (16,))] if shape.kind == "ivf" else [])
    steps += [S("range_search", (130, "half", 0)), S("range_results_again"), S("range_search", (130, "0", 1)), S("range_results_again"),
              S("set_option", ("range_bitmap_mb", 1.0)), S("range_search_device", (130, "half", 1)), S("range_results_again"),
              S("range_search", (17, "10", 0)), S("range_results_again"), S("range_search", (130, "half", 0)), S("range_results_again")]
    _run(vdb, oracle, shape, metric, steps, "range-buffers-shrink-and-grow")


@pytest.mark.parametrize("shape,metric", BOTH, ids=BOTH_IDS)
def test_replacing_install(shape, metric, vdb, oracle):
    """filter_has_list and the buffers a replacing install reuses: dense, a hundred rows (the sparse list appears), dense (it goes)"""
    steps = _fill(shape)
    last = "alternating" if shape.kind == "flat" else "id-run"
    for install in (S("set_filter", ("random-0.5", "bool")), S("set_filter", ("hundred", "ids")), S("set_filter_device", ("random-0.1",)),
                    S("set_filter", ("all-zeros", "bool")), S("set_filter", (last, "words"))):
        steps += [install, S("filter_count"), S("search_filtered", (5, 10, 0)), S("search_filtered", (64, 100, 1))]
    _run(vdb, oracle, shape, metric, steps, "replacing-install")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_append_crosses_a_route(metric, vdb, oracle):
    """12 000 rows sit below the x16 layout's 15 360, 20 421 above: the append re-derives the scan copies in another layout, the
    filter of the old rows is gone, and a new one covers the appended rows"""
    shape = sc.Shape("flat", "cross-12000+8421", 20421, 32, (12000, 20421))
    steps = [S("add", (1_000_003,)), S("set_filter", ("random-0.5", "bool")), S("search_filtered", (64, 10, 0)), S("append"),
             S("search_filtered", (64, 10, 0)), S("filter_count"), S("set_filter", ("last-span-only", "ids")), S("search_filtered", (64, 10, 0)),
             S("set_filter", ("random-0.5", "words")), S("search_filtered", (64, 10, 1)), S("search", (64, 10, 1))]
    _run(vdb, oracle, shape, metric, steps, "append-crosses-a-route")


@pytest.mark.parametrize("shape,metric", BOTH, ids=BOTH_IDS)
def test_refused_calls_change_nothing(shape, metric, vdb, oracle):
    """include/vdbhip.h: a refused add -- flat or IVF -- and a refused install change nothing: rows, filter, range result"""
    probes = [S("search", (16, 10, 0)), S("search_filtered", (16, 10, 0)), S("filter_count"), S("range_results_again")]
    refusals = [S("add_refused"), S("set_filter_refused")] if shape.kind == "flat" else \
        [S("add_refused", ("id_base",)), S("add_refused", ("list",)), S("set_filter_refused")]
    steps = _fill(shape, 1_000_003) + [S("set_filter", ("random-0.1", "bool")), S("range_search", (16, "10", 0))] + probes
    for r in refusals:
        steps += [r] + probes
    _run(vdb, oracle, shape, metric, steps, "refused-calls-change-nothing")


def test_refused_flat_adds_keep_the_filter_and_the_range_result(vdb, oracle):
    """the refusals of vdb_add that the step vocabulary has no name for: a null pointer with n > 0, a negative n, and an append to an
    "int8_only" index -- each leaves the filter, the range result and the rows as they were"""
    from vdbhip import _ffi

    lib = _ffi.load()
    rng = np.random.default_rng(97)
    X = np.clip(np.rint(rng.gamma(0.6, 40.0, size=(33000, 32))), 0, 255).astype(np.float32)
    Q = X[:16] + 1
    for int8_only in (0, 1):
        index = vdb.FlatIndex(32, "l2", 0)
        try:
            index.set_option("int8_only", int8_only)
            index.add(X[:32900])
            index.set_filter(np.arange(0, 32900, 3))
            before = index.search_filtered(Q, 10) + index.range_search(Q, 4000.0)
            assert before[2][-1] > 0
            h = index._handle()
            refused = [lib.vdb_add(h, None, 5, 0), lib.vdb_add(h, _ffi.ptr(X), -1, 0), lib.vdb_add(h, _ffi.ptr(X), 5, 7)]
            want = [_ffi.VDB_ERR_INVALID] * 3
            if int8_only:
                refused.append(lib.vdb_add(h, _ffi.ptr(X), 5, 0))
                want.append(_ffi.VDB_ERR_UNSUPPORTED)
                assert "ONE add" in _ffi.last_error()
            assert refused == want, (refused, want)
            assert index.stats()["ntotal"] == 32900 and index.filter_count == 10967
            D, I = np.empty_like(before[3]), np.empty_like(before[4])
            assert lib.vdb_range_results(h, _ffi.ptr(D), _ffi.ptr(I)) == _ffi.VDB_OK, _ffi.last_error()
            after = index.search_filtered(Q, 10) + (before[2], D, I)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
            # an empty append is an add that passed its checks: it drops both
            assert lib.vdb_add(h, _ffi.ptr(X), 0, 0) == _ffi.VDB_OK
            n = ctypes.c_int64(0)
            assert lib.vdb_filter_count(h, ctypes.byref(n)) == _ffi.VDB_ERR_STATE and "no filter" in _ffi.last_error()
            assert lib.vdb_range_results(h, _ffi.ptr(D), _ffi.ptr(I)) == _ffi.VDB_ERR_STATE and "no range result" in _ffi.last_error()
        finally:
            index.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivf_to_flat_and_back(metric, vdb, oracle):
    """ivf_built and the rows of a vdb_add on an IVF handle: vdb_search answers over them, the IVF calls say "not built", the next
    vdb_ivf_add replaces them"""
    steps = [S("add", (0,)), S("set_filter", ("random-0.5", "bool")), S("range_search", (16, "10", 0)), S("search", (64, 10, 0)),
             S("flat_search", (16, 10, 0)), S("flat_add", (1_000_003,)), S("flat_search", (64, 10, 0)), S("search", (64, 10, 0)),
             S("search_filtered", (16, 10, 0)), S("filter_count"), S("range_results_again"), S("set_centroids"), S("flat_search", (64, 10, 1)),
             S("add_assigned", (0,)), S("flat_search", (16, 10, 0)), S("search", (64, 10, 1)), S("search_filtered", (64, 10, 1)),
             S("set_filter", ("one-list-only", "ids")), S("search_filtered", (64, 10, 1)), S("append"), S("search", (64, 10, 0))]
    _run(vdb, oracle, IVF, metric, steps, "ivf-to-flat-and-back")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_kind_change_drops_the_filter(metric, vdb, oracle):
    """filter_kind: the handle becomes an LSH index under an installed filter; the range result is materialised and stays"""
    steps = _fill(FLAT) + [S("set_filter", ("random-0.1", "bool")), S("range_search", (16, "10", 0)), S("search_filtered", (16, 10, 0)),
                           S("become_lsh"), S("search_filtered", (16, 10, 0)), S("filter_count"), S("range_results_again"),
                           S("set_filter", ("random-0.1", "ids")), S("search_filtered", (16, 10, 0)), S("search", (16, 10, 0))]
    _run(vdb, oracle, FLAT, metric, steps, "kind-change-drops-the-filter")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_integer_then_float_batches(metric, vdb, oracle):
    """has_bias / has_bias8 of an install on a byte-valued index: an integer batch scans the int8 copy, the next batch the fp16 one,
    under one installed filter; vdb_stats.scan_dtype says which scan served, as filter_cases.Route records it"""
    steps = _fill(FLAT_I8) + [S("set_option", ("filter_sparse_pairs", 0.0)), S("set_filter", ("random-0.5", "words"))]
    for _ in range(3):
        steps += [S("search_filtered", (64, 10, 0)), S("search_filtered", (64, 10, 1)), S("search", (64, 10, 0)), S("search", (64, 10, 1))]
    steps += [S("search_filtered", (5, 100, 0)), S("search_filtered", (5, 100, 1))]
    seen = []

    def each(index, model, i, step):
        if step.op in ("search", "search_filtered"):
            st = index.stats()
            seen.append((step.op, step.args[0], step.args[-1], st["last_path_name"], st["scan_dtype"]))

    _run(vdb, oracle, FLAT_I8, metric, steps, "integer-then-float-batches", each)
    for op, nq, qset, path, dtype in seen:
        if nq == 64:
            assert (path, dtype) == ("mfma_scan", 1 - qset), seen      # (batch A holds integers, batch B does not)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_integer_then_float_batches_ivf(metric, vdb, oracle):
    """the same alternation through the list scans of an IVF-Flat index of byte-valued rows"""
    shape = replace(IVF_I8, name="i8-d64-mixed", qkinds=("int", "float"))
    steps = _fill(shape) + [S("set_nprobe", (8,)), S("set_filter", ("random-0.5", "bool"))]
    for _ in range(2):
        steps += [S("search_filtered", (130, 10, 0)), S("search_filtered", (130, 10, 1)), S("search", (130, 10, 0)), S("range_search", (130, "10", 1)),
                  S("search", (130, 10, 1))]
    _run(vdb, oracle, shape, metric, steps, "integer-then-float-batches-ivf")

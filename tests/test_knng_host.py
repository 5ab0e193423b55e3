"""k-NN graph, host side (no GPU): the NumPy restatement against itself (the forgetting proof, the prune, the step cap), the
C-ABI surface and the plugin classes' parameter mapping."""
from __future__ import annotations

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import knng_restatement as ref  # noqa: E402

KNNG_ENTRY_POINTS = {"vdb_knng_build", "vdb_knng_set", "vdb_knng_get", "vdb_knng_search", "vdb_knng_search_device"}


def path_graph(n: int, degree: int = 4) -> np.ndarray:
    g = np.full((n, degree), -1, np.int32)
    for i in range(n):
        nb = [j for j in (i - 1, i + 1) if 0 <= j < n]
        g[i, :len(nb)] = nb
    return g


def random_graph(rng, n: int, degree: int) -> np.ndarray:
    g = np.full((n, degree), -1, np.int32)
    for i in range(n):
        m = int(rng.integers(0, degree + 1))
        others = np.delete(np.arange(n), i)
        pick = rng.choice(others, size=min(m, n - 1), replace=False)
        g[i, :pick.size] = pick
    return g


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_forgetting_everything_but_the_list_changes_no_result(oracle, metric):
    """The visited structure is a cache: re-scoring every neighbour that is not in L returns what an exact visited set returns --
    on the pruned graph of a random corpus, on random digraphs, on integer data full of exact ties, at beams from 1 up."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((600, 12)).astype(np.float32)
    Q = rng.standard_normal((40, 12)).astype(np.float32)
    graphs = [ref.build(X, 8, 16, metric), random_graph(rng, 600, 6), random_graph(rng, 600, 24)]
    for g in graphs:
        for k, ef, nentry, cap in [(1, 1, 1, None), (5, 5, 32, None), (10, 40, 7, None), (10, 40, 32, 9), (20, 100, 600, None)]:
            a = ref.search(X, g, Q, k, ef, metric, nentry=nentry, max_iters=cap)
            b = ref.search(X, g, Q, k, ef, metric, nentry=nentry, max_iters=cap, forget=True)
            assert same(a, b), (k, ef, nentry, cap)
            assert (b[2] >= a[2]).all()                    # forgetting only ever scores more
    Xi = rng.integers(0, 4, size=(500, 8)).astype(np.float32)
    Qi = rng.integers(0, 4, size=(30, 8)).astype(np.float32)
    gi = ref.build(Xi, 8, 16, "l2")
    for k, ef in [(1, 1), (10, 10), (10, 64)]:
        a = ref.search(Xi, gi, Qi, k, ef, "l2")
        b = ref.search(Xi, gi, Qi, k, ef, "l2", forget=True)
        assert same(a, b)
        keys = oracle.pair_keys(Xi, Qi, np.where(a[1] >= 0, a[1], 0), "l2")
        order = keys * 1000 + a[1]
        assert (np.diff(order, axis=1)[a[1][:, 1:] >= 0] > 0).all()      # ties within a result are in id order


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_prune_with_ncand_equal_to_degree_permutes_the_candidates(oracle, metric):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 6)).astype(np.float32)
    cand, ckeys = ref.candidates(X, 12, metric)
    assert (cand != np.arange(300)[:, None]).all() and (np.diff(ref.sortable(ckeys).astype(np.float64), axis=1) >= 0).all()
    _, exact = oracle.knn(X, X, 13, metric)
    for i in range(300):
        assert cand[i].tolist() == [v for v in exact[i].tolist() if v != i][:12]
    g = ref.prune(X, cand, ckeys, 12, metric)
    assert np.array_equal(np.sort(g, axis=1), np.sort(cand, axis=1))
    assert (g[:, 0] == cand[:, 0]).all()                   # the nearest candidate is always selected first
    assert not np.array_equal(g, cand)                     # ... and somewhere the heuristic moved a rejected candidate back
    wide = ref.build(X, 6, 12, metric)
    assert (wide[:, 0] == cand[:, 0]).all() and all(set(wide[i]) <= set(cand[i]) for i in range(300))
    # fewer rows than candidates: everything but the row itself, then -1
    small = ref.build(X[:3], 4, 8, metric)
    assert small.shape == (3, 4) and (small[:, 2:] == -1).all() and sorted(small[0, :2].tolist()) == [1, 2]
    assert ref.build(X[:1], 4, 4, metric).tolist() == [[-1, -1, -1, -1]]


def test_duplicate_rows_push_a_row_out_of_its_own_candidates(oracle):
    X = np.zeros((10, 3), np.float32)
    X[7:] = np.arange(9, dtype=np.float32).reshape(3, 3) + 1
    cand, _ = ref.candidates(X, 4)                          # rows 0..6 are identical: 5 nearest of row 6 are rows 0..4
    assert cand[6].tolist() == [0, 1, 2, 3] and cand[0].tolist() == [1, 2, 3, 4] and cand[2].tolist() == [0, 1, 3, 4]


def test_step_cap_on_a_path(oracle):
    """Rows on a line, entry at row 0, the query at the far end: every step expands one more row of the path."""
    n = 40
    X = np.zeros((n, 2), np.float32)
    X[:, 0] = np.arange(n)
    Q = np.array([[n - 1, 0]], np.float32)
    g = path_graph(n)
    D, I, scored, capped = ref.search(X, g, Q, 3, 8, nentry=1, max_iters=5)
    assert capped.all() and scored[0] == 6 and I[0].tolist() == [5, 4, 3]
    assert D[0].tolist() == [float((n - 1 - i) ** 2) for i in (5, 4, 3)]
    D, I, scored, capped = ref.search(X, g, Q, 3, 8, nentry=1)
    assert not capped.any() and I[0].tolist() == [n - 1, n - 2, n - 3] and scored[0] == n
    # the cap counts only when it cut something off: 39 steps reach the end with row 39 still unexpanded, 40 finish
    assert ref.search(X, g, Q, 3, 8, nentry=1, max_iters=n - 1)[3].all()
    assert not ref.search(X, g, Q, 3, 8, nentry=1, max_iters=n)[3].any()
    # k above what was reached: padding
    D, I, _, _ = ref.search(X, g, Q, 5, 8, nentry=1, max_iters=2, id_base=100)
    assert I[0].tolist() == [102, 101, 100, -1, -1] and D[0, 3] == ref.FLT_MAX
    assert ref.entry_rows(10, 100, 4) == [0, 2, 5, 7] and ref.entry_rows(3, 100, 32) == [0] and ref.entry_rows(100, 2, 32) == [0, 3]


def test_header_and_ffi_carry_the_knng_entry_points():
    from vdbhip import _ffi

    header = (ROOT / "include" / "vdbhip.h").read_text()
    proto = dict(re.findall(r"^int (vdb_knng_[a-z_]+)\(([^;]*)\);", header, re.M))
    assert set(proto) == KNNG_ENTRY_POINTS and KNNG_ENTRY_POINTS <= set(_ffi.SIGNATURES)
    for name, args in proto.items():
        assert len(_ffi.SIGNATURES[name][1]) == len(args.split(",")), name
    assert "VDB_PATH_KNNG = 5" in header and _ffi.PATH_NAMES[5] == "knng" and "#define VDB_ABI_VERSION 4" in header
    for option in ("knng_nentry", "knng_max_iters", "knng_visited_bits", "knng_build_block"):
        assert f'"{option}"' in header
    lib = _ffi.load()
    for name in KNNG_ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.vdb_abi_version() == 4
    assert lib.vdb_knng_build(None, 32, 64) == _ffi.VDB_ERR_INVALID                     # null handle: no GPU touched
    assert "null handle" in _ffi.last_error()
    assert lib.vdb_knng_search(None, None, 0, 1, 1, None, None) == _ffi.VDB_ERR_INVALID


def test_plugin_classes_map_the_hnsw_parameters_without_a_gpu():
    import vdbhip
    from vdbhip import HipKnnGraphIndexer, HipKnnGraphSearch, HipKnnGraphSearcher
    from vdbhip.knng import graph_parameters

    assert graph_parameters(16) == (32, 64) and graph_parameters(32) == (64, 128) and graph_parameters(8, 100) == (16, 100)
    assert graph_parameters(2) == (4, 8)
    for bad in (1, 33, 0):
        with pytest.raises(ValueError, match="M must be"):
            graph_parameters(bad)
    for bad in (31, 129):
        with pytest.raises(ValueError, match="ncand must be"):
            graph_parameters(16, bad)
    ix = HipKnnGraphIndexer("g", 64)
    assert (ix.M, ix.degree, ix.ncand, ix.efSearch, ix.efConstruction, ix.metric) == (16, 32, 64, 100, 200, "l2")
    assert ix.describe()["params"]["efConstruction"] == 200
    assert "unused" in HipKnnGraphIndexer.__doc__.lower()
    with pytest.raises(ValueError, match="supports metrics"):
        HipKnnGraphIndexer("g", 64, metric="hamming")
    with pytest.raises(ValueError, match="efSearch"):
        HipKnnGraphIndexer("g", 64, efSearch=513)
    with pytest.raises(ValueError, match="Expected dimension 64, got 32"):
        ix.build(np.zeros((4, 32), np.float32))
    se = HipKnnGraphSearcher("s", 64, efSearch=50)
    with pytest.raises(RuntimeError, match="not attached"):
        se.batch_search(np.zeros((1, 64), np.float32), 5)
    with pytest.raises(ValueError, match="hip_knng"):
        se.attach(vdbhip.IndexArtifact(kind="hip_ivf", data=None), np.zeros((1, 64), np.float32))
    alone = HipKnnGraphSearch("hnsw", 64, M=8, efConstruction=100, efSearch=64, metric="cosine")
    assert (alone.degree, alone.ncand) == (16, 32)
    assert alone.get_parameters() == {"M": 8, "efConstruction": 100, "efSearch": 64, "metric": "cosine"}
    with pytest.raises(RuntimeError, match="Index not built"):
        alone.batch_search(np.zeros((1, 64), np.float32), 5)
    assert vdbhip.get_indexer_class("HipKnnGraphIndexer") is HipKnnGraphIndexer
    assert vdbhip.get_searcher_class("HipKnnGraphSearcher") is HipKnnGraphSearcher
    assert isinstance(vdbhip.get_algorithm_instance("HipKnnGraphSearch", 64, name="hnsw", M=16), HipKnnGraphSearch)
    algo = vdbhip.get_algorithm_instance(                       # the hnsw row of the reference's configs
        "Composite", 64, name="hnsw", metric="l2",
        indexer={"type": "HipKnnGraphIndexer", "M": 16, "efConstruction": 200, "efSearch": 100},
        searcher={"type": "HipKnnGraphSearcher"})
    assert isinstance(algo.indexer, HipKnnGraphIndexer) and isinstance(algo.searcher, HipKnnGraphSearcher)
    # the older classes keep refusing what they refuse: a graph artifact is not theirs
    with pytest.raises(ValueError, match="hip_ivf"):
        vdbhip.HipIVFSearcher("s", 64).attach(vdbhip.IndexArtifact(kind="hip_knng", data=None), np.zeros((1, 64), np.float32))

"""PQ<M>, host side (no GPU): key parsing, the C-ABI surface, the plugin classes' parameter checks, the registry entries and
the NumPy restatement of the code contract against a brute-force loop."""
from __future__ import annotations

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import pq_restatement as ref  # noqa: E402

PQ_ENTRY_POINTS = {"vdb_pq_train", "vdb_pq_set_codebooks", "vdb_pq_get_codebooks", "vdb_pq_add", "vdb_pq_add_codes",
                   "vdb_pq_get_codes"}


def test_parse_pq_key():
    from vdbhip import parse_pq_key

    assert parse_pq_key("PQ64") == 64 and parse_pq_key("PQ50") == 50 and parse_pq_key("PQ64x8") == 64
    assert parse_pq_key(" PQ8 ") == 8
    for bad in ("PQ64x4", "PQ64x16", "PQ", "PQ0", "pq64", "IVF100,PQ8", "OPQ16,PQ16", "PQ64,Flat", "IVF100,Flat", "PQ-4", "PQ8x", ""):
        with pytest.raises(ValueError):
            parse_pq_key(bad)


def test_the_ivf_parsers_and_classes_still_refuse_pq_keys():
    from vdbhip import HipApproximateSearch, HipIVFIndexer, parse_index_key
    from vdbhip.ivf import parse_ivf_key

    for key in ("PQ64", "PQ64x8", "IVF100,PQ8", "IVF1024,PQ16x8"):
        with pytest.raises(ValueError):
            parse_index_key(key)
        with pytest.raises(ValueError):
            parse_ivf_key(key)
        with pytest.raises(ValueError):
            HipApproximateSearch("a", 64, key)
        with pytest.raises(ValueError):
            HipIVFIndexer("i", 64, index_key=key)


def test_header_and_ffi_carry_the_pq_entry_points():
    from vdbhip import _ffi

    header = (ROOT / "include" / "vdbhip.h").read_text()
    declared = set(re.findall(r"^int (vdb_pq_[a-z_]+)\(", header, re.M))
    assert declared == PQ_ENTRY_POINTS
    assert PQ_ENTRY_POINTS <= set(_ffi.SIGNATURES)
    assert "#define VDB_ABI_VERSION 4" in header
    lib = _ffi.load()
    for name in PQ_ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.vdb_abi_version() == 4
    assert lib.vdb_pq_set_codebooks(None, 8, None) == _ffi.VDB_ERR_INVALID             # null handle: no GPU touched
    assert lib.vdb_pq_add(None, None, 0, 0) == _ffi.VDB_ERR_INVALID


def test_plugin_classes_validate_without_a_gpu():
    import vdbhip
    from vdbhip import HipPQIndexer, HipPQSearch, HipPQSearcher, PQIndex

    ix = HipPQIndexer("pq", 64, index_key="PQ64", seed=7)
    assert ix.index_key == "PQ64" and ix.metric == "l2" and ix.params["seed"] == 7
    assert HipPQIndexer("pq", 50, metric="cosine", index_key="PQ50").metric == "cosine"
    assert HipPQIndexer("pq", 384, metric="ip", index_type="PQ64x8").index_key == "PQ64x8"
    with pytest.raises(ValueError):
        HipPQIndexer("pq", 64, index_key="IVF100,Flat")
    with pytest.raises(ValueError, match="multiple of 48"):
        HipPQIndexer("pq", 64, index_key="PQ48")
    with pytest.raises(ValueError, match="Expected dimension 64, got 32"):
        ix.build(np.zeros((4, 32), np.float32))
    se = HipPQSearcher("s", 64)
    with pytest.raises(RuntimeError, match="not attached"):
        se.batch_search(np.zeros((1, 64), np.float32), 5)
    with pytest.raises(ValueError, match="hip_pq"):
        se.attach(vdbhip.IndexArtifact(kind="hip_ivf", data=None), np.zeros((1, 64), np.float32))
    algo = HipPQSearch("a", 64, index_type="PQ64")
    assert algo.metric == "l2" and HipPQSearch("a", 64, index_type="PQ8", metric="cosine").metric == "ip"
    with pytest.raises(RuntimeError, match="not been built"):
        algo.batch_search(np.zeros((1, 64), np.float32), 5)
    with pytest.raises(RuntimeError, match="before build_index"):
        algo.save_index("/nonexistent/dir")
    with pytest.raises(FileNotFoundError):
        algo.load_index("/nonexistent/dir")
    with pytest.raises(ValueError):
        HipPQSearch("a", 64, index_type="IVF100,PQ8")
    with pytest.raises(ValueError):
        HipPQSearch("a", 64, index_type="PQ7")
    # several devices: refused before any GPU call
    with pytest.raises(ValueError, match="one GPU"):
        PQIndex(64, 8, "l2", [0, 1])
    with pytest.raises(ValueError, match="one GPU"):
        HipPQSearch("a", 64, index_type="PQ8", device_ids=[0, 1])
    with pytest.raises(ValueError, match="metric"):
        PQIndex(64, 8, "cosine", 0)
    for dim, m in ((64, 0), (64, 7), (600, 300), (4, 8)):
        with pytest.raises(ValueError, match="M must divide"):
            PQIndex(dim, m, "l2", 0)


def test_registry_entries():
    import vdbhip
    from vdbhip import HipPQIndexer, HipPQSearch, HipPQSearcher

    assert vdbhip.get_indexer_class("HipPQIndexer") is HipPQIndexer
    assert vdbhip.get_searcher_class("HipPQSearcher") is HipPQSearcher
    assert vdbhip.ALGORITHM_REGISTRY["HipPQSearch"] is HipPQSearch
    assert isinstance(vdbhip.get_algorithm_instance("HipPQSearch", 64, index_type="PQ64"), HipPQSearch)
    algo = vdbhip.get_algorithm_instance(                       # the `pq` row of the reference's config
        "Composite", 64, name="pq", metric="l2",
        indexer={"type": "HipPQIndexer", "index_key": "PQ64"}, searcher={"type": "HipPQSearcher"})
    assert isinstance(algo.indexer, HipPQIndexer) and isinstance(algo.searcher, HipPQSearcher)
    for name in ("HipPQIndexer", "HipPQSearcher", "HipPQSearch", "PQIndex", "parse_pq_key"):
        assert name in vdbhip.__all__


def test_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(3)
    M, dsub = 3, 2
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    cb[1, 200] = cb[1, 17]                    # two equal centroids: the smaller index wins whenever they are nearest
    x = rng.standard_normal((40, M * dsub)).astype(np.float32)
    x[0, 2:4] = cb[1, 200]                    # a row that sits on the duplicated centroid
    x[1, 0:2] = cb[0, 99]                     # a row equal to a centroid
    x[2, 4:6] = (cb[2, 5].astype(np.float64) * 0.5 + cb[2, 6].astype(np.float64) * 0.5).astype(np.float32)
    codes = ref.encode(x, cb)
    assert codes.dtype == np.uint8 and codes.shape == (40, M)
    assert np.array_equal(codes, ref.encode_bruteforce(x, cb))
    assert codes[0, 1] == 17 and codes[1, 0] == 99
    xr = ref.reconstruct(codes, cb)
    assert xr.dtype == np.float32 and xr.shape == x.shape
    for i in (0, 7, 39):
        for m in range(M):
            assert np.array_equal(xr[i, m * dsub:(m + 1) * dsub], cb[m, codes[i, m]])
    # dsub = 1, integer centroids, rows exactly between two of them: the tie goes to the smaller c
    cb1 = np.arange(256, dtype=np.float32).reshape(1, 256, 1) * 2.0          # 0, 2, 4, ...
    x1 = np.array([[1.0], [3.0], [4.0], [509.0], [600.0], [-7.0]], np.float32)
    c1 = ref.encode(x1, cb1)
    assert c1[:, 0].tolist() == [0, 1, 2, 254, 255, 0]
    assert np.array_equal(c1, ref.encode_bruteforce(x1, cb1))
    # the fma emulation on values whose square is inexact in float64
    t = np.array([[1.0 + 2.0 ** -30, 3.000000000123, 1e-3 + 1e-12]], np.float64)
    acc = np.array([[0.1, 7.0, 1e-7]], np.float64)
    from fractions import Fraction
    want = [float(Fraction(float(a)) * Fraction(float(a)) + Fraction(float(b))) for a, b in zip(t[0], acc[0])]
    assert ref._fma_sq_add(t, acc)[0].tolist() == want

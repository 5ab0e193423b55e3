"""IVF<nlist>,PQ<M>, host side (no GPU): key parsing, the C-ABI surface, the plugin classes' parameter checks, the registry
entries, the NumPy restatement of the code contract against a brute-force loop, and the host condition of the near-tie case of
tests/test_gpu_ivf_pq.py."""
from __future__ import annotations

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import guard_cases as gc  # noqa: E402
import ivfpq_cases as cases  # noqa: E402
import ivfpq_restatement as ref  # noqa: E402

IVFPQ_ENTRY_POINTS = {"vdb_ivfpq_train", "vdb_ivfpq_set_codebooks", "vdb_ivfpq_get_codebooks", "vdb_ivfpq_add_codes",
                      "vdb_ivfpq_get_codes"}


def test_parse_ivfpq_key():
    from vdbhip import parse_ivfpq_key

    assert parse_ivfpq_key("IVF256,PQ64") == (256, 64) and parse_ivfpq_key("IVF256,PQ64x8") == (256, 64)
    assert parse_ivfpq_key("IVF256,PQ50") == (256, 50) and parse_ivfpq_key(" IVF8 , PQ4 ") == (8, 4)
    for bad in ("IVF256,PQ64x4", "IVF256,PQ64x16", "IVF256,PQ", "IVF256,PQ0", "IVF0,PQ8", "IVF,PQ8", "ivf256,pq64", "PQ64", "PQ64x8",
                "IVF256,Flat", "IVF256,SQ8", "OPQ16,IVF256,PQ16", "IVF256,PQ64,Flat", "IVF256_HNSW32,PQ64", "IVF256,PQ-4", "IVF256,PQ8x",
                "IVF256 PQ8", ""):
        with pytest.raises(ValueError):
            parse_ivfpq_key(bad)


def test_the_other_parsers_and_classes_keep_refusing_the_key():
    from vdbhip import HipApproximateSearch, HipIVFIndexer, HipPQSearch, get_indexer_class, parse_index_key, parse_pq_key
    from vdbhip.ivf import parse_ivf_key

    for key in ("IVF256,PQ64", "IVF256,PQ64x8", "IVF256,PQ50"):
        for parse in (parse_index_key, parse_ivf_key, parse_pq_key):
            with pytest.raises(ValueError):
                parse(key)
        with pytest.raises(ValueError):
            HipApproximateSearch("a", 64, key)
        with pytest.raises(ValueError):
            HipPQSearch("a", 64, index_type=key)
        for name in ("HipIVFIndexer", "HipFactoryIndexer"):
            assert get_indexer_class(name) is HipIVFIndexer
            with pytest.raises(ValueError):
                get_indexer_class(name)("i", 64, index_key=key)


def test_header_and_ffi_carry_the_ivfpq_entry_points():
    from vdbhip import _ffi

    header = (ROOT / "include" / "vdbhip.h").read_text()
    declared = set(re.findall(r"^int (vdb_ivfpq_[a-z_]+)\(", header, re.M))
    assert declared == IVFPQ_ENTRY_POINTS
    assert IVFPQ_ENTRY_POINTS <= set(_ffi.SIGNATURES)
    assert not any(n.startswith(("vdb_pq_", "vdb_lsh_")) for n in IVFPQ_ENTRY_POINTS)
    assert "#define VDB_ABI_VERSION 4" in header
    lib = _ffi.load()
    for name in IVFPQ_ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.vdb_abi_version() == 4
    # null handle: rejected before any GPU call
    assert lib.vdb_ivfpq_train(None, 8, None, 0, 1, 0, 0) == _ffi.VDB_ERR_INVALID
    assert "null handle" in _ffi.last_error()
    assert lib.vdb_ivfpq_set_codebooks(None, 8, None) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_ivfpq_get_codebooks(None, None, None) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_ivfpq_add_codes(None, None, 0, 0, None) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_ivfpq_get_codes(None, None) == _ffi.VDB_ERR_INVALID
    assert lib.vdb_ivf_set_codec(None, 2) == _ffi.VDB_ERR_INVALID


def test_plugin_classes_validate_without_a_gpu():
    import vdbhip
    from vdbhip import HipIVFPQIndexer, HipIVFPQSearch, HipIVFSearcher, IVFPQIndex

    ix = HipIVFPQIndexer("ivf_pq", 64, index_key="IVF256,PQ64", nprobe=24, seed=7)
    assert ix.index_key == "IVF256,PQ64" and ix.metric == "l2" and ix.params["nprobe"] == 24 and ix.params["seed"] == 7
    assert HipIVFPQIndexer("p", 50, metric="cosine", index_key="IVF256,PQ50").metric == "cosine"
    assert HipIVFPQIndexer("p", 384, metric="ip", index_type="IVF16,PQ64x8").index_key == "IVF16,PQ64x8"
    for key in ("IVF100,Flat", "IVF100,SQ8", "PQ64"):
        with pytest.raises(ValueError):
            HipIVFPQIndexer("p", 64, index_key=key)
        with pytest.raises(ValueError):
            HipIVFPQSearch("a", 64, index_type=key)
    with pytest.raises(ValueError, match="multiple of 48"):
        HipIVFPQIndexer("p", 64, index_key="IVF16,PQ48")
    with pytest.raises(ValueError, match="multiple of 7"):
        HipIVFPQSearch("a", 64, index_type="IVF16,PQ7")
    with pytest.raises(ValueError, match="Expected dimension 64, got 32"):
        ix.build(np.zeros((4, 32), np.float32))
    se = HipIVFSearcher("s", 64)                               # the searcher of the artifact is the IVF one
    with pytest.raises(ValueError, match="hip_ivf"):
        se.attach(vdbhip.IndexArtifact(kind="hip_pq", data=None), np.zeros((1, 64), np.float32))
    algo = HipIVFPQSearch("a", 64, index_type="IVF256,PQ64")
    assert algo.metric == "l2" and HipIVFPQSearch("a", 64, index_type="IVF8,PQ8", metric="cosine").metric == "ip"
    with pytest.raises(RuntimeError, match="not been built"):
        algo.batch_search(np.zeros((1, 64), np.float32), 5)
    with pytest.raises(RuntimeError, match="before build_index"):
        algo.save_index("/nonexistent/dir")
    with pytest.raises(FileNotFoundError):
        algo.load_index("/nonexistent/dir")
    # several devices: refused before any GPU call
    with pytest.raises(ValueError, match="one GPU"):
        IVFPQIndex(64, 16, 8, "l2", [0, 1])
    with pytest.raises(ValueError, match="one GPU"):
        HipIVFPQSearch("a", 64, index_type="IVF16,PQ8", device_ids=[0, 1])
    with pytest.raises(ValueError, match="one GPU"):
        HipIVFPQIndexer("p", 64, index_key="IVF16,PQ8", device_ids=[0, 1])
    for dim, m in ((64, 0), (64, 7), (600, 300), (4, 8)):
        with pytest.raises(ValueError, match="M must divide"):
            IVFPQIndex(dim, 16, m, "l2", 0)


def test_registry_entries():
    import vdbhip
    from vdbhip import HipIVFPQIndexer, HipIVFPQSearch, HipIVFSearcher

    assert vdbhip.get_indexer_class("HipIVFPQIndexer") is HipIVFPQIndexer
    assert [n for n, c in vdbhip.INDEXER_REGISTRY.items() if c is HipIVFPQIndexer] == ["HipIVFPQIndexer"]      # that name only
    assert vdbhip.ALGORITHM_REGISTRY["HipIVFPQSearch"] is HipIVFPQSearch
    assert isinstance(vdbhip.get_algorithm_instance("HipIVFPQSearch", 64, index_type="IVF256,PQ64"), HipIVFPQSearch)
    algo = vdbhip.get_algorithm_instance(                       # the `ivf_pq` row of the reference's config
        "Composite", 64, name="ivf_pq", metric="l2",
        indexer={"type": "HipIVFPQIndexer", "index_key": "IVF256,PQ64", "nprobe": 24}, searcher={"type": "HipIVFSearcher", "nprobe": 24})
    assert isinstance(algo.indexer, HipIVFPQIndexer) and isinstance(algo.searcher, HipIVFSearcher)
    for name in ("HipIVFPQIndexer", "HipIVFPQSearch", "IVFPQIndex", "parse_ivfpq_key"):
        assert name in vdbhip.__all__


def test_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    n, d, M = 200, 8, 4
    dsub = d // M
    C = rng.standard_normal((3, d)).astype(np.float32) * 2
    lor = rng.integers(0, 3, n).astype(np.int32)
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    cb[1, 200] = cb[1, 17]                                      # two equal entries: the smaller index wins whenever they are nearest
    x = (C[lor] + rng.standard_normal((n, d))).astype(np.float32)
    x[0, 2:4] = C[lor[0], 2:4] + cb[1, 200]                     # a row whose residual sits (to rounding) on the duplicated entry
    x[1] = C[lor[1]]                                            # a zero residual
    r = ref.residual(x, C, lor)
    assert r.dtype == np.float32 and np.array_equal(r[1], np.zeros(d, np.float32))
    codes = ref.encode(x, C, lor, cb)
    assert codes.dtype == np.uint8 and codes.shape == (n, M)
    assert np.array_equal(codes, ref.encode_bruteforce(x, C, lor, cb))
    assert codes[0, 1] != 200
    xh = ref.decode(codes, C, lor, cb)
    assert xh.dtype == np.float32 and np.array_equal(xh, ref.decode_bruteforce(codes, C, lor, cb))
    # the residual, not the row, is quantized: the same row under another centroid gets other codes
    assert not np.array_equal(ref.encode(x, C, (lor + 1) % 3, cb), codes)
    # the residual is rounded to float32 BEFORE the float64 chain: dsub = 1, entries 0 and 2^-30, x = 1 + 2^-23 under c_l = 1
    # has the float32 residual 2^-23 exactly, far nearer to 2^-30 than to 0; a large x under a small centroid rounds
    cb1 = np.zeros((1, 256, 1), np.float32)
    cb1[0, 1:, 0] = np.float32(2.0 ** -30) * np.arange(1, 256, dtype=np.float32)
    c1 = np.array([[1.0], [2.0e-8]], np.float32)
    x1 = np.array([[1.0 + 2.0 ** -23], [1.0]], np.float32)
    l1 = np.array([0, 1], np.int32)
    got = ref.encode(x1, c1, l1, cb1)
    assert np.array_equal(got, ref.encode_bruteforce(x1, c1, l1, cb1))
    assert np.float32(1.0) - np.float32(2.0e-8) == np.float32(1.0) and got[1, 0] == 255


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_near_tie_case_is_critical(metric):
    """The near-tie case of tests/test_gpu_ivf_pq.py on the host: with every list probed, the fp16 emulation of the scan over the
    decoded rows gets at least guard_cases.FLOOR of the queries wrong, so a list scan over the codes that drops the guard fails there."""
    t = cases.near_tie_inputs(metric)
    # duplicated rows: identical codes in one list, hence identical decoded rows
    nb = cases.NEAR_TIE_NB
    assert np.array_equal(t["codes"][nb:nb + 64], t["codes"][:64]) and np.array_equal(t["lor"][nb:nb + 64], t["lor"][:64])
    assert np.array_equal(t["Xhat"][nb:nb + 64], t["Xhat"][:64])
    # replicas differ by single codebook entries (never the family)
    a, b = t["codes"][:nb].astype(int), t["codes"][2 * nb:3 * nb].astype(int)
    assert (a // 16 == b // 16).all() and (a != b).any(axis=1).mean() > 0.9
    share = gc.critical_share(t["Xhat"], t["Q"], metric, t["k"])
    print(f"near-tie IVF-PQ case, {metric}: critical share {share:.3f}")
    assert share >= gc.FLOOR, share

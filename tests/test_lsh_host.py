"""Sign-LSH, host side (no GPU): the projection construction, the C-ABI surface, the plugin classes' parameter checks, the
candidate-count formula and the NumPy restatement of the contract on a hand-made example."""
from __future__ import annotations

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import lsh_restatement as ref  # noqa: E402

LSH_ENTRY_POINTS = {"vdb_lsh_set_projection", "vdb_lsh_get_projection", "vdb_lsh_get_codes", "vdb_lsh_candidates",
                    "vdb_lsh_candidates_device", "vdb_lsh_search", "vdb_lsh_search_device"}


@pytest.mark.parametrize("dim,nbits", [(64, 256), (50, 32), (128, 128), (384, 256), (768, 256), (64, 1024)])
def test_make_projection_shape_seed_and_orthonormality(dim, nbits):
    from vdbhip import make_projection

    r = make_projection(dim, nbits, 5)
    assert r.shape == (nbits, dim) and r.dtype == np.float32 and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r, make_projection(dim, nbits, 5))
    assert not np.array_equal(r, make_projection(dim, nbits, 6))
    r64 = r.astype(np.float64)
    if nbits >= dim:
        assert np.abs(r64.T @ r64 - np.eye(dim)).max() <= 1e-5
    else:
        assert np.abs(r64 @ r64.T - np.eye(nbits)).max() <= 1e-5


def test_header_and_ffi_carry_the_lsh_entry_points():
    from vdbhip import _ffi

    header = (ROOT / "include" / "vdbhip.h").read_text()
    declared = set(re.findall(r"^int (vdb_lsh_[a-z_]+)\(", header, re.M))
    assert declared == LSH_ENTRY_POINTS
    assert LSH_ENTRY_POINTS <= set(_ffi.SIGNATURES)
    assert "VDB_PATH_LSH = 4" in header and _ffi.PATH_NAMES[4] == "lsh"
    lib = _ffi.load()
    for name in LSH_ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.vdb_abi_version() == 4
    assert lib.vdb_lsh_set_projection(None, 32, None) == _ffi.VDB_ERR_INVALID          # null handle: no GPU touched


def test_plugin_classes_validate_without_a_gpu():
    import vdbhip
    from vdbhip import HipLSHIndexer, HipLSHSearcher

    ix = HipLSHIndexer("lsh", 64)
    assert ix.num_bits == 256 and ix.metric == "l2" and ix.describe()["params"]["num_bits"] == 256
    for metric in ("l2", "cosine", "ip"):
        assert HipLSHIndexer("lsh", 64, metric=metric, num_bits=64, seed=3).seed == 3
    with pytest.raises(ValueError, match="FaissLSHIndexer supports metrics"):
        HipLSHIndexer("lsh", 64, metric="hamming")
    for bad in (0, -5):
        with pytest.raises(ValueError, match="num_bits must be positive"):
            HipLSHIndexer("lsh", 64, num_bits=bad)
    with pytest.raises(ValueError, match="multiple of 32"):
        HipLSHIndexer("lsh", 64, num_bits=100)
    with pytest.raises(ValueError, match="Expected dimension 64, got 32"):
        ix.build(np.zeros((4, 32), np.float32))
    se = HipLSHSearcher("s", 64)
    assert (se._lsh_rerank, se._lsh_candidate_multiplier, se._lsh_max_candidates) == (True, 8.0, None)
    se = HipLSHSearcher("s", 64, lsh_rerank=False, lsh_candidate_multiplier=64.0, lsh_max_candidates=500)
    assert (se._lsh_rerank, se._lsh_candidate_multiplier, se._lsh_max_candidates) == (False, 64.0, 500)
    with pytest.raises(RuntimeError, match="not attached"):
        se.batch_search(np.zeros((1, 64), np.float32), 5)
    with pytest.raises(ValueError, match="hip_lsh"):
        se.attach(vdbhip.IndexArtifact(kind="faiss", data=None), np.zeros((1, 64), np.float32))
    assert vdbhip.get_indexer_class("HipLSHIndexer") is HipLSHIndexer
    assert vdbhip.get_searcher_class("HipLSHSearcher") is HipLSHSearcher
    algo = vdbhip.get_algorithm_instance(                       # the faiss_lsh_l2 row of the reference's config
        "Composite", 64, name="faiss_lsh_l2", metric="l2",
        indexer={"type": "HipLSHIndexer", "num_bits": 256},
        searcher={"type": "HipLSHSearcher", "lsh_candidate_multiplier": 64.0})
    assert isinstance(algo.indexer, HipLSHIndexer) and isinstance(algo.searcher, HipLSHSearcher)
    with pytest.raises(NotImplementedError):
        algo.save_index("/nonexistent")


def test_candidate_count_follows_the_reference_formula():
    """modular.py:463-468: max(k, 1); int(max(., k * mult)) only when mult > 1; min with lsh_max_candidates; min with ntotal."""
    from vdbhip import HipLSHSearcher
    from vdbhip.lsh import candidate_count

    assert candidate_count(20, 64.0, None, 20000) == 1280
    assert candidate_count(200, 64.0, None, 20000) == 12800
    assert candidate_count(10, 8.0, None, 1_000_000) == 80
    assert candidate_count(10, 1.0, None, 1000) == 10          # multiplier not above 1: k itself
    assert candidate_count(10, 0.5, None, 1000) == 10
    assert candidate_count(10, 2.55, None, 1000) == 25         # int() truncates 25.5
    assert candidate_count(0, 8.0, None, 1000) == 1            # max(k, 1)
    assert candidate_count(10, 8.0, 50, 1000) == 50
    assert candidate_count(10, 8.0, 5, 1000) == 5              # the cap may fall below k
    assert candidate_count(10, 8.0, None, 30) == 30            # never more than the rows
    assert candidate_count(10, 8.0, 0, 1000) == 0
    assert HipLSHSearcher("s", 8, lsh_candidate_multiplier=64.0).candidate_count(20, 20000) == 1280


def test_restatement_on_a_hand_made_example():
    r = np.zeros((32, 2), np.float32)          # rows 2 and 4..31 are zero: those bits are 1 for every vector
    r[0] = (1, 0)
    r[1] = (0, 1)
    r[3] = (-1, -1)
    x = np.array([[1, 1], [0, 0], [-1, 2], [-0.0, -3]], np.float32)
    bits = ref.sign_bits(x, r)
    assert bits[:, 2].all() and bits[:, 4:].all()
    assert bits[1].all()                                        # the all-zero row: every sum is 0.0 -> every bit 1
    assert bits[:, :4].tolist() == [[True, True, True, False], [True, True, True, True], [False, True, True, False],
                                    [True, False, True, True]]
    codes = ref.encode(x, r)
    assert codes.dtype == np.uint32 and codes.shape == (4, 1)
    assert codes[:, 0].tolist() == [0xFFFFFFF7, 0xFFFFFFFF, 0xFFFFFFF6, 0xFFFFFFFD]
    assert not ref.sign_bits(np.array([[np.nan, 1]], np.float32), r).any()      # NaN sums: bit 0 (0 * NaN is NaN too)
    assert np.array_equal(ref.unpack_codes(codes), bits)
    ham = ref.hamming(codes[:1], codes)
    assert ham.dtype == np.int32 and ham.tolist() == [[0, 1, 1, 2]]
    h, i = ref.candidates(codes[:1], codes, 3, id_base=100)
    assert h.tolist() == [[0, 1, 1]] and i.tolist() == [[100, 101, 102]]        # the tie at distance 1 goes to the smaller id
    h, i = ref.candidates(codes[1:2], codes, 6)
    assert h.tolist() == [[0, 1, 1, 2, ref.INT32_MAX, ref.INT32_MAX]] and i.tolist() == [[1, 0, 3, 2, -1, -1]]
    # a 64-bit code: bit j lives in word j / 32
    r2 = np.zeros((64, 2), np.float32)
    r2[40] = (-1, 0)
    assert ref.encode(np.array([[1, 0]], np.float32), r2).tolist() == [[0xFFFFFFFF, 0xFFFFFEFF]]

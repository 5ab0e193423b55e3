"""CPU-only checks of the IVF<nlist>,SQ8 surface: key parsing, plugin construction, and the C-ABI declarations."""
from __future__ import annotations

import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_index_key_parser_accepts_flat_and_sq8_only():
    from vdbhip.ivf import parse_index_key, parse_ivf_key

    assert parse_index_key("IVF256,SQ8") == (256, "SQ8")
    assert parse_index_key(" IVF1024 , Flat ") == (1024, "Flat")
    for bad in ("IVF32,PQ8", "PQ64", "SQ8", "IVF256,SQ4", "IVF256,SQfp16", "Flat", "IVF,SQ8"):
        with pytest.raises(ValueError):
            parse_index_key(bad)
    # the row-sharded form keeps serving Flat lists only
    assert parse_ivf_key("IVF64,Flat") == 64
    with pytest.raises(ValueError):
        parse_ivf_key("IVF256,SQ8")


def test_plugins_accept_sq8_keys_without_touching_the_gpu():
    import vdbhip
    from vdbhip.ivf import HipApproximateSearch, HipIVFIndexer

    algo = HipApproximateSearch("ivf_sq8", 64, index_type="IVF256,SQ8", metric="l2", nprobe=24)
    assert algo.index_type == "IVF256,SQ8" and algo._format() == "vdbhip-ivfsq8-v1"
    assert HipApproximateSearch("f", 64, index_type="IVF256,Flat")._format() == "vdbhip-ivfflat-v1"
    ix = vdbhip.get_indexer_class("HipFactoryIndexer")("ivf_sq8", 64, metric="cosine", index_key="IVF256,SQ8", nprobe=48)
    assert isinstance(ix, HipIVFIndexer) and ix.index_key == "IVF256,SQ8"
    with pytest.raises(ValueError):
        HipApproximateSearch("pq", 64, index_type="IVF32,PQ8")
    with pytest.raises(ValueError):
        HipIVFIndexer("pq", 64, index_key="IVF32,PQ8")
    with pytest.raises(ValueError):
        vdbhip.HipShardedApproximateSearch("s", 64, index_type="IVF256,SQ8")


def test_sq8_index_refuses_several_devices_before_any_gpu_call():
    from vdbhip.ivf import IVFSQ8Index

    with pytest.raises(ValueError, match="one GPU"):
        IVFSQ8Index(64, 256, "l2", device=[0, 1])


def test_header_documents_the_sq8_entry_points():
    header = (ROOT / "include" / "vdbhip.h").read_text()
    for name in ("vdb_ivf_set_codec", "vdb_ivf_sq8_train_ranges", "vdb_ivf_sq8_set_ranges", "vdb_ivf_sq8_get_ranges",
                 "vdb_ivf_get_codes"):
        assert re.search(r"\bint " + name + r"\(", header), name
    from vdbhip import _ffi

    assert {"vdb_ivf_set_codec", "vdb_ivf_get_codes"} <= set(_ffi.SIGNATURES)

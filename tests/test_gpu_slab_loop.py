"""Per-search panels, slab by slab: a streamed index (`stream_panels`) and an int8-only index (`int8_only`) make the fp16
panels of every search in a scratch slab, a few scan chunks at a time.  The shapes are the smallest that give several slabs,
chunks of two lengths (the spans do not divide evenly over the chunks) and a short last slab; results must be those of the
index that keeps its panels resident, bit for bit, whatever the slab size.  (PQ: the `pq_slab_chunks` sweep of test_gpu_pq.)"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCHES = (600, 64, 3)


@pytest.fixture(scope="module")
def vdb():
    import vdbhip

    return vdbhip


@pytest.fixture(scope="module")
def streamed(vdb, oracle):
    """47 000 x 136 Gaussian rows (p16 panels, 46 spans of 1024 rows): 600 queries scan 12 chunks of 3 or 4 spans, 64 or 3
    queries 24 chunks of 1 or 2 spans.  One resident and one streamed index, the resident results per batch, the oracle's ids."""
    rng = np.random.default_rng(47)
    X = rng.standard_normal((47_000, 136)).astype(np.float32)
    Q = rng.standard_normal((600, 136)).astype(np.float32)
    res = vdb.FlatIndex(136, "l2", 0)
    res.add(X)
    want = {nq: res.search(Q[:nq], 10) for nq in BATCHES}
    res.close()
    Io = oracle.knn(X, Q, 10, "l2")[1]
    idx = vdb.FlatIndex(136, "l2", 0)
    idx.set_option("stream_panels", 1)
    idx.add(X)
    yield idx, Q, want, Io
    idx.close()


@pytest.mark.parametrize("slab_rows", [0, 4096, 12288, 20480])
def test_streamed_slabs_equal_the_resident_index(streamed, slab_rows):
    """600 queries: 1 / 12 / 4 / 3 slabs (20 480 rows = 5 chunks of up to 4 spans: 5 + 5 + 2)."""
    idx, Q, want, Io = streamed
    idx.set_option("stream_slab_rows", slab_rows)
    for nq in BATCHES:
        D, I = idx.search(Q[:nq], 10)
        assert idx.stats()["last_path_name"] == "mfma_scan"
        np.testing.assert_array_equal(I, want[nq][1], err_msg=f"nq={nq}")
        np.testing.assert_array_equal(D, want[nq][0], err_msg=f"nq={nq}")
        np.testing.assert_array_equal(I, Io[:nq], err_msg=f"nq={nq}")


@pytest.fixture(scope="module")
def int8_only(vdb):
    """40 000 x 50 byte-valued rows (u8 window, 79 spans of 512 rows): 600 queries scan 32 chunks of 2 or 3 spans.  A default
    and an int8-only index; the default index's results for non-integer batches (fp16 scan) and for an integer batch."""
    rng = np.random.default_rng(50)
    X = np.clip(np.round(rng.gamma(0.6, 40.0, size=(40_000, 50))), 0, 218).astype(np.float32)
    Qi = np.clip(np.round(rng.gamma(0.6, 40.0, size=(600, 50))), 0, 218).astype(np.float32)
    Qf = (Qi + rng.standard_normal(Qi.shape).astype(np.float32) * 3).astype(np.float32)
    ref = vdb.FlatIndex(50, "l2", 0)
    ref.add(X)
    want = {(nq, k): ref.search(Qf[:nq], k) for nq in BATCHES for k in (10, 100)}
    want_int = ref.search(Qi, 10)
    ref.close()
    idx = vdb.FlatIndex(50, "l2", 0)
    idx.set_option("int8_only", 1)
    idx.add(X)
    assert idx.stats()["has_i8_copy"] == 2
    yield idx, Qi, Qf, want, want_int
    idx.close()


@pytest.mark.parametrize("slab_chunks", [0, 1, 3, 1024])
def test_int8_only_slabs_equal_the_default_index(int8_only, slab_chunks):
    """600 queries: 4 / 32 / 11 (the last of 2 chunks) / 1 slabs.  k = 100 takes the direct-bin geometry (64-row bins)."""
    idx, Qi, Qf, want, want_int = int8_only
    idx.set_option("int8_slab_chunks", slab_chunks)
    for nq in BATCHES:
        for k in (10, 100):
            D, I = idx.search(Qf[:nq], k)
            st = idx.stats()
            assert st["last_path_name"] == "mfma_scan", st
            if k == 10:
                assert st["scan_dtype"] == 0, st          # (non-integer batch: the fp16 slabs served it)
            np.testing.assert_array_equal(I, want[nq, k][1], err_msg=f"nq={nq} k={k}")
            np.testing.assert_array_equal(D, want[nq, k][0], err_msg=f"nq={nq} k={k}")
    D, I = idx.search(Qi, 10)
    st = idx.stats()
    assert st["last_path_name"] == "mfma_scan" and st["scan_dtype"] == 1, st
    np.testing.assert_array_equal(I, want_int[1])
    np.testing.assert_array_equal(D, want_int[0])

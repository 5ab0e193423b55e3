"""Host model of WaveTopK::offer (tests/topk_model.py) and the cases of tests/test_gpu_topk.py, checked without a GPU.

Every generated case must keep the input contract of the merge entry points, the model's final list must equal
np.lexsort((ids, keys))[:k] and the C oracle, and a case that states branch counts must reach them under the `kBatchMin`
the library is built with (read from csrc/topk.hpp): a case that misses its branch fails here, before it runs on a GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

from . import topk_cases as tc
from . import topk_model as tm


def test_kpl_table():
    assert [tm.kpl_for(k) for k in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert {tm.kpl_for(k) for k in tc.KS} == {1, 2, 4, 8, 16, 32}


def test_sortable_order_and_round_trip():
    v = np.array([-np.inf, -3.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.nextafter(1.0, 2.0), 1e300, np.inf])
    u = tm.sortable_u64(v)
    assert (np.diff(u.astype(object)) > 0).all()
    assert tm.unsortable_f64(u).tobytes() == v.tobytes()
    assert int(u[-1]) < 2**64 - 1          # +inf as a real key still sorts below the sentinel of an empty slot


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_plain_orders(order):
    """Sorted parts in a plain order: the model agrees with lexsort."""
    rng = np.random.default_rng(5)
    for k in (64, 129, 1025):
        nparts = 8
        keys = np.sort(rng.random((nparts, 1, k)), axis=-1)
        if order == "ascending":
            keys += np.arange(nparts)[:, None, None]
        elif order == "descending":
            keys -= np.arange(nparts)[:, None, None]
        ids = rng.permutation(nparts * k).reshape(nparts, 1, k).astype(np.int64)
        lk, li, c = tm.offer_stream(*tm.merge_stream(keys, ids, 0), k, tm.batch_min_from_header())
        D, I = tm.lexsort_rows(keys, ids, k, "l2")
        np.testing.assert_array_equal(tm.final_rows(lk, li, k, "l2")[1], I[0])


def test_rerank_order_with_holes():
    """rerank_kernel offers its candidates in array order, holes (invalid lanes) included."""
    rng = np.random.default_rng(6)
    for k in (5, 64, 65, 200):
        n = 1000
        keys = np.round(rng.standard_normal(n), 1)
        ids = rng.permutation(4 * n)[:n].astype(np.int64)
        valid = rng.random(n) < 0.8
        lk, li, c = tm.offer_stream(keys, ids, valid, k, tm.batch_min_from_header())
        o = np.lexsort((ids[valid], keys[valid]))[:k]
        np.testing.assert_array_equal(li, ids[valid][o])
        np.testing.assert_array_equal(lk, keys[valid][o])
        assert c.serial_full + c.serial_partial > 0 and c.batch_full + c.batch_partial + c.batch_empty > 0


@pytest.mark.parametrize("batch_min", [1, 12, 65])
def test_model_result_does_not_depend_on_the_route(batch_min):
    c = tc.case_by_name("branch-k129-ip")
    D, I = tm.lexsort_rows(c.keys, c.ids, c.k, c.metric)
    for q in range(c.nq):
        lk, li, cnt = tm.offer_stream(*tm.merge_stream(c.keys, c.ids, q), c.k, batch_min)
        Dm, Im = tm.final_rows(lk, li, c.k, c.metric)
        np.testing.assert_array_equal(Im, I[q])
        np.testing.assert_array_equal(Dm, D[q])
        if batch_min == 65:
            assert cnt.batch_empty + cnt.batch_partial + cnt.batch_full == 0
        if batch_min == 1:
            assert cnt.serial_partial + cnt.serial_full == 0


def test_case_names_cover_the_issue():
    names = tc.case_names()
    assert len(names) == len(set(names)) == len(tc.KINDS) * len(tc.KS) * 2 + 1
    nqs = {tc.case_by_name(n).nq for n in names if "-k64-" in n or n.startswith("many")}
    assert {1, 3, 4, 5, 16392} <= nqs
    assert any((tc.case_by_name(n).nparts * tc.case_by_name(n).k) % 64 for n in names)


@pytest.mark.parametrize("name", tc.case_names())
def test_case(name, oracle):
    c = tc.case_by_name(name)
    assert c.keys.shape == c.ids.shape == (c.nparts, c.nq, c.k)
    assert c.keys.dtype == np.float64 and c.ids.dtype == np.int64
    tc.check_contract(c)
    D, I = tm.lexsort_rows(c.keys, c.ids, c.k, c.metric)
    Do, Io = oracle.merge_partials(c.keys, c.ids, c.metric)
    np.testing.assert_array_equal(Io, I)
    np.testing.assert_array_equal(Do, D)
    if not c.model:
        return
    bm = tm.batch_min_from_header()
    for q in range(c.nq):
        lk, li, cnt = tm.offer_stream(*tm.merge_stream(c.keys, c.ids, q), c.k, bm)
        Dm, Im = tm.final_rows(lk, li, c.k, c.metric)
        np.testing.assert_array_equal(Im, I[q])
        np.testing.assert_array_equal(Dm, D[q])
        if c.require:
            for what, least in c.require.items():
                if what == "accepted":
                    assert set(least) <= cnt.accepted_full, (name, q, sorted(cnt.accepted_full))
                else:
                    assert getattr(cnt, what) >= least, (name, q, what, least, cnt)


def test_special_cases_are_what_they_say():
    for metric in tc.METRICS:
        for k in tc.KS:
            c = tc.case_by_name(f"short-k{k}-{metric}")
            valid = (c.ids >= 0).sum(axis=(0, 2))
            assert valid[2] < k and valid[3] == 0 and valid[4] == k
            assert ((c.ids[:, 1] >= 0).sum(axis=1) == 0).any()                  # a whole part empty
            c = tc.case_by_name(f"ties-k{k}-{metric}")
            assert len(np.unique(c.keys[:, 0][c.ids[:, 0] >= 0])) == 1
            D, _ = tm.lexsort_rows(c.keys, c.ids, k, metric)
            if k > 1:
                assert D[2, k - 1] == D[2, k - 2]                                # a run of equal keys ends the list ...
            allk = np.sort(c.keys[:, 2][c.ids[:, 2] >= 0])
            assert allk[k - 1] == allk[k]                                        # ... and goes on past slot k - 1
            if k > 64:                                                           # ... and one straddles a register boundary
                assert any(allk[s - 1] == allk[s] for s in range(64, k, 64))
            c = tc.case_by_name(f"values-k{k}-{metric}")
            v = c.keys[c.ids >= 0]
            assert np.isposinf(v).any() and (np.abs(v[v != 0]) < 2.3e-308).any() and (v == 0).any()
            assert np.signbit(v[v == 0]).all() == (metric == "ip")
            assert (v < 0).any() == (metric == "ip")
    c = tc.case_by_name("many-queries-k3-l2")
    assert c.nq == 16385 + 7 and c.nq > 4096 * 4 and c.nparts == 2 and c.k == 3      # more slots than the capped grid has waves

"""The reference of the filtered IVF-Flat search and its mask generators (tests/ivf_filter_cases.py), checked on the CPU.

`reference()` -- the oracle's IVF search over the admitted rows, ids mapped back -- must equal the definition stated directly: per
query the nprobe nearest lists, pair_keys over the ADMITTED rows of those lists, lexsort by (key, id).  No GPU."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from tests import ivf_filter_cases as ic

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32


def _small(metric, seed=5, n=900, d=12, nlist=9, nq=11):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(F32)
    X[n // 2:n // 2 + 40] = X[:40]                 # exact duplicates: ties by id
    Q = rng.standard_normal((nq, d)).astype(F32)
    Q[0] = X[3]
    C = X[:nlist].copy()
    return X, C, Q, ic.host_assign(C, X, metric)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_reference_equals_the_definition(oracle, metric):
    X, C, Q, lor = _small(metric)
    probed = ic.nearest_lists(C, Q[0], metric, 3)
    for name, mask in ic.masks(len(X), lor, probed).items():
        for k, nprobe, id_base in ((1, 1, 0), (10, 3, 1_000_003), (100, 9, 0)):
            got = ic.reference(oracle.ivf_search, X, C, lor, Q, k, nprobe, metric, mask, id_base)
            want = ic.brute_reference(oracle.pair_keys, X, C, lor, Q, k, nprobe, metric, mask, id_base)
            np.testing.assert_array_equal(got[1], want[1], err_msg=f"{metric} {name} k={k} nprobe={nprobe}")
            np.testing.assert_array_equal(got[0], want[0], err_msg=f"{metric} {name} k={k} nprobe={nprobe}")
            assert got[0].dtype == F32 and got[1].dtype == np.int64


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_all_ones_is_the_unfiltered_search_and_all_zeros_is_padding(oracle, metric):
    X, C, Q, lor = _small(metric, seed=6)
    ones, zeros = np.ones(len(X), np.bool_), np.zeros(len(X), np.bool_)
    d, i = ic.reference(oracle.ivf_search, X, C, lor, Q, 10, 3, metric, ones, 7)
    do, io = oracle.ivf_search(X, C, lor, Q, 10, 3, metric, id_base=7)
    assert d.tobytes() == do.tobytes() and i.tobytes() == io.tobytes()
    d, i = ic.reference(oracle.ivf_search, X, C, lor, Q, 10, 3, metric, zeros)
    assert (i == -1).all() and (d == ic.pad_value(metric)).all()


def test_mask_generators():
    n, nlist = 20000, 64
    lor = (np.random.default_rng(1).integers(0, nlist, n)).astype(np.int32)
    probed = np.array([5, 17, 40])
    m = ic.masks(n, lor, probed)
    assert set(m) == {"all-ones", "all-zeros", "random-0.5", "random-0.1", "random-0.01", "id-run", "three-lists-cleared", "one-list-only",
                      "single-row", "last-row"}
    for dens in (0.5, 0.1, 0.01):
        got = m[f"random-{dens}"].mean()
        assert abs(got - dens) < 4 * np.sqrt(dens * (1 - dens) / n), (dens, got)          # four standard deviations of a binomial
    assert m["all-ones"].all() and not m["all-zeros"].any()
    run = np.flatnonzero(m["id-run"])
    assert len(run) == n // 10 and (np.diff(run) == 1).all()
    assert not m["three-lists-cleared"][np.isin(lor, probed)].any() and m["three-lists-cleared"][~np.isin(lor, probed)].all()
    assert (lor[m["one-list-only"]] == 5).all() and m["one-list-only"].sum() == (lor == 5).sum()
    assert m["single-row"].sum() == 1 and m["last-row"].sum() == 1 and m["last-row"][n - 1]
    assert all(not v.flags.writeable for v in m.values())
    w = ic.tail_set_words(m["last-row"][:n - 7])
    assert len(w) == (n - 7 + 31) // 32 and int(w[-1]) >> ((n - 7) % 32) == (1 << (32 - (n - 7) % 32)) - 1


def test_list_order_is_stable_by_list():
    lor = np.array([2, 0, 1, 0, 2, 2, 1], np.int32)
    perm, off = ic.list_order(lor)
    assert perm.tolist() == [1, 3, 2, 6, 0, 4, 5] and off.tolist() == [0, 2, 4, 7]


def test_header_documents_the_calls_and_the_table_rows():
    header = (ROOT / "include" / "vdbhip.h").read_text()
    for fn in ("vdb_ivf_filter_set", "vdb_ivf_filter_set_device", "vdb_ivf_filter_count", "vdb_ivf_search_filtered", "vdb_ivf_search_filtered_device"):
        assert re.search(r"^int " + fn + r"\(vdb_handle h", header, re.M), fn
    row = re.search(r"vdb_ivf_search_filtered\(_device\)\s+([+US ]+)$", header, re.M)
    assert row and row.group(1).split() == ["+", "U", "U", "U", "U", "+", "U", "U", "U"]
    assert "#define VDB_ABI_VERSION 4" in header

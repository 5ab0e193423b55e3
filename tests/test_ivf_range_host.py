"""Host side of the range search on IVF-Flat indexes: the reference of tests/ivf_range_cases.py against the definition stated
directly, the C-ABI surface of the four calls, and the near-tie cases.

A condition, not a measurement: on every near-tie case the NumPy emulation of (scan score, packed minimum, threshold, marks) with the
bare threshold -- eps = 0 -- leaves out a true result for at least a quarter of the queries, and with the library's bound it leaves
out none.  A case below the floor would pass on the GPU with the bound removed; it fails here instead.  The shares measured when the
cases were written are in tests/golden/ivf_range_measurements.json.  No GPU."""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import guard_cases as gc
from tests import ivf_filter_cases as ic
from tests import ivf_range_cases as irc
from tests import range_cases as rc

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
FLOOR = 0.25             # share of the queries the bare threshold must fail on every near-tie case


def _small(metric, seed, n, d, nlist, nq):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(F32)
    X[n // 2:n // 2 + 40] = X[:40]                 # exact duplicates: equal D on both sides of a radius
    Q = rng.standard_normal((nq, d)).astype(F32)
    Q[0] = X[3]
    C = X[:nlist].copy()
    return X, C, Q, ic.host_assign(C, X, metric)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", [(900, 12, 9, 11), (1500, 20, 5, 7)], ids=["900x12", "1500x20"])
def test_reference_equals_the_definition(oracle, metric, shape):
    X, C, Q, lor = _small(metric, 5 + shape[1], *shape)
    for nprobe, id_base in ((1, 0), (3, 1_000_003), (shape[2], 0)):
        full = irc.full_lists(oracle.ivf_search, X, C, lor, Q, nprobe, metric)
        assert (full[1] >= 0).sum(axis=1).max() <= irc.probed_rows_bound(lor, len(C), nprobe) == full[0].shape[1]
        for name, r in irc.radii(full, metric).items():
            got = irc.cut(full, lor, r, metric, id_base)
            want = irc.brute_reference(oracle.pair_keys, X, C, lor, Q, nprobe, metric, r, id_base)
            for g, w, part in zip(got, want, ("lims", "D", "I")):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (metric, name, nprobe, part)
            if name == "a-returned-D":             # the strict comparison leaves the row with that very D out
                assert not (got[1] == F32(r)).any() and (full[0] == F32(r)).any()
        # (list, id) order, and nprobe = nlist returns the flat rule's rows
        lims, _, I = irc.cut(full, lor, irc.radii(full, metric)["median100"], metric)
        for q in range(len(Q)):
            rows = I[lims[q]:lims[q + 1]]
            assert (np.diff(lor[rows].astype(np.int64) * len(X) + rows) > 0).all()
    keys = oracle.pair_keys(X, Q, np.tile(np.arange(len(X), dtype=np.int64), (len(Q), 1)), metric)
    r = irc.radii(full, metric)["median100"]
    flat = rc.expected(keys, r, metric)
    lims, D, I = irc.cut(full, lor, r, metric)
    assert np.array_equal(lims, flat[0])
    for q in range(len(Q)):
        assert sorted(I[lims[q]:lims[q + 1]].tolist()) == flat[2][lims[q]:lims[q + 1]].tolist()


def test_abi_surface():
    from vdbhip import _ffi

    header = (ROOT / "include" / "vdbhip.h").read_text()
    names = ("vdb_ivf_range_search", "vdb_ivf_range_results", "vdb_ivf_range_search_device", "vdb_ivf_range_results_device")
    lib = _ffi.load()
    for name in names:
        proto = re.search(rf"^int {name}\((.*?)\);", header, re.M | re.S)
        assert proto, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == len(proto.group(1).split(",")), name
        assert hasattr(lib, name), name
        flat = name.replace("vdb_ivf_", "vdb_")
        assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[flat], name
    assert re.search(r"VDB_PATH_IVF_RANGE = 11\b", header) and _ffi.PATH_NAMES[11] == "ivf_range"
    assert "#define VDB_ABI_VERSION 4" in header and lib.vdb_abi_version() == 4
    row = re.search(r"vdb_ivf_range_results\(_device\)\s+([+US ]+)$", header, re.M)
    assert row and row.group(1).split() == ["+", "U", "U", "U", "U", "+", "U", "U", "U"]
    # a null handle is refused by every one of them, with a message, before anything else is looked at
    for name in names:
        args = [0 if t in (_ffi.c_int64,) else 0.0 if t is _ffi.c_float else None for t in _ffi.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == _ffi.VDB_ERR_INVALID and "null handle" in _ffi.last_error(), name


def test_python_layer_offers_the_calls():
    from vdbhip import ivf, ivf_pq

    for cls in (ivf.IVFFlatIndex, ivf.IVFSQ8Index, ivf_pq.IVFPQIndex):
        assert cls.range_search is ivf.IVFFlatIndex.range_search and cls.range_search_device is ivf.IVFFlatIndex.range_search_device
    assert callable(ivf.HipApproximateSearch.range_search) and callable(ivf.HipIVFSearcher.range_search)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "ivf_range_measurements.json").read_text())["eps0_missed_share"]


@pytest.mark.parametrize("case", irc.NEAR_TIE_CASES, ids=lambda c: c.id)
def test_eps_decides_the_near_tie_cases(case, oracle, recorded):
    X, C, Q, radius = irc.near_tie(case)
    lor = gc.host_assign(C, X, case.metric)
    keys = oracle.pair_keys(X, Q, np.tile(np.arange(len(X), dtype=np.int64), (len(Q), 1)), case.metric)
    bare, per_query = irc.emulated_miss(X, C, lor, Q, radius, case.metric, keys, np.zeros(len(Q)))
    guarded, _ = irc.emulated_miss(X, C, lor, Q, radius, case.metric, keys, rc.library_eps(X, Q, case.metric))
    print(f"{case.id}: share of queries with a missed result at eps = 0: {bare:.3f}; with the library's bound: {guarded:.3f}; "
          f"{per_query:.2f} true results per query among the probed rows")
    assert bare >= FLOOR, bare
    assert guarded == 0.0, guarded
    assert 2.0 < per_query < 9.0, per_query            # the radius cuts through the replicas of a cluster, and through nothing else
    assert abs(bare - recorded[case.id]["share"]) < 0.1, (bare, recorded[case.id])


@pytest.mark.parametrize("case", irc.PACK_CASES, ids=lambda c: c.id)
def test_packing_term_alone_decides_the_integer_cases(case, oracle, recorded):
    """Exact integer scores: the library's eps is 1.02 pack_err and nothing else, and without it (eps = 1e-30: only the float64
    allowance of the threshold is left) the packed minima lose a true result for at least a quarter of the queries"""
    X, C, Q, radius = irc.pack_case(case)
    assert (X == np.rint(X)).all() and (Q == np.rint(Q)).all() and gc.scales(X, Q, case.metric) == (1.0, 1.0)
    lor = gc.host_assign(C, X, case.metric)
    keys = oracle.pair_keys(X, Q, np.tile(np.arange(len(X), dtype=np.int64), (len(Q), 1)), case.metric)
    eps = rc.library_eps(X, Q, case.metric)
    np.testing.assert_allclose(eps, irc.pack_only_eps(X, Q, case.metric), rtol=1e-6)
    # the scores of the true results are integers of magnitude >= 2^18, where the six packed bits are worth 1.97 and the nearest true
    # result is 0.5 below the radius (the corpora put them near 1.4e6 and 2.8e6: 7.9 and 15.75)
    dist = keys.astype(F32)
    truth = dist < radius
    scores = gc.emulated_scores(X, Q, case.metric)[truth]
    assert (scores == np.rint(scores)).all() and np.abs(scores).min() >= 2.0 ** 18
    assert sorted(np.unique(dist[truth]).tolist()) == [float(irc.PACK_SHIFT + j) for j in range(6)]
    bare, per_query = irc.emulated_miss(X, C, lor, Q, radius, case.metric, keys, np.full(len(Q), 1e-30), nprobe=irc.PACK_NPROBE)
    guarded, _ = irc.emulated_miss(X, C, lor, Q, radius, case.metric, keys, eps, nprobe=irc.PACK_NPROBE)
    print(f"{case.id}: share of queries with a missed result without pack_err: {bare:.3f}; with the library's bound: {guarded:.3f}; "
          f"{per_query:.2f} true results per query among the probed rows")
    assert bare >= FLOOR, bare
    assert guarded == 0.0, guarded
    assert per_query == 6.0, per_query
    assert abs(bare - recorded[case.id]["share"]) < 0.1, (bare, recorded[case.id])


def test_fixture_names_every_case(recorded):
    assert sorted(recorded) == sorted(c.id for c in irc.NEAR_TIE_CASES + irc.PACK_CASES)


def test_emulated_marks_follow_the_kernel_rule():
    """one list of 200 rows, quads of 4, bins of 64, three minima kept: a passing quad marks its 4 rows; three passing quads in one
    bin mark the bin; the last bin is clipped at the list's end"""
    n, d = 200, 8
    X = np.zeros((n, d), F32)
    X[:, 0] = 100.0
    for r in (5, 70, 75, 81, 199):
        X[r, 0] = 1.0                                  # the rows near the query
    Q = np.zeros((1, d), F32)
    Q[0, 0] = 1.0
    lor = np.zeros(n, np.int32)
    m = irc.emulated_marks(X, lor, Q, 4.0, "l2", np.zeros(1), 64, 4, 3)[0]
    want = np.zeros(n, bool)
    want[4:8] = True                                   # bin 0: one quad
    want[64:128] = True                                # bin 1: three passing quads -> the whole bin
    want[196:200] = True                               # bin 3 (rows 192 .. 199): one quad, clipped list end
    assert np.array_equal(m, want), np.flatnonzero(m != want)

"""Host side of the range search: the near-threshold inputs of tests/range_cases.py make the `+ eps` of the prefilter decisive, and
the C-ABI surface of the four calls.

A condition, not a measurement: on every case the NumPy emulation of the scan (guard_cases.emulated_scores) with the bare threshold
cs (radius - ||q||^2) / cs (-radius) -- eps = 0 -- misses a true result for at least guard_cases.FLOOR of the queries, and with the
library's bound (range_cases.library_eps) it misses none.  A case below the floor would pass on the GPU with the bound removed; it
fails here instead.  The shares measured when the cases were written are in tests/golden/range_measurements.json."""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import guard_cases as gc
from tests import range_cases as rc

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "range_measurements.json").read_text())["eps0_missed_share"]


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.id)
def test_eps_decides_the_near_threshold_cases(case, oracle, recorded):
    X, Q, radius = rc.make(case)
    keys = oracle.pair_keys(X, Q, np.tile(np.arange(len(X), dtype=np.int64), (len(Q), 1)), case.metric)
    bare, per_query = rc.missed_share(X, Q, radius, case.metric, keys, np.zeros(len(Q)))
    guarded, _ = rc.missed_share(X, Q, radius, case.metric, keys, rc.library_eps(X, Q, case.metric))
    print(f"{case.id}: share of queries with a missed result at eps = 0: {bare:.3f}; with the library's bound: {guarded:.3f}; "
          f"{per_query:.2f} true results per query")
    assert bare >= gc.FLOOR, bare
    assert guarded == 0.0, guarded
    assert 2.0 < per_query < 9.0, per_query            # the radius cuts through the 11 replicas of a cluster, and through nothing else
    assert abs(bare - recorded[case.id]["share"]) < 0.1, (bare, recorded[case.id])


def test_fixture_names_every_case(recorded):
    assert sorted(recorded) == sorted(c.id for c in rc.CASES)


def test_expected_applies_the_contract():
    keys = np.array([[0.0, 1.0, np.nan, np.inf, 0.5], [-np.inf, 2.0, 0.25, np.nan, -3.0]])
    lims, d, i = rc.expected(keys, 1.0, "l2", id_base=10)
    assert lims.tolist() == [0, 2, 5] and i.tolist() == [10, 14, 10, 12, 14] and d.tolist()[:2] == [0.0, 0.5]  # (-inf < 1 passes; NaN, +inf never)
    lims, d, i = rc.expected(keys, 0.0, "ip")
    assert lims.tolist() == [0, 0, 2] and i.tolist() == [0, 4] and d.tolist() == [np.inf, 3.0]                   # a score of +inf is returned
    assert rc.expected(keys, np.inf, "ip")[0].tolist() == [0, 0, 0] and rc.expected(keys, -1.0, "l2")[0].tolist() == [0, 0, 2]


def test_abi_surface():
    from vdbhip import _ffi

    header = (ROOT / "include" / "vdbhip.h").read_text()
    names = ("vdb_range_search", "vdb_range_results", "vdb_range_search_device", "vdb_range_results_device")
    lib = _ffi.load()
    for name in names:
        proto = re.search(rf"^int {name}\((.*?)\);", header, re.M | re.S)
        assert proto, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == len(proto.group(1).split(",")), name
        assert hasattr(lib, name), name
    assert re.search(r"VDB_PATH_RANGE = 9\b", header) and _ffi.PATH_NAMES[9] == "range"
    assert "#define VDB_ABI_VERSION 4" in header and lib.vdb_abi_version() == 4
    # a null handle is refused by every one of them, with a message, before anything else is looked at
    for name in names:
        args = [0 if t in (_ffi.c_int64,) else 0.0 if t is _ffi.c_float else None for t in _ffi.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == _ffi.VDB_ERR_INVALID and "null handle" in _ffi.last_error(), name

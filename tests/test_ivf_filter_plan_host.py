"""The sizing and routing rules of a filtered IVF-Flat search (csrc/ivf_filter_plan.hpp) run as a host program, against hand-computed
sizes and a restatement of the rule.

tests/host/ivf_filter_plan_main.cpp includes the header the library sizes and routes by and prints, per case, the unfiltered
ivf_geometry, the filtered one, the rule on its own and the bytes of an install.  No GPU, no HIP: built with the host compiler
(`make ivf_filter_plan`), and once more with the address and undefined-behaviour sanitizers; both builds must print the same lines."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"


def build(target):
    prog = PKG / "build" / target
    srcs = [ROOT / "tests" / "host" / "ivf_filter_plan_main.cpp"] + [PKG / "csrc" / f for f in (
        "ivf_filter_plan.hpp", "ivf_plan.hpp", "scan_plan.hpp", "filter_plan.hpp", "range_plan.hpp")]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", target], check=True)
    return prog


# N nlist pspans max_pspans d k nq nprobe n_allowed force_path i8
BASE = (20000, 64, 120, 3, 64, 10, 300, 8)         # the 20 000 x 64 index of the GPU tests: ~1.9 spans per list, 60 bins per query
CASES = []
for n_allowed in (20000, 19999, 10000, 2000, 321, 320, 319, 200, 1, 0):
    for force in (0, 1, 2):
        CASES.append(BASE + (n_allowed, force, n_allowed % 2))
CASES += [(20000, 64, 120, 3, 64, 1, 300, 8, na, 0, 0) for na in (33, 32, 31)]              # k = 1: 4 admitted rows probed
CASES += [(20000, 64, 120, 3, 64, 10, 300, 16, na, 0, 0) for na in (161, 160, 159)]         # nprobe 16: the boundary halves
CASES += [(20000, 64, 120, 3, 64, 100, 300, 16, na, 0, 0) for na in (20000, 10000)]         # k = 100: ivf_geometry itself declines
CASES += [(30000, 64, 150, 4, 200, 10, 300, 8, na, 0, 0) for na in (30000, 321, 320, 319)]  # D > 128: 256-row spans of 16 p16 tiles
CASES += [(60000, 16, 64, 5, 256, 10, 200, 4, na, 0, 0) for na in (60000, 161, 160, 159)]   # ... 1024-row spans (ivf_tps 64 by rule)
CASES += [(320, 64, 64, 1, 64, 10, 80, 16, na, 0, 0) for na in (320, 240, 161, 160, 159)]   # 5 rows per list: more bins than rows
CASES += [(1000003, 1024, 4400, 9, 128, 10, 10000, 32, na, 0, 1) for na in (1000003, 500000, 10000, 1281, 1280, 1279)]
TEXT = "".join(" ".join(map(str, c)) + "\n" for c in CASES)


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([str(build("ivf_filter_plan"))], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    return out


def test_bytes_against_hand_computed_sizes(lines):
    got = {c: json.loads(line) for c, line in zip(CASES, lines)}
    # 20 000 rows: 313 units of 64 rows = 626 words = 2504 bytes, + 8 (count); 120 spans x 256 rows = 30 720 panel rows
    p = got[BASE + (20000, 0, 0)]
    assert p["words"] == 626 and p["bytes"] == 2504 + 8 + 30720 * 4 == 125392
    p = got[BASE + (19999, 0, 1)]                  # with the int8 copy: two more windows
    assert p["bytes"] == 2504 + 8 + 30720 * 4 + 2 * 30720 * 4 == 371152
    p = got[(30000, 64, 150, 4, 200, 10, 300, 8, 30000, 0, 0)]
    assert p["span_rows"] == 256 and p["words"] == 938 and p["bytes"] == 938 * 4 + 8 + 150 * 256 * 4
    p = got[(60000, 16, 64, 5, 256, 10, 200, 4, 60000, 0, 0)]
    assert p["span_rows"] == 1024 and p["words"] == 1876 and p["bytes"] == 1876 * 4 + 8 + 64 * 1024 * 4
    p = got[(320, 64, 64, 1, 64, 10, 80, 16, 320, 0, 0)]
    assert p["words"] == 10 and p["bytes"] == 40 + 8 + 64 * 256 * 4
    p = got[(1000003, 1024, 4400, 9, 128, 10, 10000, 32, 1000003, 0, 1)]
    assert p["words"] == 2 * 15626 and p["bytes"] == 31252 * 4 + 8 + 3 * 4400 * 256 * 4


def test_rule_matches_the_restatement_on_both_sides_of_its_boundary(lines):
    seen = set()
    for c, line in zip(CASES, lines):
        N, nlist, pspans, _, _, k, _, nprobe, n_allowed, force, _ = c
        p = json.loads(line)
        if not p["ok"]:                            # the unfiltered geometry declines: so does the filtered one, whatever the filter
            assert not p["filtered_ok"] and p["declines"] == -1, c
            continue
        est = nprobe * p["bins_per_span"] * pspans / nlist
        declines = n_allowed < N and min(est, nprobe * n_allowed / nlist) < 4 * k
        assert p["declines"] == int(declines), (c, p)
        assert p["filtered_ok"] == int(not declines or force == 2), (c, p)
        assert p["same"] == p["filtered_ok"], (c, p)            # where it serves, the geometry is the unfiltered one, field by field
        seen.add((bool(declines), force))
    assert {(True, 0), (False, 0), (True, 2), (False, 2)} <= seen
    got = {c: json.loads(line) for c, line in zip(CASES, lines)}
    # nprobe * n_allowed / nlist < 4 k, strictly: 8 * 320 / 64 = 40 = 4 k serves, 319 declines
    assert [got[BASE + (na, 0, na % 2)]["filtered_ok"] for na in (321, 320, 319)] == [1, 1, 0]
    assert [got[(20000, 64, 120, 3, 64, 1, 300, 8, na, 0, 0)]["filtered_ok"] for na in (33, 32, 31)] == [1, 1, 0]
    assert [got[(20000, 64, 120, 3, 64, 10, 300, 16, na, 0, 0)]["filtered_ok"] for na in (161, 160, 159)] == [1, 1, 0]
    assert [got[(1000003, 1024, 4400, 9, 128, 10, 10000, 32, na, 0, 1)]["filtered_ok"] for na in (1281, 1280, 1279)] == [1, 1, 0]
    # force_path 1 declines everything, as it does unfiltered
    assert all(not got[BASE + (na, 1, na % 2)]["ok"] for na in (20000, 200))


def test_every_row_admitted_is_the_unfiltered_geometry(lines):
    for c, line in zip(CASES, lines):
        if c[8] >= c[0]:
            p = json.loads(line)
            assert p["filtered_ok"] == p["ok"] and p["same"] == 1, (c, p)
    # 5 rows per list: 64 bins per query but only 80 rows probed -- a rule that ignored "every row admitted" could not tell
    p = json.loads(lines[CASES.index((320, 64, 64, 1, 64, 10, 80, 16, 320, 0, 0))])
    assert p["ok"] == 1 and p["filtered_ok"] == 1


def test_sanitized_build_prints_the_same(lines):
    prog = build("ivf_filter_plan_san")
    out = subprocess.run([str(prog)], input=TEXT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == lines

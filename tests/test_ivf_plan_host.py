"""The rules of an IVF search batch (csrc/ivf_plan.hpp) run as a host program: which path serves, geometry, capacities, launches.

tests/host/ivf_plan_main.cpp includes the header the library plans from and prints, per case, the geometry of the list-major MFMA scan
(or the split count of the exact list scan), the capacities of the work lists and of the select, and the fp16 / int8 / K-loop launch
with template arguments, grid, block and row parts.  No GPU, no HIP: built with the host compiler (`make ivf_plan`).

1. The census GPU tests (test_gpu_census_ivf.py, test_gpu_census_ivf_coded.py) name a launch shape by setting options and assert only
   that the list scan served.  Here every parametrised case of the two files is planned over the list sizes those files build --
   census.corpus, the oracle's assignment to the first 64 rows (the files' own centroids for SQ8, census_coded.ivf_lists for IVF-PQ),
   then `adjust` -- and must reach the shape its name and docstring claim.
2. The documented gates of ivf_geometry, restated below in `geometry`, over a matrix.
3. Invariants of every planned launch.
4. Every plan is a listed instantiation, and every listed instantiation is planned.

Where a GPU test's docstring and the C++ disagree, the C++ is pinned here and the GPU test is left as it is:
  * test_kloop_list_scan (`ivf_tps` 16 / 64 x `ivf_tile` 1 / 2 x `ivf_group` 1 / 2 / 4) names twelve shapes; there are seven.  On
    1024-row spans (`ivf_tps` 64) neither `ivf_tile` nor `ivf_group` is read: all six of those cases launch
    ivf_kloop_scan_kernel<64, 2, 4, 1> on 512 slots per item, with candidate groups of 4 rows.  The six cases at `ivf_tps` 16 reach
    <16, 2, group, tile> as named.
  * test_list_scan_parts: its claims hold (unit of 4 spans at the default bin size, so `ivf_part` 1 is the launch of 4; unit of 2 spans
    with `ivf_bt` 4, where `ivf_part` 1 gives parts of 2 spans and 4 parts of 4; one span at D = 200).  Only the long list's size is
    off: "about 1900 rows, 8 spans" is the IVF-PQ census (census_coded.ivf_lists); under `adjust` the IVF-Flat and SQ8 corpora give
    2294 to 2395 rows, 9 or 10 spans, so `ivf_part` 4 cuts it into 3 parts there, not 2.  It is cut in every case, as claimed.
"""
from __future__ import annotations

import itertools
import json
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import census
from tests import census_coded as cc
from tests.test_gpu_census_ivf import K, N, NLIST, NPROBE, SHAPES, adjust
from tests.test_gpu_census_ivf_coded import PQ, SQ8, sq8_inputs

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
PROGRAM = PKG / "build" / "ivf_plan"

MAX_ENTRIES, MAX_PROBES = 4096, 512       # kIvfMaxEntries, kIvfMaxProbes (ivf_plan.hpp)


def build():
    srcs = [ROOT / "tests" / "host" / "ivf_plan_main.cpp", PKG / "csrc" / "ivf_plan.hpp", PKG / "csrc" / "scan_plan.hpp"]
    if not PROGRAM.exists() or any(s.stat().st_mtime > PROGRAM.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", "ivf_plan"], check=True)
    return PROGRAM


def span_rows_of(n, nlist, d, opts):
    """ivf_build_panel_space: 256-row spans for D <= 128; above, 16 `ivf_tps` rows -- 64 tiles for lists of thousands of rows, else 16."""
    if d <= 128:
        return 256, 0
    tps = opts.get("ivf_tps", 0)
    if tps not in (16, 64):
        tps = 64 if n / nlist > 2048.0 else 16
    return 16 * tps, tps


class Case:
    """One line of the program's input, and what the test knows about it."""

    def __init__(self, sizes, d, k, nq, nprobe, i8_ok=0, codec=0, **opts):
        sizes = np.asarray(sizes, np.int64)
        self.n, self.nlist, self.d, self.k, self.nq, self.nprobe, self.opts = int(sizes.sum()), len(sizes), d, k, nq, nprobe, opts
        self.span, self.tps = span_rows_of(self.n, self.nlist, d, opts)
        spans = (sizes + self.span - 1) // self.span
        self.pspans, self.max_pspans = int(spans.sum()), int(spans.max())
        self.line = (f"{self.n} {self.nlist} {self.pspans} {self.max_pspans} {d} {k} {nq} {nprobe} i8_ok={i8_ok} codec={codec} "
                     + " ".join(f"{name}={v}" for name, v in opts.items()) + "\n")


def run(cases):
    out = subprocess.run([str(build())], input="".join(c.line for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    plans = [json.loads(line) for line in out]
    for c, p in zip(cases, plans):
        assert (p["span_rows"], p["tps"], p["tile16"]) == (c.span, c.tps, int(c.d > 128)), (c.line, p)
    return plans


@pytest.fixture(scope="module")
def keys():
    """{family: {targs}} of the three lists."""
    got = {}
    for line in subprocess.run([str(build()), "--keys"], capture_output=True, text=True, check=True).stdout.splitlines():
        j = json.loads(line)
        got[j["family"]] = {tuple(t) for t in j["keys"]}
        assert len(got[j["family"]]) == len(j["keys"]), "an instantiation is listed twice"
    assert {f: len(v) for f, v in got.items()} == {"scan_kernel": 12, "scan_i8_kernel": 48, "ivf_kloop_scan_kernel": 7}
    return got


# ---- 1. the census cases ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def census_sizes(oracle):
    """List sizes of a census index, by the key its file builds it under."""
    cache = {}

    def get(key):
        if key not in cache:
            if key[0] == "pq":
                lor = cc.ivf_lists()
            elif key[0] == "sq8":
                X, _, C, _, _ = sq8_inputs(key[1], key[2])
                lor = adjust(oracle.ivf_assign(C, X, key[3]))
            else:
                X = census.corpus(key[0], N, key[1], seed=5)
                lor = adjust(oracle.ivf_assign(X[:NLIST].copy(), X, key[2]))
            cache[key] = np.bincount(lor, minlength=NLIST)
            s = cache[key]
            assert (s[0], s[2], s[4], s[5], s[6]) == (0, 1, 255, 256, 257) and s[1] > 1500 and s.sum() == N
        return cache[key]

    return get


def census_case(sizes, key, nq, **opts):
    if key[0] in ("pq", "sq8"):
        return Case(sizes(key), key[1] if key[0] == "pq" else key[2], K, nq, NPROBE, codec=2 if key[0] == "pq" else 1, **opts)
    return Case(sizes(key), key[1], K, nq, NPROBE, i8_ok=int(key[0] == "bytes"), **opts)


def serves(p, c, i8):
    """The list scan serves: fp16 always, int8 beside it where the index has the copy (integer queries then take it: scan_dtype 1)."""
    assert p["ok"] and p["exact"] is None and not p["kloop"], (c.line, p)
    assert p["f16"]["listed"] and (p["i8"] is not None) == i8 == p["caps"]["use_i8"], (c.line, p)
    if i8:
        assert p["i8"]["listed"] and [p["i8"][x] for x in ("grid_x", "grid_y", "block", "part_spans")] == \
            [p["f16"][x] for x in ("grid_x", "grid_y", "block", "part_spans")], (c.line, p)


FLAT = list(SHAPES)
CODED_ALL = PQ + SQ8 + [("sq8", "bytes", 128, "l2"), ("sq8", "gauss", 64, "ip")]


def test_census_default_and_exact_cases(census_sizes):
    for key in FLAT + CODED_ALL:
        i8 = key[0] == "bytes"
        cases = [census_case(census_sizes, key, nq, ivf_min_batch=1) for nq in (40, 700)]
        for c, p in zip(cases, run(cases)):
            serves(p, c, i8)
    for key in FLAT + PQ + SQ8:        # `ivf_min_batch` above the batch: the exact list scan
        c = census_case(census_sizes, key, 700, ivf_min_batch=100_000)
        p, = run([c])
        assert not p["ok"] and 1 <= p["exact"]["S"] <= NPROBE, (c.line, p)


def test_census_waves_and_bins(census_sizes):
    for key in FLAT + PQ[1::2] + SQ8:
        for nw, bt in itertools.product((2, 4, 8), (4, 16)):
            c = census_case(census_sizes, key, 700, ivf_nw=nw, ivf_bt=bt, ivf_min_batch=1)
            p, = run([c])
            serves(p, c, key[0] == "bytes")
            ks = 4 if c.d <= 64 else 8
            assert p["f16"]["targs"] == [ks, nw, 2, 2, 4 if bt == 4 else 8, 1, 0] and p["f16"]["block"] == 64 * nw, (c.line, p)
            assert (p["nw"], p["bt"], p["bin_rows"]) == (nw, 4 if bt == 4 else 8, 64 if bt == 4 else 128), (c.line, p)
            if p["i8"]:
                assert p["i8"]["targs"][:6] == [ks // 2, 8 // (ks // 2), 2, nw, 4 if bt == 4 else 8, 1], (c.line, p)


def test_census_int8_rings_and_groups(census_sizes):
    for (d, metric), ring, group in itertools.product(((64, "ip"), (128, "l2")), (2, 4, 8), (4, 8)):
        c = census_case(census_sizes, ("bytes", d, metric), 700, i8_ring=ring, ivf_i8_group=group, ivf_min_batch=1)
        p, = run([c])
        serves(p, c, True)
        assert p["i8"]["targs"][6:] == ([8, 0, 4, 0] if group == 8 else [4, 0, ring, 0]), (c.line, p)


def test_census_parts(census_sizes):
    for key in FLAT + PQ[0::2] + SQ8:
        got = {}
        for part, bt in ((4, 0), (1, 4), (4, 4), (1, 0)):        # (1, 0): the launch the docstring says is no case of its own
            c = census_case(census_sizes, key, 700, ivf_bt=bt, ivf_part=part, ivf_min_batch=1)
            p, = run([c])
            serves(p, c, key[0] == "bytes")
            long_spans = -(-int(census_sizes(key)[1]) // 256)
            assert c.max_pspans == long_spans > 4 and p["bt"] == (4 if bt == 4 else 8), (c.line, p)      # (default bins: 128 rows)
            unit = 4 // p["bps"]
            assert unit == (2 if bt == 4 else 4), (c.line, p)
            assert p["f16"]["part_spans"] == (part + unit - 1) // unit * unit, (c.line, p)
            assert p["f16"]["grid_y"] == -(-long_spans // p["f16"]["part_spans"]) > 1, (c.line, p)
            got[(part, bt)] = p["f16"]
        assert got[(1, 0)] == got[(4, 0)] and got[(1, 4)]["part_spans"] == 2 and got[(4, 4)]["part_spans"] == 4
    for part in (1, 4):        # D = 200 on 256-row spans: a unit of one span
        c = Case(census_sizes(("gauss", 200, "l2")), 200, K, 700, NPROBE, ivf_tps=16, ivf_tile=0, ivf_group=0, ivf_part=part, ivf_min_batch=1)
        p, = run([c])
        assert p["ok"] and p["kloop"] and c.max_pspans > 4, (c.line, p)
        assert p["kloop_launch"]["part_spans"] == part and p["kloop_launch"]["grid_y"] == -(-c.max_pspans // part) > 1, (c.line, p)


def test_census_kloop_cases(census_sizes):
    for tps, tile, group in itertools.product((16, 64), (1, 2), (1, 2, 4)):
        key = ("gauss", 200, "l2") if tps == 16 else ("wide", 200, "ip")
        for nq in (700, 40) if (tile, group) == (1, 1) else (700,):
            c = Case(census_sizes(key), 200, K, nq, NPROBE, ivf_tps=tps, ivf_tile=tile, ivf_group=group, ivf_part=0, ivf_min_batch=1)
            p, = run([c])
            assert p["ok"] and p["kloop"] and p["kloop_launch"]["listed"] and p["kloop_launch"]["block"] == 512, (c.line, p)
            # (`ivf_tps` 64: neither option is read -- see the module docstring)
            want = [16, 2, group, tile] if tps == 16 else [64, 2, 4, 1]
            assert p["kloop_launch"]["targs"] == want and p["group"] == (256 if want[3] == 2 else 512), (c.line, p)
            assert p["caps"]["kgroup"] == want[2] and p["select"]["nm"] == 5 and p["bin_rows"] == 4 * tps, (c.line, p)


# ---- 2. the documented gates ---------------------------------------------------------------------------------------------------------
def geometry(c, force_path=0, ivf_min_batch=1, mfma_ok=1):
    """ivf_geometry restated: (ok, reason it is not, nw, group, unit of the row parts)."""
    if not mfma_ok or force_path in (1, 3) or c.nq < ivf_min_batch:
        return False, "gate", 0, 0, 0
    if c.k > 256:
        return False, "k", 0, 0, 0
    if c.nprobe > MAX_PROBES:
        return False, "nprobe", 0, 0, 0
    kloop = c.d > 128
    avg = c.pspans / c.nlist
    bt = 4 if c.nprobe * c.span / 128.0 * avg < 8.0 * c.k else 8
    bt = {4: 4, 16: 8}.get(c.opts.get("ivf_bt", 0), bt)
    bps = 8 // bt
    bins_per_span = 4 if kloop else 2 * bps
    est = c.nprobe * bins_per_span * avg
    if est < 4.0 * c.k:
        return False, "few", 0, 0, 0
    if est > 0.7 * MAX_ENTRIES:
        return False, "many", 0, 0, 0
    pairs = c.nq * c.nprobe
    per_list = pairs / c.nlist
    nw = min((2, 4, 8), key=lambda w: (math.ceil(per_list / (64.0 * w)) * 64.0 * w * {2: 1.10, 4: 1.05, 8: 1.0}[w], w))
    nw = c.opts.get("ivf_nw", 0) or nw
    if kloop:
        nw = 4 if c.tps == 16 and c.opts.get("ivf_tile", 0) == 2 else 8
    group = 64 * nw
    items = (pairs + group - 1) // group
    run_pad = 0 if kloop else 6
    max_bins = items * (bins_per_span * c.max_pspans + run_pad) + bins_per_span * c.pspans + run_pad * min(c.nlist, pairs)
    if max_bins * group * 4 > 3 << 30 or (items + min(c.nlist, pairs)) * group > 1 << 30:
        return False, "size", 0, 0, 0
    return True, "", nw, group, 1 if kloop else 4 // bps


MATRIX_NLIST = (64, 100, 1024, 4096, 16384)
MATRIX_ROWS = (20, 100, 300, 750, 2000, 5000)          # N / nlist; one list five times as long
MATRIX_D = (64, 128, 200, 384, 768)
MATRIX_K = (1, 2, 10, 64, 65, 256, 257)
MATRIX_NQ = (1, 63, 64, 65, 300, 10_000, 16_384)
MATRIX_NPROBE = (1, 8, 32, 128, 512, 513)


@pytest.fixture(scope="module")
def matrix():
    cases = []
    for nlist, rows in itertools.product(MATRIX_NLIST, MATRIX_ROWS):
        sizes = np.full(nlist, rows, np.int64)
        sizes[0] = 5 * rows
        for d, k, nq, nprobe in itertools.product(MATRIX_D, MATRIX_K, MATRIX_NQ, MATRIX_NPROBE):
            cases.append(Case(sizes, d, k, nq, min(nprobe, nlist), i8_ok=1))         # (a search clamps nprobe to nlist)
    return cases, run(cases)


def test_gates(matrix):
    why = {"": 0, "k": 0, "few": 0, "many": 0, "size": 0, "nprobe": 0}
    for c, p in zip(*matrix):
        ok, reason, nw, group, _ = geometry(c)
        assert p["ok"] == ok, (c.line, reason, p)
        why[reason] += 1
        if ok:
            assert (p["nw"], p["group"], p["kloop"]) == (nw, group, c.d > 128), (c.line, p)
            assert p["bin_bytes"] <= 3 << 30 and p["max_slots"] <= 1 << 30
    assert min(why[r] for r in ("", "k", "few", "many")) >= 300 and why["nprobe"] > 0, why
    # the gates the matrix leaves open
    sizes = np.full(1024, 977, np.int64)
    side = [(dict(force_path=fp, ivf_min_batch=mb, mfma_ok=m), Case(sizes, 128, 10, nq, 32, force_path=fp, ivf_min_batch=mb, mfma_ok=m))
            for fp, mb, m, nq in itertools.product((0, 1, 2, 3), (1, 64, 65), (0, 1), (1, 64, 300))]
    for (g, c), p in zip(side, run([c for _, c in side])):
        assert p["ok"] == geometry(c, **g)[0] == (g["mfma_ok"] == 1 and g["force_path"] in (0, 2) and c.nq >= g["ivf_min_batch"]), (c.line, p)
    # the data point of the cost model's comment: nlist 1024, 10 000 queries, nprobe 8 / 32 / 128 -> 2 / 2 / 4 waves
    cases = [Case(sizes, 128, 10, 10_000, nprobe) for nprobe in (8, 32, 128)]
    assert [p["ok"] and p["nw"] for p in run(cases)] == [2, 2, 4]


# ---- 3. invariants of every planned launch ---------------------------------------------------------------------------------------------
def select_lds_words(vals_entries, probe_cap, act_cap, nm):
    """ivf_select_lds_words (ivf_mfma.hpp:462): vals | p_off (+ 32) | p_base lo / hi | p_list (+ 32) | act | vals2."""
    return vals_entries + 4 * probe_cap + 64 + act_cap * (1 + nm)


def test_launch_invariants(matrix):
    planned = exact = 0
    for c, p in zip(*matrix):
        if not p["ok"]:
            assert 1 <= p["exact"]["S"] <= c.nprobe, (c.line, p)
            exact += 1
            continue
        unit = geometry(c)[4]
        assert p["max_slots"] == p["max_items"] * p["group"] and p["cnt_words"] == 2 * c.nlist + p["max_slots"] + c.nq, (c.line, p)
        s = p["select"]
        assert s["act_cap"] >= 64 and 2 * 4 * select_lds_words(s["vals_entries"], s["probe_cap"], s["act_cap"], s["nm"]) <= 64 << 10, (c.line, p)
        assert s["probe_cap"] >= c.nprobe and s["max_entries"] <= MAX_ENTRIES and s["nm"] == (5 if c.d > 128 else 3), (c.line, p)
        launches = [p["kloop_launch"]] if p["kloop"] else [p["f16"]] + ([p["i8"]] if p["i8"] else [])
        assert (p["f16"] is None and p["i8"] is None) if p["kloop"] else (p["kloop_launch"] is None and p["i8"] is not None), (c.line, p)
        for L in launches:
            assert L["listed"] and L["grid_x"] == p["max_items"] and L["block"] == (512 if p["kloop"] else 64 * p["nw"]), (c.line, p)
            if L["part_spans"] == 0:
                assert L["grid_y"] == 1, (c.line, p)
            else:
                assert L["part_spans"] % unit == 0 and L["part_spans"] < c.max_pspans, (c.line, p)
                assert L["grid_y"] == (c.max_pspans + L["part_spans"] - 1) // L["part_spans"] <= 64, (c.line, p)
        if len(launches) == 2:
            assert [launches[0][x] for x in ("grid_x", "grid_y", "block", "part_spans")] == \
                [launches[1][x] for x in ("grid_x", "grid_y", "block", "part_spans")], (c.line, p)
        planned += 1
    assert planned > 1000 and exact > 1000


# ---- 4. every plan is listed, every listed instantiation is planned ----------------------------------------------------------------------
def test_every_plan_is_listed_and_every_listed_kernel_is_planned(matrix, keys):
    produced = {f: set() for f in keys}

    def collect(cases, plans):
        for c, p in zip(cases, plans):
            for name in ("f16", "i8", "kloop_launch"):
                if p["ok"] and p[name]:
                    assert p[name]["listed"] and tuple(p[name]["targs"]) in keys[p[name]["family"]], (c.line, p)
                    produced[p[name]["family"]].add(tuple(p[name]["targs"]))

    collect(*matrix)
    # the tuning options, walked off default: 1024 lists of 977 rows (one of 4885), 300 queries, 32 probes
    sizes = np.full(1024, 977, np.int64)
    sizes[0] = 4885
    more = [Case(sizes, d, 10, 300, 32, i8_ok=1, ivf_nw=nw, ivf_bt=bt, i8_ring=ring, ivf_i8_group=grp)
            for d, nw, bt, ring, grp in itertools.product((64, 128), (0, 2, 4, 8), (0, 4, 16), (0, 2, 4, 8), (4, 8))]
    more += [Case(sizes, 200, 10, 300, 32, ivf_tps=tps, ivf_tile=tile, ivf_group=grp)
             for tps, tile, grp in itertools.product((16, 64), (0, 1, 2), (0, 1, 2, 4))]
    plans = run(more)
    assert all(p["ok"] for p in plans)
    collect(more, plans)
    assert produced == keys, {f: sorted(keys[f] - produced[f]) for f in keys}

"""The rules of the int8 range prefilter (csrc/range_plan.hpp: threshold, route, grid, LDS bytes) run as a host program.

tests/host/range_i8_plan_main.cpp prints range_i8_thr / range_i8_kq / range_i8_grid / range_i8_route / range_i8_lds_bytes; the
threshold is checked by brute force against the contract's rule over every (t', parity, Kq, radius) of a small window.  No GPU, no
HIP: built with the host compiler (`make range_i8_plan`) and once more with the address and undefined-behaviour sanitizers."""
from __future__ import annotations

import itertools
from fractions import Fraction
import json
import re
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
OFFSET, SPAN = 1000, 14                     # accumulators t' in [OFFSET - SPAN, OFFSET + SPAN]
KQS = (-7, -2, -1, 0, 1, 2, 9)
RADII = [float(r) / 2 for r in range(-12, 41)] + [0.25, 17.75, float("inf"), float("-inf"), FLT_MAX, -FLT_MAX, 1e-30, 3e9, -3e9]
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
SHAPES = [(1, 16421), (15, 16421), (130, 16421), (384, 16421), (512, 15500), (513, 15500), (1030, 16421), (2048, 1_000_000), (1, 1_000_000)]


def build(target):
    prog = PKG / "build" / target
    srcs = [ROOT / "tests" / "host" / "range_i8_plan_main.cpp", PKG / "csrc" / "range_plan.hpp"]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", target], check=True)
    return prog


def bits(r):
    return "%x" % struct.unpack("<I", struct.pack("<f", r))[0]


THR = list(itertools.product((0, 1), RADII, KQS))
KQ = [(m, q2, sq, d, cx, cq) for m in (0, 1) for (q2, sq, d) in ((0, 0, 1), (77, 11, 3), (255 * 255 * 128, 255 * 128, 128), (129, -15, 30))
      for cx, cq in ((128, 127), (0, -1), (128, -1))]
TEXT = ("".join(f"thr {m} {bits(r)} {kq} {OFFSET}\n" for m, r, kq in THR) + "".join("kq %d %d %d %d %d %d\n" % c for c in KQ) +
        "".join(f"grid {nq} {n}\n" for nq, n in SHAPES) + "".join("route %d %d %d %d %d\n" % c for c in itertools.product((0, 1), repeat=5)) +
        "lds 1\nlds 2\n")


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([str(build("range_i8_plan"))], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(THR) + len(KQ) + len(SHAPES) + 32 + 2
    return out


def test_threshold_against_the_rule_by_brute_force(lines):
    exact_ip = slack_l2 = 0
    for (metric, r, kq), line in zip(THR, lines):
        thr = int(line)
        assert INT_MIN <= thr <= INT_MAX
        for t, parity in itertools.product(range(OFFSET - SPAN, OFFSET + SPAN + 1), (0, 1)):
            key = 2 * (t - OFFSET) + parity + kq if metric == 0 else (t - OFFSET) + kq
            if metric == 0 and key < 0:
                continue                                            # (a squared distance is never negative)
            passes = bool(F32(key) < F32(r)) if metric == 0 else bool(F32(-key) > F32(r))
            what = (metric, r, kq, t, parity, thr)
            if passes:
                assert t <= thr, what                               # never loses a result
            elif t <= thr and metric == 1:
                raise AssertionError(("IP candidate that is no result", what))
            elif t <= thr:
                assert Fraction(r) <= key < Fraction(r) + 1, what   # L2: only the dropped parity bit
                slack_l2 += 1
            exact_ip += metric == 1 and passes
    assert exact_ip > 1000 and slack_l2 > 100
    by = {(m, r, kq): int(v) for (m, r, kq), v in zip(THR, lines)}
    for kq in KQS:                                                  # the clamps: nothing passes / every real row passes
        assert by[0, 0.0, kq] == by[0, -3.0, kq] == by[0, float("-inf"), kq] == by[1, float("inf"), kq] == INT_MIN
        assert by[0, float("inf"), kq] == by[0, FLT_MAX, kq] == by[1, float("-inf"), kq] == by[1, -FLT_MAX, kq] == INT_MAX
        assert by[1, FLT_MAX, kq] == INT_MIN and (1 << 30) < by[0, 3e9, kq] < INT_MAX == by[1, -3e9, kq]


def test_kq_terms(lines):
    for (m, q2, sq, d, cx, cq), line in zip(KQ, lines[len(THR):]):
        assert int(line) == (q2 - 2 * cx * sq + 2 * d * cx * cq if m == 0 else -cx * sq + d * cx * cq)


def test_route_grid_and_lds(lines):
    rest = lines[len(THR) + len(KQ):]
    for (nq, n), line in zip(SHAPES, rest):
        g = json.loads(line)
        words = (n + 1023) // 1024 * 32
        cb = 8 if nq > 512 else 4
        tile = 8 * 16 * cb
        spc = max(2, min(16, (words // 16) * -(-nq // tile) // 512))
        assert g == dict(cb=cb, spc=spc, chunks=-(-(words // 16) // spc), qtiles=-(-nq // tile), qpad=-(-nq // tile) * tile), (nq, n, g)
        assert g["chunks"] * g["spc"] * 512 >= n and g["qpad"] >= nq and g["chunks"] < 65536 and g["qtiles"] < 65536
    routes = rest[len(SHAPES):len(SHAPES) + 32]
    for c, line in zip(itertools.product((0, 1), repeat=5), routes):
        assert int(line) == int(all(c)), c
    assert [int(v) for v in rest[-2:]] == [2 * (8 * 2 * 64 * 16 + 1024), 2 * (8 * 4 * 64 * 16 + 1024)] == [34816, 67584]
    assert int(rest[-1]) <= 160 * 1024                               # the LDS of a CU (the VGPRs of the CB = 8 forms admit one workgroup per CU)


def test_sanitized_build_prints_the_same(lines):
    out = subprocess.run([str(build("range_i8_plan_san"))], input=TEXT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == lines


def test_option_is_listed_and_reaches_the_python_layer():
    header = (ROOT / "include" / "vdbhip.h").read_text()
    comment = re.search(r"/\* Options \(vdb_set_option;.*?\*/\nint vdb_set_option\(", header, re.S).group(0)
    assert '"range_i8"' in comment
    sys.path.insert(0, str(PKG))
    import inspect

    from vdbhip import algorithms, index
    assert list(inspect.signature(index.FlatIndex.set_option).parameters) == ["self", "key", "value"]   # any name goes through to the C ABI
    for cls in (algorithms.HipExactSearch, algorithms.HipLinearSearcher):
        assert "range_int8" in inspect.signature(cls.__init__).parameters, cls

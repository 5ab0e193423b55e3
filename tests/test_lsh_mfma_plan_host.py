"""The rules of the int8 MFMA Hamming scan (csrc/lsh_mfma_plan.hpp: K-steps, row tiles, query tile, LDS bytes, grid) run as a host
program, and the plugin parameter `mfma_scan` (option "lsh_mfma") against the fake library of the plugin contract tests.  No GPU,
no HIP: `make lsh_mfma_plan`."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_plugin_contract_host import H, fake  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
WPS = [1, 2, 4, 8, 16, 32]
SHAPES = [(1000, 37), (1000, 1), (33037, 5), (40000, 300), (300000, 37), (1, 1), (1 << 20, 10000)]      # (n, nq): the GPU test's, and the edges
CASES = [(wp, n, nq) for wp in WPS for n, nq in SHAPES]


@pytest.fixture(scope="module")
def plans():
    prog = PKG / "build" / "lsh_mfma_plan"
    srcs = [ROOT / "tests" / "host" / "lsh_mfma_plan_main.cpp", PKG / "csrc" / "lsh_mfma_plan.hpp"]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", "lsh_mfma_plan"], check=True)
    text = "".join("plan %d %d %d\n" % c for c in CASES)
    out = subprocess.run([str(prog)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    return [json.loads(line) for line in out]


def test_tiles_lds_and_grid_at_every_width(plans):
    for (wp, n, nq), r in zip(CASES, plans):
        assert r["ksteps"] == -(-wp // 2) and r["rt"] * r["ksteps"] <= 32, (wp, r)            # A fragments: at most 128 VGPRs
        assert r["lds_limit"] == 65 * 1024 and r["lds"] == r["qtile"] * (64 * r["ksteps"] + 4) <= r["lds_limit"], (wp, r)
        assert r["qtile"] % 16 == 0 and 16 <= r["qtile"] <= 64 * r["waves"], (wp, r)           # one thread per query stages its constant
        assert r["rows_pass"] == 16 * r["waves"] * r["rt"] and r["row_tile"] % r["rows_pass"] == 0, (wp, r)
        assert r["operand"] == -(-nq // 16) * 16 * 64 * r["ksteps"], (wp, nq, r)
        gx, gy = r["grid"]
        assert (gx - 1) * r["row_tile"] < n <= gx * r["row_tile"] and (gy - 1) * r["qtile"] < nq <= gy * r["qtile"], (wp, n, nq, r)
    assert [p["qtile"] for p in plans[::len(SHAPES)]] == [256, 256, 256, 256, 128, 64]


@pytest.mark.parametrize("value", [True, False, None])
def test_mfma_scan_sets_the_option_only_when_on(fake, value):  # noqa: F811
    import vdbhip.lsh as lsh

    d = 16
    x = np.random.default_rng(0).standard_normal((600, d)).astype(np.float32)
    want = [(H, b"lsh_mfma", 1.0)] if value else []
    art = lsh.HipLSHIndexer("ix", d, "l2", num_bits=64, mfma_scan=value).build(x)
    names = fake.names()
    assert fake.calls("vdb_set_option") == want and (not value or names.index("vdb_set_option") < names.index("vdb_lsh_set_projection")), names
    fake.clear()
    lsh.HipLSHSearcher("s", d, "l2", mfma_scan=value, reserve_queries=0).attach(art, x)
    assert fake.calls("vdb_set_option") == want

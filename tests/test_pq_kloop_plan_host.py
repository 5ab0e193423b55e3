"""The rules of the flat PQ K-loop scan of the product codes (csrc/pq_kloop_plan.hpp: which batches it serves, code pitch, ring depth,
LDS bytes, the narrow rule, the launch) run as a host program; the padded table and operand order restated in NumPy; and the plugin
parameter `direct_kloop` (option "pq_kloop") against the fake library of the plugin contract tests.  No GPU, no HIP:
`make pq_kloop_plan`."""
from __future__ import annotations

import itertools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_plugin_contract_host import H, fake  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
# option, pq, D, M, scan path, direct rows, adc, filtered: the truth table at 192 / 24, then the edges of D, M and Kp
SERVES = [(o, p, 192, 24, s, r, a, f) for o, p, s, r, a, f in itertools.product((0, 1), (0, 1), (0, 1), (0, 128), (0, 1), (0, 1))] + \
         [(1, 1, d, m, 1, 0, 0, 0) for d, m in ((128, 16), (129, 43), (768, 64), (512, 256), (514, 257), (4096, 256), (4080, 240), (4104, 8), (192, 16))]
LDS = [1, 8, 64, 65, 128, 256]
PLANS = [(m, nq, sb, qg) for m in (24, 64, 65, 256) for nq, sb, qg in ((1, 1, 0), (17, 1, 0), (63, 1, 0), (63, 0, 0), (64, 1, 0), (600, 1, 0), (10000, 1, 3))]
SPACES = [(24, 8), (16, 12), (22, 6), (8, 17), (65, 3), (64, 12)]                        # (M, dsub): the shapes of the GPU test
TEXT = ("".join("serves %d %d %d %d %d %d %d %d\n" % c for c in SERVES) + "".join("lds %d\n" % m for m in LDS) +
        "".join("plan %d %d %d %d\n" % c for c in PLANS) + "".join("space %d %d\n" % c for c in SPACES))


@pytest.fixture(scope="module")
def lines():
    prog = PKG / "build" / "pq_kloop_plan"
    srcs = [ROOT / "tests" / "host" / "pq_kloop_plan_main.cpp"] + [PKG / "csrc" / n for n in ("pq_kloop_plan.hpp", "ivf_pq_kloop_plan.hpp", "ivf_plan.hpp", "scan_plan.hpp")]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", "pq_kloop_plan"], check=True)
    out = subprocess.run([str(prog)], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(SERVES) + len(LDS) + len(PLANS) + len(SPACES)
    return out


def test_serve_rule_over_its_truth_table_and_the_edges_of_d_m_and_kp(lines):
    for c, line in zip(SERVES, lines):
        o, p, d, m, s, r, a, f = c
        dsub = d // m
        want = o == 1 and p == 1 and d > 128 and s == 1 and r == 0 and not a and not f and m <= 256 and m * 8 * -(-dsub // 8) <= 4096
        assert int(line) == int(want), c


def test_code_pitch_ring_depth_and_lds_bytes(lines):
    for m, line in zip(LDS, lines[len(SERVES):]):
        r = json.loads(line)
        cp = 64 if m <= 64 else 256
        assert (r["cp"], r["bs"]) == (cp, 2) and cp >= m and r["lds"] == 4 * 16384 + 2 * 128 * cp <= 160 * 1024, (m, r)
        assert r["wgs"] == (2 if m <= 64 else 1) and r["wgs"] * r["lds"] <= 160 * 1024 and (r["wgs"] < 2 or r["lds"] <= 80 * 1024), (m, r)


def test_every_plan_is_the_flat_kloop_launch_with_the_narrow_rule_and_an_instantiated_kernel(lines):
    for (m, nq, sb, qg), line in zip(PLANS, lines[len(SERVES) + len(LDS):]):
        r = json.loads(line)
        narrow = int(nq < 64 and sb == 1)
        assert r["family"] == "pq_kloop_scan_kernel" and r["targs"] == [2, narrow, 64 if m <= 64 else 256] and r["listed"], (m, nq, r)
        assert [r["grid"], r["block"], r["nqtiles"], r["qgroup"]] == r["f16"] and r["block"] == 512 and r["nqtiles"] == -(-nq // 512), (m, nq, r)


def test_padded_table_and_operand_order_reproduce_the_dot_product_exactly(lines):
    rng = np.random.default_rng(0)
    for (m, dsub), line in zip(SPACES, lines[len(SERVES) + len(LDS) + len(PLANS):]):
        r = json.loads(line)
        P, dim = 8 * -(-dsub // 8), np.array(r["dim"])
        assert (r["P"], r["Kp"], r["nk"]) == (P, m * P, -(-m * P // 64)) and sorted(dim[dim >= 0]) == list(range(m * dsub))
        tab = rng.integers(-64, 64, (m, 256, dsub)).astype(np.float16)       # small integers: every product and sum below is exact
        q = rng.integers(-64, 64, m * dsub).astype(np.float16)
        code = rng.integers(0, 256, m)
        T = np.zeros((m, 256, P), np.float16)
        T[:, :, :dsub] = tab                                                 # the padded table: a copy, zero beyond dsub
        B = np.where(dim >= 0, q[np.maximum(dim, 0)], np.float16(0))         # the operand row: zero where there is no dimension
        A = np.zeros(64 * r["nk"], np.float16)
        A[:m * P] = T[np.arange(m), code].ravel()                            # pieces behind Kp: any table piece against B = 0
        A[m * P:] = T[0, 0, 0]
        xhat = tab[np.arange(m), code].ravel()
        assert float(A.astype(np.float64) @ B.astype(np.float64)) == float(xhat.astype(np.float64) @ q.astype(np.float64))


@pytest.mark.parametrize("value", [True, False, None])
def test_direct_kloop_sets_the_option_only_when_on(fake, value):  # noqa: F811
    import vdbhip.pq as pq

    d = 16
    x = np.random.default_rng(0).standard_normal((600, d)).astype(np.float32)
    want = [(H, b"pq_kloop", 1.0)] if value else []
    pq.PQIndex(d, 4, "l2", 0, direct_kloop=value)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    pq.HipPQSearch("a", d, "PQ4", "l2", direct_kloop=value).build_index(x)
    names = fake.names()
    assert fake.calls("vdb_set_option") == want and (not value or names.index("vdb_set_option") < names.index("vdb_pq_add")), names
    fake.clear()
    art = pq.HipPQIndexer("ix", d, "l2", index_key="PQ4").build(x)
    assert fake.calls("vdb_set_option") == []
    s = pq.HipPQSearcher("s", d, "l2", direct_kloop=value)
    s.attach(art, x)
    assert fake.calls("vdb_set_option") == want

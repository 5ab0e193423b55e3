"""The rules of the IVF-PQ K-loop scan of the product codes (csrc/ivf_pq_kloop_plan.hpp: which adds build its bookkeeping, which batches
it serves, the padded operand space, the launch and its LDS bytes) run as a host program, and the plugin parameter `direct_kloop`
(option "ivf_pq_kloop") against the fake library of the plugin contract tests.  No GPU, no HIP: `make ivf_pq_kloop_plan`."""
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
# option, codec, D, M: both sides of D = 128 and D = 4096; M = 256 / 257; Kp = 4080 at dsub 17 -> P 24 -> 5760 > 4096 (refused)
BUILDS = list(itertools.product((0, 1), (0, 1, 2, 3), (128, 192), (16,))) + [(1, 2, d, m) for d, m in
          ((4096, 256), (4104, 8), (768, 64), (384, 64), (136, 8), (512, 256), (514, 257), (4080, 240), (4096, 512))]
SERVES = list(itertools.product((0, 1), (0, 1, 2, 3), (0, 1), (0, 1), (0, 1)))          # option, codec, built, K-loop geometry, filtered
SPACES = [(24, 8), (16, 12), (22, 6), (8, 17), (64, 12)]                                 # (M, dsub): the shapes of the GPU test
PLANS = [(m, tps, kg) for m in (8, 64, 65, 256) for tps, kg in ((16, 1), (16, 2), (16, 4), (64, 4))]
TEXT = ("".join("builds %d %d %d %d\n" % c for c in BUILDS) + "".join("serves %d %d %d %d %d\n" % c for c in SERVES) +
        "".join("space %d %d\n" % c for c in SPACES) + "".join("plan %d %d %d\n" % c for c in PLANS))


@pytest.fixture(scope="module")
def lines():
    prog = PKG / "build" / "ivf_pq_kloop_plan"
    srcs = [ROOT / "tests" / "host" / "ivf_pq_kloop_plan_main.cpp"] + [PKG / "csrc" / n for n in ("ivf_pq_kloop_plan.hpp", "ivf_plan.hpp", "scan_plan.hpp")]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", "ivf_pq_kloop_plan"], check=True)
    out = subprocess.run([str(prog)], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(BUILDS) + len(SERVES) + len(SPACES) + len(PLANS)
    return out


def test_builds_and_serves_over_their_truth_tables(lines):
    for (opt, codec, d, m), line in zip(BUILDS, lines):
        dsub = d // m
        want = opt == 1 and codec == 2 and 128 < d <= 4096 and m <= 256 and m * 8 * -(-dsub // 8) <= 4096
        assert int(line) == int(want), (opt, codec, d, m)
    for c, line in zip(SERVES, lines[len(BUILDS):]):
        opt, codec, built, geom, filtered = c
        assert int(line) == int(opt == 1 and codec == 2 and built == 1 and geom == 1 and not filtered), c


def test_operand_map_is_a_bijection_onto_the_non_zero_positions(lines):
    for (m, dsub), line in zip(SPACES, lines[len(BUILDS) + len(SERVES):]):
        r = json.loads(line)
        P = 8 * -(-dsub // 8)
        assert (r["P"], r["Kp"], r["nk"]) == (P, m * P, -(-m * P // 64)) and len(r["dim"]) == 64 * r["nk"]
        dim = np.array(r["dim"])
        pos = np.flatnonzero(dim >= 0)
        assert sorted(dim[pos]) == list(range(m * dsub))                                  # every dimension exactly once
        assert np.array_equal(pos, [s * P + j for s in range(m) for j in range(dsub)])   # ... inside its own sub-space, below Kp


def test_every_plan_names_an_instantiated_kernel_within_its_lds_budget(lines):
    for (m, tps, kg), line in zip(PLANS, lines[len(BUILDS) + len(SERVES) + len(SPACES):]):
        r = json.loads(line)
        cp, bs = (64, 2) if m <= 64 else (256, 1)
        assert r["family"] == "ivf_pq_kloop_scan_kernel" and r["targs"] == [tps, bs, kg, cp] and r["block"] == 512 and r["listed"], (m, r)
        assert r["lds"] == 2 * bs * 16384 + 8 * 5 * 4 * 64 * 4 + 2 * 128 * cp <= r["budget"] == 160 * 1024 and cp >= m, (m, r)


@pytest.mark.parametrize("value", [True, False])
def test_direct_kloop_of_the_plugin_classes_reaches_set_option_before_the_add(fake, value):  # noqa: F811
    import vdbhip.ivf_pq as ivf_pq

    d = 16
    x = np.random.default_rng(0).standard_normal((600, d)).astype(np.float32)
    want = [(H, b"ivf_pq_kloop", float(value))]

    def set_before_add():
        names = fake.names()
        return fake.calls("vdb_set_option") == want and names.index("vdb_set_option") < min(i for i, n in enumerate(names) if n.startswith("vdb_ivf_add"))

    ivf_pq.HipIVFPQIndexer("ix", d, "l2", index_key="IVF4,PQ4", direct_kloop=value).build(x)
    assert set_before_add(), fake.names()
    fake.clear()
    ivf_pq.HipIVFPQSearch("a", d, "IVF4,PQ4", "l2", direct_kloop=value).build_index(x)
    assert set_before_add(), fake.names()
    fake.clear()
    ivf_pq.IVFPQIndex(d, 4, 4, "l2", 0, direct_kloop=value)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    ivf_pq.HipIVFPQIndexer("ix", d, "l2", index_key="IVF4,PQ4").build(x)          # not given: the option is never touched
    assert fake.calls("vdb_set_option") == []

"""The rules of the direct IVF-PQ list scan (csrc/ivf_pq_direct_plan.hpp: which batches it serves, the LDS bytes by (D, M, KSTEPS), the
launch) run as a host program, and the plugin parameter `direct_codes` against a fake library.  No GPU, no HIP: `make ivf_pqd_plan`, and
once more with the address and undefined-behaviour sanitizers."""
from __future__ import annotations

import itertools
import json
import subprocess
from pathlib import Path

import pytest

from tests.test_plugin_contract_host import DIM, H, X, fake  # noqa: F401  (the fake library of the plugin contract tests)

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
SERVE = list(itertools.product((0, 1), (0, 1, 2, 3), (0, 1), (0, 1), (0, 1)))       # option, codec, geometry ok, kloop, filtered
LDS = [(128, 64, 8), (128, 16, 8), (128, 128, 8), (64, 64, 4), (64, 16, 4), (48, 8, 4), (50, 10, 4), (66, 22, 8), (15, 3, 4)]     # D, M, ksteps
PLANS = [(1_000_000, 1024, 4500, 12, d, 10, nq, nprobe, nw, bt, part) for d in (64, 128) for nq, nprobe in ((10_000, 8), (10_000, 128), (64, 32))
         for nw in (0, 2, 4, 8) for bt in (0, 4, 16) for part in (0, 1)]
KEYS = [[ks, nw, bt] for ks in (4, 8) for nw in (2, 4, 8) for bt in (4, 8)]
TEXT = ("".join("serve %d %d %d %d %d\n" % c for c in SERVE) + "".join("lds %d %d %d\n" % c for c in LDS) +
        "".join("plan " + " ".join(map(str, c)) + "\n" for c in PLANS) + "keys\n")


def build(target):
    prog = PKG / "build" / target
    srcs = [ROOT / "tests" / "host" / "ivf_pqd_plan_main.cpp"] + [PKG / "csrc" / n for n in ("ivf_pq_direct_plan.hpp", "ivf_plan.hpp", "scan_plan.hpp")]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", target], check=True)
    return prog


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([str(build("ivf_pqd_plan"))], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(SERVE) + len(LDS) + len(PLANS) + 1
    return out


def test_serve_rule_over_its_truth_table(lines):
    for c, line in zip(SERVE, lines):
        opt, codec, ok, kloop, filtered = c
        assert int(line) == int(opt == 1 and codec == 2 and ok == 1 and not kloop and not filtered), c


def test_lds_bytes_hold_table_stages_codes_and_bias_within_a_cu(lines):
    for (d, m, ks), line in zip(LDS, lines[len(SERVE):]):
        r = json.loads(line)
        assert r["pitch"] >= m and r["pitch"] % 4 == 0 and (r["pitch"] // 4) % 2 == 1 and r["pitch"] <= m + 7, (m, r)     # whole rows, an odd number of dwords
        assert r["table"] >= 512 * d and r["table"] % 1024 == 0 and r["table"] < 512 * d + 1024, (d, r)                   # whole 1-KiB pieces
        assert r["stage"] == 2 * ks * 1024 and r["codes"] == 64 * r["pitch"], r
        assert r["total"] == r["table"] + 2 * r["stage"] + 2 * r["codes"] + 512 <= 160 * 1024, r
        assert r["wgs"] == 160 * 1024 // r["total"] >= 1, r
        assert (d, m) not in ((128, 64), (64, 16)) or r["wgs"] == (1 if d == 128 else 3), r      # the occupancies DESIGN 4.4 quotes


def test_every_plan_names_an_instantiated_kernel_on_the_fp16_grid(lines):
    assert json.loads(lines[-1]) == KEYS
    seen = set()
    for c, line in zip(PLANS, lines[len(SERVE) + len(LDS):]):
        r = json.loads(line)
        assert r["ok"] and r["family"] == "ivf_pq_scan_kernel" and r["listed"] and r["targs"] in KEYS, (c, r)
        assert r["targs"] == r["f16_targs"] and r["grid"] == r["f16_grid"] and r["part_spans"][0] == r["part_spans"][1], (c, r)
        seen.add(tuple(r["targs"]))
    assert seen == {tuple(k) for k in KEYS}                  # ... and every instantiation is one some plan reaches


def test_sanitized_build_prints_the_same(lines):
    out = subprocess.run([str(build("ivf_pqd_plan_san"))], input=TEXT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == lines


@pytest.mark.parametrize("value", [True, False])
def test_direct_codes_of_the_plugin_classes_reaches_set_option(fake, value):  # noqa: F811
    import vdbhip.ivf as ivf
    import vdbhip.ivf_pq as ivf_pq

    want = [(H, b"ivf_pq_direct", float(value))]
    art = ivf_pq.HipIVFPQIndexer("ix", DIM, "l2", index_key="IVF4,PQ4", direct_codes=value).build(X)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    s = ivf.HipIVFSearcher("s", DIM, "l2", direct_codes=value)
    s.attach(art, X)
    assert fake.calls("vdb_set_option") == want           # (an IVF-PQ artifact: the option of its own direct scan, not the SQ8 one)
    fake.clear()
    ivf_pq.HipIVFPQSearch("a", DIM, "IVF4,PQ4", "l2", direct_codes=value).build_index(X)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    ivf_pq.IVFPQIndex(DIM, 4, 4, "l2", 0, direct_codes=value)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    ivf_pq.HipIVFPQIndexer("ix", DIM, "l2", index_key="IVF4,PQ4").build(X)          # not given: the option is never touched
    assert fake.calls("vdb_set_option") == []

"""The rules of the int8 K-loop list scan (csrc/ivf_i8k_plan.hpp: build rule, launch rule, launch) run as a host program, and the
plugin parameter `int8_kloop` of the IVF classes against a fake library.  No GPU, no HIP: `make ivf_i8k_plan`, and once more with the
address and undefined-behaviour sanitizers."""
from __future__ import annotations

import itertools
import json
import subprocess
from pathlib import Path

import pytest

from tests.test_plugin_contract_host import DIM, H, X, fake  # noqa: F401  (the fake library of the plugin contract tests)

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
BUILD = list(itertools.product((0, 1), (0, 1, 2, 3), (0, 1), (0, 1), (384, 4096, 4097)))      # option, codec, tile16, byte-valued, dim
SERVE = list(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1)))                    # copy, panel_dtype, ivf_tile, filtered, list-major
# N nlist pspans max_pspans d k nq nprobe | ivf_tps ivf_group ivf_part: the msmarco shape and a long-list shape, every span size the
# build can choose, every candidate group, whole lists and row parts
PLANS = [(100_000, 100, 440, 8, 384, 20, 10_000, 32, tps, grp, part) for tps in (0, 16) for grp in (0, 1, 2, 4) for part in (0, 1)] + \
        [(1_000_000, 256, 1100, 9, 768, 10, 10_000, 8, tps, grp, part) for tps in (0, 64) for grp in (0, 1, 2, 4) for part in (0, 2)]
KEYS = [[16, 2, 1], [16, 2, 2], [16, 2, 4], [64, 2, 4]]
TEXT = ("".join("build %d %d %d %d %d\n" % c for c in BUILD) + "".join("serve %d %d %d %d %d\n" % c for c in SERVE) +
        "".join("plan " + " ".join(map(str, c)) + "\n" for c in PLANS) + "keys\n")


def build(target):
    prog = PKG / "build" / target
    srcs = [ROOT / "tests" / "host" / "ivf_i8k_plan_main.cpp"] + [PKG / "csrc" / n for n in ("ivf_i8k_plan.hpp", "i8k_plan.hpp", "ivf_plan.hpp", "scan_plan.hpp")]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", target], check=True)
    return prog


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([str(build("ivf_i8k_plan"))], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(BUILD) + len(SERVE) + len(PLANS) + 1
    return out


def test_build_and_launch_rules_over_their_truth_tables(lines):
    for c, line in zip(BUILD, lines):
        opt, codec, tile16, byte_valued, dim = c
        assert int(line) == int(opt == 1 and codec == 0 and tile16 == 1 and byte_valued == 1 and dim <= 4096), c
    for c, line in zip(SERVE, lines[len(BUILD):]):
        has, panel_dtype, tile, filtered, list_major = c
        assert int(line) == int(has == 1 and panel_dtype == 0 and tile != 2 and not filtered and list_major == 1), c


def test_every_plan_names_an_instantiated_kernel_on_the_fp16_grid(lines):
    assert json.loads(lines[-1]) == KEYS
    seen = set()
    for c, line in zip(PLANS, lines[len(BUILD) + len(SERVE):]):
        r = json.loads(line)
        assert r["ok"] and r["family"] == "ivf_kloop_i8_scan_kernel" and r["listed"] and r["targs"] in KEYS, (c, r)
        tps = r["targs"][0]
        assert r["targs"] == [tps, 2, r["kgroup"] if tps == 16 else 4] and r["grid"] == r["f16_grid"] and r["grid"][2] == 512, (c, r)
        assert c[8] in (0, tps) and (tps == 64 or c[9] in (0, r["kgroup"])), (c, r)
        seen.add(tuple(r["targs"]))
    assert seen == {tuple(k) for k in KEYS}                  # ... and every instantiation is one some plan reaches


def test_sanitized_build_prints_the_same(lines):
    out = subprocess.run([str(build("ivf_i8k_plan_san"))], input=TEXT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == lines


@pytest.mark.parametrize("value", [True, False])
def test_int8_kloop_of_the_plugin_classes_reaches_set_option_before_the_add(fake, value):  # noqa: F811
    import vdbhip.ivf as ivf

    want = [(H, b"ivf_i8_kloop", float(value))]
    art = ivf.HipIVFIndexer("ix", DIM, "l2", index_key="IVF4,Flat", int8_kloop=value).build(X)
    assert fake.calls("vdb_set_option") == want and fake.names().index("vdb_set_option") < fake.names().index("vdb_ivf_add")
    fake.clear()
    s = ivf.HipIVFSearcher("s", DIM, "l2", int8_kloop=value)
    s.attach(art, X)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    algo = ivf.HipApproximateSearch("a", DIM, "IVF4,Flat", "l2", int8_kloop=value)
    algo.build_index(X)
    assert fake.calls("vdb_set_option") == want and fake.names().index("vdb_set_option") < fake.names().index("vdb_ivf_add")
    fake.clear()
    ivf.HipIVFIndexer("ix", DIM, "l2", index_key="IVF4,Flat").build(X)         # not given: the option is never touched
    assert fake.calls("vdb_set_option") == []

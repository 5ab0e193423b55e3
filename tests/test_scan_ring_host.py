"""The stage ring of the int8 x16 batch loop (csrc/scan_ring.hpp) walked on the host.

tests/host/scan_ring_main.cpp includes the header the kernel takes its ring decisions from and prints, for 1 to 12 stages, what a
computing wave and a fully padded wave do: LDS-DMA issues, LDS reads, barriers.  A wrong ring is a race or a hang on the GPU, not a
wrong number, so the rules are asserted here.  No GPU, no HIP: the program is built with the host compiler (`make scan_ring`), and
once more with the address and undefined-behaviour sanitizers (`make scan_ring_san`); both builds must print the same lines.

The model: the waves of a workgroup agree only at barriers.  Interval b is the code between barrier b - 1 and barrier b (interval -1
is the prologue); two waves inside the same interval may be anywhere in it.  A barrier comes behind a full wait of every wave on its
own memory operations, so what was issued in interval b is in LDS for every wave from interval b + 1 on, and no earlier."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"
RING = 3


def build(target):
    prog = PKG / "build" / target
    srcs = [ROOT / "tests" / "host" / "scan_ring_main.cpp", PKG / "csrc" / "scan_ring.hpp"]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", target], check=True)
    return prog


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([str(build("scan_ring"))], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 13
    return out


def intervals(events):
    """-> (issues [(interval, stage, buffer)], reads [(interval, stage, buffer)], barriers [id])"""
    cur, issues, reads, bars = -1, [], [], []
    for e in events:
        if e[0] == "B":
            assert e[1] == cur, "barriers are numbered in order, the prologue's is -1"
            bars.append(e[1])
            cur += 1
        else:
            (issues if e[0] == "I" else reads).append((cur, e[1], e[2]))
    return issues, reads, bars


def test_ring_is_race_free_and_complete(lines):
    for n, line in zip(range(1, 13), lines):
        w = json.loads(line)
        assert w["nstages"] == n and w["ring"] == RING
        issues, reads, bars = intervals(w["computing"])
        # one barrier per stage and the prologue's
        assert bars == list(range(-1, n)) and w["barriers"] == n + 1
        # every stage's data is issued exactly once, into buffer stage % RING
        assert sorted(s for _, s, _ in issues) == list(range(n))
        assert all(b == s % RING for _, s, b in issues + reads)
        issued_in = {s: i for i, s, _ in issues}
        # every stage is read, and only in its own interval or (tile 0, read ahead) in the one before
        assert {s for _, s, _ in reads} == set(range(n))
        assert all(i in (s, s - 1) for i, s, _ in reads)
        assert all(any(i == s - 1 for i, s2, _ in reads if s2 == s) for s in range(1, n)), "tile 0 of stages >= 1 is read ahead"
        # every buffer read was certified by an earlier barrier: the issue lies in an earlier interval, and the header names the
        # barrier that closed it
        for i, s, _ in reads:
            assert issued_in[s] < i, (n, "stage", s, "read in interval", i, "issued in", issued_in[s])
        assert w["certifier"] == [issued_in[s] for s in range(n)]
        # no buffer is issued into while a stage that reads it is unfinished: the buffer's previous stage is read only in
        # earlier intervals (any wave may still be anywhere inside the issuing wave's own interval)
        for i, s, b in issues:
            assert all(ri < i for ri, rs, rb in reads if rb == b and rs < s), (n, "issue of stage", s, "in interval", i)
            assert all(ri > i for ri, rs, rb in reads if rb == b and rs == s)
        # a wave's pieces are a whole stage old at the barrier that waits for them, the prologue's apart
        assert all(i == -1 or i == s - (RING - 1) for i, s, _ in issues)


def test_padded_wave_takes_the_same_barriers_and_issues_the_same_pieces(lines):
    for line in lines[:12]:
        w = json.loads(line)
        ci, _, cb = intervals(w["computing"])
        pi, pr, pb = intervals(w["padded"])
        assert pb == cb and pi == ci and pr == []


def test_lds_bytes(lines):
    forms = json.loads(lines[12])["forms"]
    assert len(forms) == 2 * 2 * 2 * 4 * 3
    nbatch = 0
    for f in forms:
        stage = f["st"] * 2 * f["ks2"] * 1024 + f["st"] * 32 * 4
        batch = f["nwaves"] == 8 and f["ring"] == 2 and f["st"] * f["cb"] > 16
        assert f["stage_bytes"] == stage and f["batch"] == int(batch)
        # the batch forms hold RING stages, every other form what its plan key says -- as before the ring
        assert f["buffers"] == (RING if batch else f["ring"]) and f["lds_bytes"] == f["buffers"] * stage
        nbatch += batch
    assert nbatch == 6
    by = {(f["ks2"], f["st"], f["cb"], f["nwaves"], f["ring"]): f["lds_bytes"] for f in forms}
    assert by[(2, 8, 8, 8, 2)] == 3 * 33792 == 101376 and by[(1, 8, 8, 8, 2)] == 3 * 17408
    assert by[(2, 4, 4, 4, 2)] == 2 * 16896 and by[(2, 4, 4, 1, 8)] == 8 * 16896


def test_sanitized_build_prints_the_same(lines):
    out = subprocess.run([str(build("scan_ring_san"))], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == lines

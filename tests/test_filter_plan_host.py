"""The routing and sizing rules of a filtered search (csrc/filter_plan.hpp) run as a host program, against a restatement in Python.

tests/host/filter_plan_main.cpp includes the header the library routes a filtered call by -- sparse route or masked scan, whether the
list of admitted rows is kept at install, the splits of the sparse kernel, the bytes an install adds -- and prints them per case.  No
GPU, no HIP: the program is built with the host compiler (`make filter_plan`), and once more with the address and undefined-behaviour
sanitizers (`make filter_plan_san`); both builds must print the same lines."""
from __future__ import annotations

import itertools
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectordb-retrieval_amd"

QB, SPLIT_ROWS, MAX_SPLITS, PARTIAL_BYTES, MAX_K, DEFAULT_PAIRS = 4, 128, 1024, 256 << 20, 2048, 1 << 13

NQS = (1, 3, 7, 8, 64, 513, 10_000, 3_000_000)
KS = (1, 10, 100, 128, 129, 1024, 2048)
ALLOWED = (0, 1, 63, 64, 65, 83, 84, 85, 263, 264, 265, 4159, 4160, 4161, 5000, 65_536, 1_000_000, 12_500_000)
PAIRS = (0, 1, 64_000, DEFAULT_PAIRS, 9_000_000_000_000_000_000)
FORCE = (0, 1, 2, 3)


def few(k):
    return 2 * k + 64


def route_sparse(nq, k, n, pairs, force):
    return force == 0 and (n < few(k) or nq * n < pairs)


def keeps_list(n, pairs):
    return n < max(few(MAX_K), pairs)


def blocked(nq, k):
    return k <= 128 and nq >= 2 * QB


def splits(nq, k, n):
    groups = (nq + QB - 1) // QB if blocked(nq, k) else nq
    s = min((4096 + groups - 1) // groups, n // SPLIT_ROWS, MAX_SPLITS, PARTIAL_BYTES // (nq * k * 16))
    return max(1, s)


def per_split(n, s):
    return max(64, ((n + s - 1) // s + 63) // 64 * 64)


def mask(w, n):
    left = n - w * 32
    return 0xFFFFFFFF if left >= 32 else 0 if left <= 0 else (1 << left) - 1


def n_rows(n_allowed):
    return max(n_allowed, 1) + (n_allowed * 7) % 1000


def build(target):
    prog = PKG / "build" / target
    srcs = [ROOT / "tests" / "host" / "filter_plan_main.cpp", PKG / "csrc" / "filter_plan.hpp", PKG / "csrc" / "range_plan.hpp"]
    if not prog.exists() or any(s.stat().st_mtime > prog.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(PKG), "-s", target], check=True)
    return prog


CASES = [(nq, k, n, p, f, n_rows(n)) for nq, k, n, p, f in itertools.product(NQS, KS, ALLOWED, PAIRS, FORCE)]
# the pair rule on, one below and one above nq * n_allowed == sparse_pairs; the row rule on and around 2 k + 64
BOUNDARY = [(nq, 10, n, nq * n + dp, 0, n_rows(n)) for nq, n in ((64, 1000), (1, 5000), (10_000, 100), (7, 4161)) for dp in (-1, 0, 1)]
BOUNDARY += [(1, k, 2 * k + 64 + dn, 0, 0, n_rows(2 * k + 64 + dn)) for k in KS for dn in (-1, 0, 1)]
CASES += BOUNDARY
TEXT = "".join(" ".join(map(str, c)) + "\n" for c in CASES)


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([str(build("filter_plan"))], input=TEXT, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    return out


def test_rules_match_the_restatement(lines):
    routes = set()
    for (nq, k, n, pairs, force, N), line in zip(CASES, lines):
        p = json.loads(line)
        npad = (N + 511) // 512 * 512
        s = splits(nq, k, n)
        lst = keeps_list(n, pairs)
        nbytes = npad // 32 * 4 + 8 + npad * 4 + (2 * npad * 4 if N & 1 else 0)
        if lst:
            nbytes += max(n, 4) * 4 + (npad // 32 + 63) // 64 * 4
        want = dict(sparse=int(route_sparse(nq, k, n, pairs, force)), list=int(lst), blocked=int(blocked(nq, k)), splits=s,
                    per_split=per_split(n, s), words_in=(N + 31) // 32, words=npad // 32, segments=(npad // 32 + 63) // 64,
                    mask_tail=mask((N - 1) // 32, N), mask_next=mask((N - 1) // 32 + 1, N), bytes=nbytes)
        assert p == want, ((nq, k, n, pairs, force, N), p, want)
        # what the kernels and the entry points rely on
        assert not p["sparse"] or p["list"], "a call routed to the sparse kernel finds the list its install built"
        assert p["splits"] * p["per_split"] >= n and p["per_split"] % 64 == 0 and 1 <= p["splits"] <= MAX_SPLITS
        assert p["splits"] == 1 or nq * p["splits"] * k * 16 <= PARTIAL_BYTES
        assert p["words"] >= p["words_in"] and bin(p["mask_tail"]).count("1") == (N - 1) % 32 + 1 and p["mask_next"] == 0
        assert force == 0 or not p["sparse"]
        routes.add((p["sparse"], p["blocked"], p["splits"] > 1))
    assert len(routes) == 8                  # both routes, both kernel forms, one split and several


def test_rule_boundaries(lines):
    """the host program itself, just below, on and just above both limits of the routing rule"""
    got = {c: json.loads(line)["sparse"] for c, line in zip(CASES, lines)}
    for nq, n in ((64, 1000), (1, 5000), (10_000, 100), (7, 4161)):
        assert [got[nq, 10, n, nq * n + dp, 0, n_rows(n)] for dp in (-1, 0, 1)] == [0, 0, 1], (nq, n)    # nq * n < pairs, strictly
    for k in KS:
        assert [got[1, k, few(k) + dn, 0, 0, n_rows(few(k) + dn)] for dn in (-1, 0, 1)] == [1, 0, 0], k   # n < 2 k + 64, strictly
    assert keeps_list(4159, 0) and not keeps_list(4160, 0) and keeps_list(4160, 4161)


def test_sanitized_build_prints_the_same(lines):
    prog = build("filter_plan_san")
    out = subprocess.run([str(prog)], input=TEXT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == lines

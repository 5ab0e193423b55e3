"""Every device / pinned allocation of libvdbhip is given back: the $VDBHIP_ALLOC_LOG of one child process that builds,
searches (host and device API), resets, re-fills and destroys one handle of every kind must pair each "A" / "HA" line with a
later "F" / "HF" line of the same address and size, never free an address twice, and end with nothing live.

The library opens the log once per process, hence the child: this file run as a script (`--child`).  The parent only reads
the log; nothing here provokes a fault."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CHILD_TIMEOUT_S = 300
KINDS = ["flat", "flat_i8", "int8_only", "stream_panels", "ivf_flat_d64", "ivf_flat_d192", "ivf_sq8", "flat_lsh"]


# ---- the child ---------------------------------------------------------------------------------------------------------------
def _device_search(torch, call, q, k):
    """One device-API search of the host queries `q` on the current torch stream; returns I on the host."""
    q_t = torch.from_numpy(q).cuda()
    D_t = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
    I_t = torch.empty((len(q), k), dtype=torch.int64, device="cuda")
    call(q_t.data_ptr(), len(q), k, D_t.data_ptr(), I_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return I_t.cpu().numpy()


def _floats(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _bytes(n, d, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, d)).astype(np.float32)


def _flat_cycle(torch, idx, X, Q, report, extra=None):
    """add, host search, device search, (extra), reset, re-add, one more host search, destroy"""
    k = 10
    idx.add(X)
    _, I_host = idx.search(Q, k)
    I_dev = _device_search(torch, idx.search_device, Q, k)
    assert np.array_equal(I_host, I_dev)
    report.update({key: idx.stats()[key] for key in ("has_i8_copy", "bytes_resident", "bytes_workspace")})
    if extra:
        extra(idx)
    idx.reset()
    assert idx.stats()["ntotal"] == 0
    idx.add(X)
    idx.search(Q, k)
    idx.close()


def _ivf_cycle(torch, idx, X, Q, report):
    """train, add, (nprobe 8: list-major MFMA scan | nprobe 1: exact list scan) x (host, device), reset, re-add, destroy"""
    k = 10
    idx.train(X, niter=2)
    idx.add(X)
    idx.reserve(len(Q), k)
    for nprobe in (8, 1):
        idx.set_nprobe(nprobe)
        _, I_host = idx.search(Q, k)
        scanned = idx.stats()["last_rows_scanned"]             # (> 0 only behind the list-major MFMA scan)
        I_dev = _device_search(torch, idx.search_device, Q, k)
        assert np.array_equal(I_host, I_dev)
        report[f"nprobe{nprobe}_mfma"] = bool(scanned > 0)
    report.update({key: idx.stats()[key] for key in ("bytes_resident", "bytes_workspace")})
    idx.reset()
    idx.add(X)
    idx.set_nprobe(8)
    idx.search(Q, k)
    idx.close()


def child() -> None:
    sys.path[:0] = [str(ROOT), str(ROOT / "vectordb-retrieval_amd")]
    import torch
    import vdbhip
    from vdbhip import _ffi

    report = {kind: {} for kind in KINDS}
    Q32, Q64, Q192 = _floats(64, 32, 1), _floats(64, 64, 2), _floats(64, 192, 3)
    Qb = _bytes(64, 64, 4)

    def flat_extras(idx):           # the other host-API entry points that stage through the workspace or own temporaries
        idx.reserve(64, 10)
        idx.rerank(Q32, np.tile(np.arange(20, dtype=np.int64), (64, 1)), 10)
        idx.debug_scan_scores(Q32[:8], 0, 512)

    _flat_cycle(torch, vdbhip.FlatIndex(32, "l2", 0), _floats(20000, 32, 10), Q32, report["flat"], flat_extras)
    _flat_cycle(torch, vdbhip.FlatIndex(64, "l2", 0), _bytes(20000, 64, 11), Qb, report["flat_i8"])

    idx = vdbhip.FlatIndex(64, "l2", 0)
    idx.set_option("int8_only", 1)
    _flat_cycle(torch, idx, _bytes(40000, 64, 12), Qb, report["int8_only"])

    idx = vdbhip.FlatIndex(192, "ip", 0)
    idx.set_option("stream_panels", 1)
    _flat_cycle(torch, idx, _floats(20000, 192, 13), Q192, report["stream_panels"])

    _ivf_cycle(torch, vdbhip.IVFFlatIndex(64, 32, "l2", 0), _floats(20000, 64, 14), Q64, report["ivf_flat_d64"])
    _ivf_cycle(torch, vdbhip.IVFFlatIndex(192, 32, "l2", 0), _floats(20000, 192, 15), Q192, report["ivf_flat_d192"])
    _ivf_cycle(torch, vdbhip.IVFSQ8Index(64, 32, "l2", 0), _floats(20000, 64, 16), Q64, report["ivf_sq8"])

    def lsh_extras(idx):
        _, I_host = idx.lsh_search(Q32, 10, 256)
        I_dev = _device_search(torch, lambda q, nq, k, d, i, st: idx.lsh_search_device(q, nq, k, 256, d, i, st), Q32, 10)
        assert np.array_equal(I_host, I_dev)
        idx.lsh_candidates(Q32, 256)

    idx = vdbhip.FlatIndex(32, "l2", 0)
    idx.lsh_set_projection(vdbhip.make_projection(32, 64, seed=5))
    _flat_cycle(torch, idx, _floats(20000, 32, 17), Q32, report["flat_lsh"], lsh_extras)

    # the multi-device handle: over two GPUs when the box has them, else its shards share GPU 0 (the same host code)
    devs = [0, 1] if _ffi.device_count() >= 2 else [0, 0]
    report["multi"] = {"devices": devs}
    _flat_cycle(torch, vdbhip.FlatIndex(32, "l2", devs), _floats(20000, 32, 18), Q32, report["multi"])
    idx = vdbhip.IVFFlatIndex(64, 32, "l2", devs)
    idx.train(_floats(20000, 64, 19), niter=2)
    idx.add(_floats(20000, 64, 19))
    idx.set_nprobe(8)
    idx.search(Q64, 10)
    idx.reset()
    idx.close()
    print("ALLOC_BALANCE_REPORT " + json.dumps(report), flush=True)


# ---- the parent ----------------------------------------------------------------------------------------------------------------
def check_log(lines):
    """Returns (problems, allocations seen).  Device ("A"/"F") and pinned ("HA"/"HF") addresses are tracked apart."""
    live = {"A": {}, "HA": {}}
    problems, seen = [], 0
    for n, line in enumerate(lines, 1):
        parts = line.split()
        if len(parts) != 3 or parts[0] not in ("A", "F", "HA", "HF"):
            continue                                            # (GRAPH_* lines and the buffers a graph names)
        tag, ptr, size = parts[0], parts[1], int(parts[2])
        if tag in ("A", "HA"):
            seen += 1
            if ptr in live[tag]:
                problems.append(f"line {n}: {tag} {ptr} while the {live[tag][ptr][0]} bytes of line {live[tag][ptr][1]} are live")
            live[tag][ptr] = (size, n)
        else:
            was = live[tag[:-1] + "A"].pop(ptr, None)
            if was is None:
                problems.append(f"line {n}: {tag} {ptr} {size} frees what is not allocated (a double free?)")
            elif was[0] != size:
                problems.append(f"line {n}: {tag} {ptr} {size} frees the {was[0]} bytes of line {was[1]}")
    for tag, table in live.items():
        for ptr, (size, n) in table.items():
            problems.append(f"line {n}: {tag} {ptr} {size} is never freed")
    return problems, seen


def test_every_allocation_is_freed_once(tmp_path):
    log = tmp_path / "alloc.log"
    env = dict(os.environ, VDBHIP_ALLOC_LOG=str(log))
    run = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, cwd=str(ROOT), timeout=CHILD_TIMEOUT_S,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    tail = [ln for ln in run.stdout.splitlines() if ln.startswith("ALLOC_BALANCE_REPORT ")]
    assert tail, run.stdout[-4000:]
    report = json.loads(tail[-1].split(" ", 1)[1])
    print(json.dumps(report, indent=1))                         # (bytes_resident / bytes_workspace of every kind, for the record)
    assert report["flat"]["has_i8_copy"] == 0 and report["flat_i8"]["has_i8_copy"] == 1 and report["int8_only"]["has_i8_copy"] == 2
    for kind in ("ivf_flat_d64", "ivf_flat_d192", "ivf_sq8"):   # both list scans ran (D > 128 SQ8 has no MFMA scan: not built here)
        assert report[kind]["nprobe8_mfma"] is True and report[kind]["nprobe1_mfma"] is False, (kind, report[kind])
    problems, seen = check_log(log.read_text().splitlines())
    print(f"{seen} allocations, {len(problems)} problems")
    assert seen > 100                                           # (the log was written at all)
    assert not problems, "\n".join(problems[:40])


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()

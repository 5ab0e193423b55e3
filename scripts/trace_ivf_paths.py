#!/usr/bin/env python3
"""One fixed sequence of IVF searches through every branch of the IVF search host code (fp16 list scan: 4 / 8 k-steps, 64- /
128-row bins, 2 / 4 / 8 waves; int8 list scan: integer and non-integer batches, and switched off by
"panel_dtype"; K-loop: 256- and 1024-row spans, the square tile, groups of 1 / 2 / 4 rows; SQ8 at D <= 128 and D > 128; exact list scan with one and several splits; the flagged-query
fallback; a second batch inside one call; partial results through a two-shard index; the plan with and without the LDS
histogram; the int8 list scan's rings 2 / 8 and octs; row parts chosen above 2048 and above 4096 work items), for a run under `rocprofv3 --kernel-trace --stats`: two builds of the library that enqueue the same work give
the same kernel names and call counts.  Prints a running checksum of every result so that the outputs can be compared too.
Usage: rocprofv3 --kernel-trace --stats -d DIR -- python scripts/trace_ivf_paths.py"""
import sys, zlib
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "vectordb-retrieval_amd")]
import numpy as np, vdbhip

rng = np.random.default_rng(9)
crc = 0


def run(tag, idx, Q, nprobe, k=10, **opts):
    global crc
    for key, v in opts.items():
        idx.set_option(key, v)
    idx.set_nprobe(nprobe)
    D, I = idx.search(Q, k)
    crc = zlib.crc32(I.tobytes(), zlib.crc32(D.tobytes(), crc))
    st = idx.stats()
    print(tag, len(Q), nprobe, opts, "lists" if st["last_candidates"] > 0 else "exact", st["scan_dtype"], f"{crc:08x}", flush=True)


def gauss(n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def byte_rows(n, d):
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(np.float32)


def ivf(X, nlist, metric="l2", cls=vdbhip.IVFFlatIndex, device=0, **opts):
    idx = cls(X.shape[1], nlist, metric, device)
    for key, v in opts.items():
        idx.set_option(key, v)
    idx.set_centroids(X[:nlist].copy())
    if cls is vdbhip.IVFSQ8Index:
        idx.train_ranges(X)
    idx.add(X)
    return idx


for d in (64, 128):                          # fp16 list scan
    X, Q = gauss(20000, d), gauss(300, d)
    idx = ivf(X, 64)
    for nw in (2, 4, 8):
        for bt in (4, 16):
            run(f"f16_d{d}", idx, Q, 16, ivf_nw=nw, ivf_bt=bt)
    if d == 64:
        idx.set_option("ivf_nw", 0); idx.set_option("ivf_bt", 0)
        run("exact_s1", idx, Q[:8], 1, force_path=1); run("exact_split", idx, Q[:8], 8)
        run("fallback", idx, Q[:64], 16, force_path=0, list_cap=1)
        run("two_batches", idx, np.tile(Q, (56, 1))[:16500], 8, list_cap=0)
    idx.close()
X, Qi = byte_rows(20000, 64), byte_rows(300, 64)          # int8 list scan
idx = ivf(X, 64); run("i8_int", idx, Qi, 8); run("i8_float", idx, Qi + 3 * gauss(300, 64), 8)
run("i8_off", idx, Qi, 8, panel_dtype=1); idx.close()
X, Q = gauss(30000, 256), gauss(200, 256)                 # K-loop
idx = ivf(X, 16, "ip", ivf_tps=64); run("kloop_tps64", idx, Q, 8); idx.close()
idx = ivf(X, 16, "ip", ivf_tps=16)
for group in (1, 2, 4):
    run("kloop_tps16", idx, Q, 8, ivf_group=group)
run("kloop_square", idx, Q, 8, ivf_tile=2, ivf_group=0); idx.close()
for d in (64, 192):                                       # SQ8: list scan over converted panels, exact scan over codes
    X, Q = gauss(20000, d), gauss(300, d)
    idx = ivf(X, 64, cls=vdbhip.IVFSQ8Index); run(f"sq8_d{d}", idx, Q, 16); idx.close()
X, Q = gauss(20000, 64), gauss(300, 64)                   # partial results: two shards on GPU 0
idx = ivf(X, 64, device=[0, 0]); run("two_shards", idx, Q, 16); run("two_shards_exact", idx, Q[:8], 4); idx.close()
for nlist in (2100, 8200):                                # plan: LDS histogram (full pairs per block) | separate kernels
    X, Q = gauss(5 * nlist, 64), gauss(300, 64)
    idx = ivf(X, nlist); run(f"nlist{nlist}", idx, Q, 16); idx.close()
# branches of csrc/ivf_plan.hpp the walk above does not reach (tests/host/ivf_plan_main.cpp says which)
X, Qi = byte_rows(20000, 128), byte_rows(300, 128)        # int8 list scan: rings 2 / 8, octs
idx = ivf(X, 64)
for ring in (2, 8):
    run("i8_ring", idx, Qi, 8, i8_ring=ring)
run("i8_octs", idx, Qi, 8, i8_ring=0, ivf_i8_group=8); idx.close()
for nlist in (2100, 8200):                                # row parts by work items: above 2048 and above 4096 items, one list of 13 spans
    X, Q = gauss(5 * nlist + 3000, 64), gauss(300, 64)
    X[-3000:] = X[0] + 0.01 * X[-3000:]
    idx = ivf(X, nlist)
    for bt in (4, 16):
        run(f"parts_nlist{nlist}", idx, Q, 16, k=5, ivf_bt=bt)
    idx.close()
print(f"checksum {crc:08x}")

#!/usr/bin/env python3
"""One fixed sequence of flat searches through every branch of search_batch (dense, exhaustive, MFMA scan: resident fp16,
paired with int8, streamed slabs, int8-only slabs, PQ slabs; direct bins; serving shapes; the options "scan_pair", "small_batch",
"fused_stats" and "panel_dtype" at their non-default value), for a run under
`rocprofv3 --kernel-trace --stats`: two builds of the library that enqueue the same work give the same kernel names and
call counts.  Prints a checksum of every result so that the outputs can be compared as well.
Usage: rocprofv3 --kernel-trace --stats -d DIR -- python scripts/trace_search_paths.py"""
import sys, zlib
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "vectordb-retrieval_amd")]
import numpy as np, vdbhip

rng = np.random.default_rng(8)
crc = 0


def run(tag, idx, Q, batches=(600, 64, 3), ks=(10, 100)):
    global crc
    for nq in batches:
        for k in ks:
            D, I = idx.search(Q[:nq], k)
            crc = zlib.crc32(I.tobytes(), zlib.crc32(D.tobytes(), crc))
            print(tag, nq, k, idx.stats()["last_path_name"], f"{crc:08x}", flush=True)


def gauss(n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def byte_rows(n, d):
    return np.clip(np.round(rng.gamma(0.6, 40.0, size=(n, d))), 0, 218).astype(np.float32)


def flat(X, metric="l2", **opts):
    idx = vdbhip.FlatIndex(X.shape[1], metric, 0)
    for key, v in opts.items():
        idx.set_option(key, v)
    idx.add(X)
    return idx


X, Q = gauss(5000, 64), gauss(600, 64)
idx = flat(X); run("dense", idx, Q, ks=(10,)); idx.close()
X, Q = gauss(12000, 96), gauss(600, 96)
idx = flat(X, "ip"); run("dense_lds", idx, Q, batches=(600,), ks=(40,)); run("exact", idx, Q, batches=(8,), ks=(10,)); idx.close()
X, Q = gauss(40000, 128), gauss(600, 128)
idx = flat(X); run("f16", idx, Q)
idx.set_option("force_path", 1); run("exact_blocked", idx, Q, batches=(600, 5), ks=(10,))
idx.set_option("force_path", 0); idx.set_option("list_cap", 1); run("fallback", idx, Q, batches=(64,), ks=(10,)); idx.close()
X, Qi = byte_rows(40000, 128), byte_rows(1024, 128)
Qf = Qi + gauss(1024, 128) * 3
idx = flat(X); run("pair_int", idx, Qi, batches=(1024, 600, 64, 3)); run("pair_float", idx, Qf, ks=(10,))
idx.set_option("scan_pair", 0); run("two_launches", idx, Qi, ks=(10,)); idx.set_option("scan_pair", 1)
for opt, off in (("small_batch", 0), ("fused_stats", 0), ("panel_dtype", 1)):      # each at its other value, the rest at their defaults
    idx.set_option(opt, off); run(f"{opt}={off}", idx, Qi, batches=(64, 3), ks=(10,)); idx.set_option(opt, 1 - off)
idx.close()
idx = flat(X, flat_shape=32); run("i8_32", idx, Qi, ks=(10,)); idx.close()
X, Q = gauss(47000, 136), gauss(600, 136)
idx = flat(X, stream_panels=1, stream_slab_rows=20480); run("streamed", idx, Q)
idx.set_option("small_batch", 0); run("streamed_small_batch=0", idx, Q, batches=(64, 3), ks=(10,)); idx.close()
X, Qi = byte_rows(40000, 50), byte_rows(600, 50)
idx = flat(X, int8_only=1, int8_slab_chunks=3); run("int8_only_float", idx, Qi + gauss(600, 50) * 3); run("int8_only_int", idx, Qi, ks=(10,))
cand = rng.integers(0, 40000, size=(20, 30)).astype(np.int64)
D, I = idx.rerank(Qi[:20], cand, 5); crc = zlib.crc32(I.tobytes(), zlib.crc32(D.tobytes(), crc)); idx.close()
for d in (64, 192):
    X, Q = gauss(40000, d), gauss(600, d)
    pq = vdbhip.PQIndex(d, 16, "l2", 0)
    pq.train(X[:4096], niter=2)
    pq.add(X)
    pq.set_option("pq_slab_chunks", 3); run(f"pq{d}", pq, Q); pq.close()
print(f"checksum {crc:08x}")

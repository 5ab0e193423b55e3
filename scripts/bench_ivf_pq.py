"""IVF1024,PQ64 and IVF1024,PQ16 vs IVF1024,SQ8 and IVF1024,Flat on the same centroids: QPS, recall@10, per-stage times and
resident footprint.

Gaussian 1M x 128 corpus (non-integer values: IVF-Flat takes its fp16 list scan), 10 000 Gaussian queries, k = 10, l2.
The IVF-Flat index trains the centroids (the library's k-means, 25 iterations, seed 1234); the SQ8 index gets the same
centroids and trains its ranges on the corpus, the IVF-PQ indexes get them and train their codebooks on the residuals
(25 iterations, seed 1234).  The coded indexes make their fp16 panels per batch before the scan: that pass is part of
`prep_ms` (IVF-Flat's prep_ms is the same prep without it), and `panel_pass` reports the difference with the bytes the
pass writes per second.  Per nprobe: device-resident QPS timed as bench.py's IVF legs (queries and
results in HBM, `warmup` untimed searches, then `steps` timed ones between two device synchronisations), recall@10 against
the exact float64 result, and (bytes_resident - bytes_workspace) / (4 N D).  Prints ONE JSON line.

    python scripts/bench_ivf_pq.py [--steps 5] [--warmup 2] [--n 1000000]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "vectordb-retrieval_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def recall(exact, got, k):
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(exact, got)]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--M", type=int, nargs="+", default=[64, 16])
    args = ap.parse_args()
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    d, k, nlist = 128, 10, 1024
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X_t = torch.randn((args.n, d), generator=g, device=dev, dtype=torch.float32)
    Q_t = torch.randn((args.nq, d), generator=g, device=dev, dtype=torch.float32)
    X, Q = X_t.cpu().numpy(), Q_t.cpu().numpy()
    del X_t
    flat_exact = vdbhip.FlatIndex(d, "l2", 0)
    flat_exact.add(X)
    _, exact = flat_exact.search(Q, k)
    flat_exact.close()
    t0 = time.perf_counter()
    fl = vdbhip.IVFFlatIndex(d, nlist, "l2", 0)
    fl.train(X, niter=25, seed=1234, max_points_per_centroid=256)
    fl.add(X)
    t_fl = time.perf_counter() - t0
    t0 = time.perf_counter()
    sq = vdbhip.IVFSQ8Index(d, nlist, "l2", 0)
    sq.set_centroids(fl.centroids())
    sq.train_ranges(X)
    sq.add(X)
    t_sq = time.perf_counter() - t0
    pqs, t_pq = {}, {}
    for M in args.M:
        t0 = time.perf_counter()
        pq = vdbhip.IVFPQIndex(d, nlist, M, "l2", 0)
        pq.set_centroids(fl.centroids())
        pq.train_codebooks(X, niter=25, seed=1234, max_points_per_centroid=256)
        pq.add(X)
        t_pq[f"pq{M}"] = round(time.perf_counter() - t0, 2)
        pqs[f"pq{M}"] = pq
    D_t = torch.empty((args.nq, k), dtype=torch.float32, device=dev)
    I_t = torch.empty((args.nq, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"config": f"Gaussian {args.n} x {d}, {args.nq} queries, k={k}, l2; IVF{nlist} (own k-means, the same centroids "
                     f"for Flat, SQ8 and PQ)", "build_s": dict({"flat": round(t_fl, 2), "sq8": round(t_sq, 2)}, **t_pq)}
    for name, idx in [("flat", fl), ("sq8", sq)] + list(pqs.items()):
        res = {}
        for p in args.nprobe:
            idx.set_nprobe(p)
            for _ in range(args.warmup):
                idx.search_device(Q_t.data_ptr(), args.nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            idx.set_option("timing", 1)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                idx.search_device(Q_t.data_ptr(), args.nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            st = idx.stats()
            idx.set_option("timing", 0)
            res[f"nprobe{p}"] = {"qps": round(args.nq * args.steps / el, 1), "ms_per_search": round(el / args.steps * 1e3, 3),
                                 "recall@10": round(recall(exact, I_t.cpu().numpy(), k), 6),
                                 "scan_ms": round(st["last_scan_ms"], 3), "prep_ms": round(st["last_prep_ms"], 3),
                                 "tail_ms": round(st["last_tail_ms"], 3), "path": st["last_path_name"],
                                 "candidates_per_query": round(st["last_candidates"] / args.nq, 2)}
        st = idx.stats()
        res["resident_over_fp32_corpus"] = round((st["bytes_resident"] - st["bytes_workspace"]) / (4.0 * args.n * d), 4)
        out[name] = res
    # the per-batch panel pass of the coded indexes: prep_ms over IVF-Flat's, and the fp16 panel bytes it writes per second
    counts = np.bincount(fl.assignment(), minlength=nlist)
    panel_bytes = int(((counts + 255) // 256 * 256).sum()) * d * 2
    for name in [n for n in out if n not in ("config", "build_s", "flat")]:
        for p in args.nprobe:
            ms = out[name][f"nprobe{p}"]["prep_ms"] - out["flat"][f"nprobe{p}"]["prep_ms"]
            out[name][f"nprobe{p}"]["panel_pass"] = {"ms": round(ms, 3), "panel_GB_per_s": round(panel_bytes / max(ms, 1e-6) / 1e6, 1)}
            if name != "sq8":
                out[name][f"nprobe{p}"]["qps_over_sq8"] = round(out[name][f"nprobe{p}"]["qps"] / out["sq8"][f"nprobe{p}"]["qps"], 3)
    out["panel_bytes"] = panel_bytes
    print(json.dumps(out))
    fl.close()
    sq.close()
    for pq in pqs.values():
        pq.close()


if __name__ == "__main__":
    main()

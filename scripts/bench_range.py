"""Range search (vdb_range_search_device) against the k-NN search of the same handle and a chunked torch baseline, on one corpus.

    --corpus gauss128   Gaussian 1M x 128, l2
    --corpus bytes128   byte-valued 1M x 128, l2 (SIFT-shaped: integers 0..255; the index keeps its int8 copy, the fp16 copy serves
                        the range prefilter)
    --corpus unit384    unit vectors 1M x 384, ip

Batches of 1, 64 and 10 000 queries.  Radii: those at which the same handle's vdb_search gives a median 10th and 100th neighbour
distance over the batch of 10 000 -- about 10 and about 100 results per query.  Everything is device-resident.  Per leg, in the same
run and alternating step by step: the range search (search + copying the result out), vdb_search_device with k = 10 and the torch
baseline (row chunks of Q @ X.T, compare, nonzero); every figure is the median over `steps` calls of the time between two device
events, after `warmup` untimed rounds.  Also per leg: total results, last_candidates / total, and the three stage times the library
records under option "timing" (prep, prefilter scan, exact filter + emit), taken in a pass of their own.  The result is merged under
its corpus name into the JSON file --out (default profiles/r20_bench_range.json) and printed as one line.  One corpus per process,
each under its own time limit:

    timeout -k 10 500 python scripts/bench_range.py --corpus gauss128 && \\
    timeout -k 10 500 python scripts/bench_range.py --corpus bytes128 && \\
    timeout -k 10 500 python scripts/bench_range.py --corpus unit384
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "vectordb-retrieval_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

K = 10
BATCHES = (1, 64, 10_000)
TORCH_CHUNK_ROWS = 65_536


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["gauss128", "bytes128", "unit384"], required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r20_bench_range.json"))
    args = ap.parse_args()
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    n, nq_max = args.n, max(BATCHES)
    d, metric = (384, "ip") if args.corpus == "unit384" else (128, "l2")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    if args.corpus == "bytes128":
        X_t = torch.clamp(torch.round(torch.empty((n, d), device=dev).exponential_(1.0 / 30.0, generator=g)), 0, 255)
        Q_t = torch.clamp(torch.round(torch.empty((nq_max, d), device=dev).exponential_(1.0 / 30.0, generator=g)), 0, 255)
    else:
        X_t = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
        Q_t = torch.randn((nq_max, d), generator=g, device=dev, dtype=torch.float32)
        if args.corpus == "unit384":
            X_t /= X_t.norm(dim=1, keepdim=True)
            Q_t /= Q_t.norm(dim=1, keepdim=True)
    stream = torch.cuda.current_stream().cuda_stream
    idx = vdbhip.FlatIndex(d, metric, 0)
    idx.add_device(X_t.data_ptr(), n, 0, stream)
    torch.cuda.synchronize()
    built = idx.stats()

    # radii from the handle's own k-NN search
    D100 = torch.empty((nq_max, 100), dtype=torch.float32, device=dev)
    I100 = torch.empty((nq_max, 100), dtype=torch.int64, device=dev)
    idx.search_device(Q_t.data_ptr(), nq_max, 100, D100.data_ptr(), I100.data_ptr(), stream)
    torch.cuda.synchronize()
    radii = {"10": float(D100[:, 9].median()), "100": float(D100[:, 99].median())}

    Dk = torch.empty((nq_max, K), dtype=torch.float32, device=dev)
    Ik = torch.empty((nq_max, K), dtype=torch.int64, device=dev)
    lims_t = torch.empty((nq_max + 1,), dtype=torch.int64, device=dev)
    xn2 = (X_t * X_t).sum(dim=1) if metric == "l2" else None
    out_buf = {"D": torch.empty((1,), dtype=torch.float32, device=dev), "I": torch.empty((1,), dtype=torch.int64, device=dev)}

    def run_range(nq, r):
        total = idx.range_search_device(Q_t.data_ptr(), nq, r, lims_t.data_ptr(), stream)
        if total > out_buf["D"].numel():
            out_buf["D"] = torch.empty((total + total // 4,), dtype=torch.float32, device=dev)
            out_buf["I"] = torch.empty((total + total // 4,), dtype=torch.int64, device=dev)
        idx.range_results_device(out_buf["D"].data_ptr(), out_buf["I"].data_ptr(), stream)
        return total

    def run_knn(nq):
        idx.search_device(Q_t.data_ptr(), nq, K, Dk.data_ptr(), Ik.data_ptr(), stream)

    def run_torch(nq, r):
        Q = Q_t[:nq]
        qn2 = (Q * Q).sum(dim=1, keepdim=True) if metric == "l2" else None
        found = 0
        for r0 in range(0, n, TORCH_CHUNK_ROWS):
            s = Q @ X_t[r0:r0 + TORCH_CHUNK_ROWS].T
            hit = (qn2 - 2.0 * s + xn2[None, r0:r0 + TORCH_CHUNK_ROWS] < r) if metric == "l2" else (s > r)
            found += int(hit.nonzero().shape[0])
        return found

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    legs = {}
    for nq in BATCHES:
        for name, r in radii.items():
            calls = {"range": lambda: run_range(nq, r), "knn_k10": lambda: run_knn(nq), "torch": lambda: run_torch(nq, r)}
            times = {c: [] for c in calls}
            for step in range(args.warmup + args.steps):          # alternating: one call of each per round
                for c, fn in calls.items():
                    ms = event_ms(fn)
                    if step >= args.warmup:
                        times[c].append(ms)
            total = run_range(nq, r)
            st = idx.stats()
            idx.set_option("timing", 1)                            # the stage times, in a pass of their own (events cost a little)
            for _ in range(args.steps):
                run_range(nq, r)
            torch.cuda.synchronize()
            tm = idx.stats()
            idx.set_option("timing", 0)
            legs[f"nq{nq}_about{name}"] = {
                "nq": nq, "radius": r, "total_results": int(total), "torch_results": int(run_torch(nq, r)),
                "range_ms": statistics.median(times["range"]), "knn_k10_ms": statistics.median(times["knn_k10"]),
                "torch_ms": statistics.median(times["torch"]),
                "candidates": int(st["last_candidates"]), "candidates_per_result": st["last_candidates"] / max(total, 1),
                "fallback_queries": int(st["last_fallback_queries"]),
                "prep_ms": tm["last_prep_ms"], "scan_ms": tm["last_scan_ms"], "tail_ms": tm["last_tail_ms"],
            }
    result = {"corpus": args.corpus, "n": n, "dim": d, "metric": metric, "steps": args.steps, "warmup": args.warmup,
              "scan_shape": built["scan_shape"], "has_i8_copy": built["has_i8_copy"], "range_bitmap_mb": 256,
              "bytes_resident_after": idx.stats()["bytes_resident"], "legs": legs}
    idx.close()
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[args.corpus] = result
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

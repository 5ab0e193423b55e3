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

    --adc   the lookup-table (ADC) scan of the probed lists against the path the batch takes without it, on the IVF-PQ indexes alone
            (profiles/r19_bench_ivfpq_adc.json).  ONE handle per workload; per nprobe and nq in {1, 2, 4, ..., 512} device-resident
            searches with option "ivfpq_adc_max_batch" 0 (the parent's behaviour) and 512 in alternating rounds, median of 20 after 3,
            results asserted identical in every cell, then the stage timers of each setting.  Workloads: Gaussian 1M x 128, l2,
            IVF1024,PQ64 and IVF1024,PQ16 at nprobe 8 and 32; unit vectors 100 000 x 384, ip, IVF256,PQ64 at nprobe 24.  "value_to_set":
            the largest nq up to which every batch size is faster with the option by more than 8 % (the box-to-box spread).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import statistics
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


ADC_WORKLOADS = {      # name: (rows, dim, nlist, M, metric, unit vectors, nprobes)
    "gauss128_ivf1024_pq64": (1_000_000, 128, 1024, 64, "l2", False, (8, 32)),
    "gauss128_ivf1024_pq16": (1_000_000, 128, 1024, 16, "l2", False, (8, 32)),
    "unit384_ivf256_pq64": (100_000, 384, 256, 64, "ip", True, (24,)),
}
ADC_NQ = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
ADC_SPREAD = 0.08


def adc_cell(torch, idx, Q_t, m, k, steps, warmup, stream):
    dev = Q_t.device
    settings = (("off", 0), ("adc", 512))
    outs = {name: (torch.empty((m, k), dtype=torch.float32, device=dev), torch.empty((m, k), dtype=torch.int64, device=dev)) for name, _ in settings}

    def search(name, value):
        idx.set_option("ivfpq_adc_max_batch", value)
        D_t, I_t = outs[name]
        idx.search_device(Q_t.data_ptr(), m, k, D_t.data_ptr(), I_t.data_ptr(), stream)

    for _ in range(warmup):
        for name, value in settings:
            search(name, value)
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in settings}
    for _ in range(steps):
        for name, value in settings:
            idx.set_option("ivfpq_adc_max_batch", value)
            D_t, I_t = outs[name]
            t0 = time.perf_counter()
            idx.search_device(Q_t.data_ptr(), m, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    row, sums = {}, {}
    for name, value in settings:
        idx.set_option("timing", 1)
        for _ in range(steps):
            search(name, value)
        torch.cuda.synchronize()
        st = idx.stats()
        idx.set_option("timing", 0)
        sums[name] = hashlib.sha256(outs[name][1].cpu().numpy().tobytes() + outs[name][0].cpu().numpy().tobytes()).hexdigest()[:16]
        row[name] = {"ms": round(statistics.median(ms[name]), 4), "path": st["last_path_name"], "scan_dtype": st["scan_dtype"],
                     "prep_ms": round(st["last_prep_ms"], 4), "scan_ms": round(st["last_scan_ms"], 4), "tail_ms": round(st["last_tail_ms"], 4),
                     "total_ms": round(st["last_total_ms"], 4), "rows_rescored_or_candidates_per_query": round(st["last_candidates"] / m, 2),
                     "flagged_queries": st["last_fallback_queries"]}
    row["adc_over_off_time"] = round(row["adc"]["ms"] / row["off"]["ms"], 4)
    row["same_results"] = sums["adc"] == sums["off"]
    assert row["same_results"], (m, sums)
    return row


def adc_main(args) -> None:
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    k = 10
    path = Path(args.out or str(ROOT / "profiles" / "r19_bench_ivfpq_adc.json"))
    allres = json.loads(path.read_text()) if path.exists() else {}
    stream = torch.cuda.current_stream().cuda_stream
    trained = {}
    for name in args.workload or sorted(ADC_WORKLOADS):
        n, d, nlist, M, metric, unit, nprobes = ADC_WORKLOADS[name]
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        X_t = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
        Q_t = torch.randn((max(ADC_NQ), d), generator=g, device=dev, dtype=torch.float32)
        if unit:
            X_t /= X_t.norm(dim=1, keepdim=True)
            Q_t /= Q_t.norm(dim=1, keepdim=True)
        X = X_t.cpu().numpy()
        del X_t
        t0 = time.perf_counter()
        idx = vdbhip.IVFPQIndex(d, nlist, M, metric, 0)
        key = (n, d, nlist, metric, unit)
        if key in trained:              # (the same corpus and lists as the workload before: its centroids)
            idx.set_centroids(trained[key])
            idx.train_codebooks(X, niter=args.niter, seed=1234, max_points_per_centroid=256)
        else:
            idx.train(X, niter=args.niter, seed=1234, max_points_per_centroid=256)
            trained[key] = idx.centroids()
        idx.add(X)
        build_s = time.perf_counter() - t0
        sizes = np.bincount(idx.assignment(), minlength=nlist)
        res = {"config": f"{name}: {n} x {d}, IVF{nlist},PQ{M}, {metric}, k={k}, device-resident searches of one handle, option "
                         f"ivfpq_adc_max_batch 0 / 512 alternating, median of {args.steps} rounds after {args.warmup}; k-means iterations {args.niter}",
               "build_s": round(build_s, 2), "longest_list": int(sizes.max()), "median_list": int(np.median(sizes)), "nprobe": {}}
        for p in nprobes:
            idx.set_nprobe(p)
            cells = {str(m): adc_cell(torch, idx, Q_t, m, k, args.steps, args.warmup, stream) for m in ADC_NQ}
            value = 0
            for m in ADC_NQ:
                if cells[str(m)]["adc_over_off_time"] >= 1.0 - ADC_SPREAD:
                    break
                value = m
            res["nprobe"][str(p)] = {"batches": cells, "value_to_set": value}
        st = idx.stats()
        res["resident_over_fp32_corpus"] = round((st["bytes_resident"] - st["bytes_workspace"]) / (4.0 * n * d), 4)
        idx.close()
        allres[name] = res
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(allres, indent=1) + "\n")
        print(json.dumps({name: {p: {"value_to_set": v["value_to_set"], "adc_over_off_time": {m: c["adc_over_off_time"] for m, c in v["batches"].items()}}
                                 for p, v in res["nprobe"].items()}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--adc", action="store_true", help="only the ADC leg: option ivfpq_adc_max_batch 0 against 512 on small batches")
    ap.add_argument("--workload", nargs="+", choices=sorted(ADC_WORKLOADS), help="--adc: the workloads to run (default: all)")
    ap.add_argument("--niter", type=int, default=25, help="--adc: k-means iterations of centroids and codebooks")
    ap.add_argument("--out", default=None, help="--adc: the JSON file to write (default profiles/r19_bench_ivfpq_adc.json)")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--M", type=int, nargs="+", default=[64, 16])
    args = ap.parse_args()
    if args.adc:
        if args.steps == 5 and args.warmup == 2:      # (the defaults of the throughput legs: the ADC leg takes medians of 20 after 3)
            args.steps, args.warmup = 20, 3
        return adc_main(args)
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

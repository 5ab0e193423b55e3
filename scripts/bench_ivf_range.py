"""Range search on an IVF-Flat index (vdb_ivf_range_search_device) against the k-NN search of the same handle, its own exact route and
the flat range search over the same rows.

    --corpus gauss128   Gaussian 1M x 128, l2, IVF1024,Flat, nprobe 8 / 32 / 128 (the fp16 list scan)
    --corpus bytes128   byte-valued 1M x 128, l2, IVF1024,Flat, nprobe 8 / 32 / 128 (the fp16 list scan: the int8 copies are not used)
    --corpus unit384    unit vectors 100 000 x 384, ip, IVF100,Flat, nprobe 32 (the K-loop list scan)

Everything is device-resident.  Every figure is the median over `steps` calls of the time between two device events, after `warmup`
untimed rounds; the compared calls of a leg alternate step by step on the same handle (option "force_path" is set outside the timed
region).  Per nprobe and batch (1, 64, 10 000 queries) the radii are the batch medians of the 10th and the 100th returned D of
vdb_ivf_search; a leg reports

  range_ms / exact_route_ms / knn10_ms / flat_range_ms      the routed call, the same call under force_path 1, vdb_ivf_search_device
                                                            (k = 10) and vdb_range_search_device of a flat handle over the same rows
  results, flat_results          the two result counts (they differ by the unprobed lists)
  candidates, candidates_per_result, fallback_queries, probed_pairs (= the exact route's candidates)
  stages                         prep / scan / tail of the routed call under option "timing" (averages over the slabs of the calls; the
                                 bitmap clear is enqueued with the prep, the whole-row reads of the filter and emit passes are tail)
  empty_ms, empty                the routed call at a radius no row can pass, and its stages: the coarse search, the bitmap clear, the
                                 scan and the whole-row reads, with nothing to mark and nothing to score

The result is merged under its corpus name into the JSON file --out and printed as one line.  One corpus per process, each under
its own time limit:

    timeout -k 10 500 python scripts/bench_ivf_range.py --corpus gauss128 && \\
    timeout -k 10 500 python scripts/bench_ivf_range.py --corpus bytes128 && \\
    timeout -k 10 300 python scripts/bench_ivf_range.py --corpus unit384
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "vectordb-retrieval_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCHES = (10_000, 64, 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["bytes128", "gauss128", "unit384"], required=True)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--niter", type=int, default=8, help="k-means iterations of the index build")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r24_bench_ivf_range.json"))
    args = ap.parse_args()
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    if args.corpus == "unit384":
        n, d, metric, nlist, nprobes = 100_000, 384, "ip", 100, (32,)
    else:
        n, d, metric, nlist, nprobes = 1_000_000, 128, "l2", 1024, (8, 32, 128)
    nq_max = max(BATCHES)
    g = torch.Generator(device=dev)
    g.manual_seed(0)

    def rows(count):
        if args.corpus == "bytes128":
            return torch.clamp(torch.round(torch.empty((count, d), device=dev).exponential_(1.0 / 30.0, generator=g)), 0, 255)
        x = torch.randn((count, d), generator=g, device=dev, dtype=torch.float32)
        return x / x.norm(dim=1, keepdim=True) if args.corpus == "unit384" else x

    X_t, Q_t = rows(n), rows(nq_max)
    X = X_t.cpu().numpy()
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    idx = vdbhip.IVFFlatIndex(d, nlist, metric, 0)
    idx.train(X, niter=args.niter)
    idx.add(X)
    build_s = time.perf_counter() - t0
    flat = vdbhip.FlatIndex(d, metric, 0)
    flat.add(X)
    del X
    Dk = torch.empty((nq_max, 100), dtype=torch.float32, device=dev)
    Ik = torch.empty((nq_max, 100), dtype=torch.int64, device=dev)
    lims = torch.empty((nq_max + 1,), dtype=torch.int64, device=dev)
    none_radius = 0.0 if metric == "l2" else float("inf")

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def alternate(calls):
        """calls: name -> (untimed setup or None, timed call)"""
        times = {c: [] for c in calls}
        for step in range(args.warmup + args.steps):
            for c, (setup, fn) in calls.items():
                if setup:
                    setup()
                ms = event_ms(fn)
                if step >= args.warmup:
                    times[c].append(ms)
        return {c: statistics.median(v) for c, v in times.items()}

    def force(v):
        return lambda: idx.set_option("force_path", v)

    legs = {}
    for nprobe in nprobes:
        idx.set_nprobe(nprobe)
        for nq in BATCHES:
            idx.search_device(Q_t.data_ptr(), nq, 100, Dk.data_ptr(), Ik.data_ptr(), stream)
            torch.cuda.synchronize()
            for rank in (10, 100):
                radius = float(Dk[:nq, rank - 1].median())
                rng = lambda r=radius: idx.range_search_device(Q_t.data_ptr(), nq, r, lims.data_ptr(), stream)       # noqa: E731
                t = alternate({
                    "range": (force(0), rng),
                    "exact_route": (force(1), rng),
                    "knn10": (force(0), lambda: idx.search_device(Q_t.data_ptr(), nq, 10, Dk.data_ptr(), Ik.data_ptr(), stream)),
                    "flat_range": (None, lambda r=radius: flat.range_search_device(Q_t.data_ptr(), nq, r, lims.data_ptr(), stream)),
                })
                idx.set_option("force_path", 1)
                results = rng()
                pairs = int(idx.stats()["last_candidates"])
                idx.set_option("force_path", 0)
                assert rng() == results
                st = idx.stats()
                flat_results = flat.range_search_device(Q_t.data_ptr(), nq, radius, lims.data_ptr(), stream)
                leg = {"nprobe": nprobe, "nq": nq, "rank": rank, "radius": radius, "range_ms": t["range"], "exact_route_ms": t["exact_route"],
                       "knn10_ms": t["knn10"], "flat_range_ms": t["flat_range"], "results": int(results), "flat_results": int(flat_results),
                       "candidates": int(st["last_candidates"]), "candidates_per_result": st["last_candidates"] / max(1, results),
                       "fallback_queries": int(st["last_fallback_queries"]), "probed_pairs": pairs}
                # the stage times in a pass of their own: setting option "timing" restarts the recording window
                for name, r in (("stages", radius), ("empty", none_radius)):
                    idx.set_option("timing", 1)
                    for _ in range(args.steps):
                        idx.range_search_device(Q_t.data_ptr(), nq, r, lims.data_ptr(), stream)
                    torch.cuda.synchronize()
                    s2 = idx.stats()
                    leg[name] = {"prep_ms": s2["last_prep_ms"], "scan_ms": s2["last_scan_ms"], "tail_ms": s2["last_tail_ms"]}
                idx.set_option("timing", 0)
                leg["empty_ms"] = alternate({"empty": (None, lambda: idx.range_search_device(Q_t.data_ptr(), nq, none_radius, lims.data_ptr(), stream))})["empty"]
                legs[f"nprobe{nprobe}_nq{nq}_rank{rank}"] = leg
    idx.close()
    flat.close()
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    result = {"corpus": args.corpus, "n": n, "dim": d, "metric": metric, "nlist": nlist, "steps": args.steps, "warmup": args.warmup,
              "niter": args.niter, "build_s": build_s, "legs": legs}
    merged[args.corpus] = result
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

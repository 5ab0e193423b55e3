"""The int8 K-loop list scan (option "ivf_i8_kloop") against the fp16 K-loop list scan of the SAME IVF-Flat handle ("panel_dtype" = 1),
in one process.

s8-valued corpora (uniform integers -128..127), centroids = rows of the corpus drawn with a seed (no k-means: uniform data has no
clusters to find, and both legs share the lists):
    msmarco   IVF100 over 100 000 x 384, nprobe 32, k = 20 (the msmarco IVF shape)
    ivf1024   IVF1024 over 1 000 000 x 768, nprobe 8 / 32 / 128, k = 10
with batches of 10 000, 64 and 1 integer queries through the device entry point.  Per (shape, nprobe, batch) the two legs alternate
call by call; each figure is the median, the spread the min and max, over `steps` calls of the time between two device events after
`warmup` untimed rounds.  Per leg also the stages under option "timing" (prep = statistics, query rows, plan | scan = the list scan |
tail = select + refine), candidates per query, fallback queries and scan_dtype, and whether the two legs return the same bytes.

--mode off: the option is never set and only the fp16 leg is timed -- run once per library (environment VDBHIP_LIBRARY) to compare
this commit with its parent on the path the commit must not change; --tag names the run in the output.

    timeout -k 10 900 python scripts/bench_ivf_i8k.py                  # writes profiles/r29_bench_ivf_i8k.json
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

SHAPES = {"msmarco": (100_000, 384, 100, (32,), 20), "ivf1024": (1_000_000, 768, 1024, (8, 32, 128), 10)}      # N, D, nlist, nprobes, k
BATCHES = (10_000, 64, 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--mode", choices=("ab", "off"), default="ab")
    ap.add_argument("--tag", default="")
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="rows of every shape x this (rehearsals)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r29_bench_ivf_i8k.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import vdbhip

    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_i8k: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    legs = ("i8k", "fp16") if args.mode == "ab" else ("fp16",)
    result = {"mode": args.mode, "tag": args.tag, "metric": args.metric, "steps": args.steps, "legs": {}}
    for name in args.shapes:
        n, d, nlist, nprobes, k = SHAPES[name]
        n = max(nlist * 40, int(n * args.scale))
        rng = np.random.default_rng(29)
        X = rng.integers(-128, 128, (n, d), dtype=np.int8).astype(np.float32)
        Q = torch.from_numpy(rng.integers(-128, 128, (max(BATCHES), d), dtype=np.int8).astype(np.float32)).to(dev)
        ix = vdbhip.IVFFlatIndex(d, nlist, args.metric, 0)
        ix.set_centroids(X[rng.choice(n, nlist, replace=False)])
        if args.mode == "ab":
            ix.set_option("ivf_i8_kloop", 1)
        ix.add(X)
        st = ix.stats()
        assert st["has_i8_copy"] == (1 if args.mode == "ab" else 0), st
        corpus = {"n": n, "d": d, "nlist": nlist, "k": k, "bytes_over_corpus": st["bytes_resident"] / (n * d * 4)}
        del X
        for nprobe in nprobes:
            ix.set_nprobe(nprobe)
            for nq in BATCHES:
                out = {leg: (torch.empty((nq, k), device=dev), torch.empty((nq, k), device=dev, dtype=torch.int64)) for leg in legs}
                times = {leg: [] for leg in legs}

                def call(leg):
                    ix.set_option("panel_dtype", 0 if leg == "i8k" else 1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ix.search_device(Q.data_ptr(), nq, k, out[leg][0].data_ptr(), out[leg][1].data_ptr())
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                for step in range(args.warmup + args.steps):
                    for leg in legs:
                        ms = call(leg)
                        if step >= args.warmup:
                            times[leg].append(ms)
                row = dict(corpus, nprobe=nprobe, nq=nq, result_checksum=int(out[legs[0]][1].sum().item()))
                if args.mode == "ab":
                    row["results_equal"] = bool(torch.equal(out["i8k"][1], out["fp16"][1]) and torch.equal(out["i8k"][0], out["fp16"][0]))
                for leg in legs:                          # the stages, in a pass of its own
                    ix.set_option("timing", 1)
                    call(leg)
                    s = ix.stats()
                    ix.set_option("timing", 0)
                    med = statistics.median(times[leg])
                    row[leg] = {"ms": med, "ms_min": min(times[leg]), "ms_max": max(times[leg]), "qps": nq / med * 1e3,
                                "prep_ms": s["last_prep_ms"], "scan_ms": s["last_scan_ms"], "tail_ms": s["last_tail_ms"], "path": s["last_path_name"],
                                "candidates_per_query": s["last_candidates"] / nq, "fallback_queries": s["last_fallback_queries"], "scan_dtype": s["scan_dtype"]}
                if args.mode == "ab":
                    row["speedup"] = row["fp16"]["ms"] / row["i8k"]["ms"]
                    row["scan_speedup"] = row["fp16"]["scan_ms"] / row["i8k"]["scan_ms"] if row["i8k"]["scan_ms"] > 0 else None
                result["legs"][f"{name}_nprobe{nprobe}_nq{nq}"] = row
        ix.close()
        del ix, Q
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

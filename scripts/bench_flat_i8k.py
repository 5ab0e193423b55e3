"""The int8 K-loop scan (option "i8_kloop") against the fp16 K-loop scan of the SAME handle ("panel_dtype" = 1), in one process.

s8-valued corpora (uniform integers -128..127) of --n rows x 384 and 768 dimensions, IP and L2, batches of 10 000, 64 and 1
integer queries, k = 10, everything device-resident.  Per (corpus, metric, batch) the two legs alternate call by call; each
figure is the median, the spread the min and max, over `steps` calls of the time between two device events after `warmup`
untimed rounds.  Per leg also: QPS, the scan kernels' time under option "timing" and their rate as a fraction of the dense int8
peak (5.0 POP/s; the fp16 leg against the same figure, for comparison only), candidates per query, scan_dtype.  Per corpus:
bytes resident over the float32 corpus with the copy and without, and whether the two legs return the same ids and distances
(result_checksum).  The result goes to --out (default profiles/r28_bench_flat_i8k.json) and is printed as one line.

    timeout -k 10 900 python scripts/bench_flat_i8k.py
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
BATCHES = (10_000, 64, 1)
INT8_PEAK = 5.0e15


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[384, 768])
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r28_bench_flat_i8k.json"))
    args = ap.parse_args()
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    result = {"n": args.n, "k": K, "steps": args.steps, "legs": {}}
    for d in args.dims:
        X = torch.randint(-128, 128, (args.n, d), generator=g, device=dev, dtype=torch.int32).float()
        Q = torch.randint(-128, 128, (max(BATCHES), d), generator=g, device=dev, dtype=torch.int32).float()
        for metric in ("ip", "l2"):
            plain = vdbhip.FlatIndex(d, metric, 0)
            plain.add_device(X.data_ptr(), args.n)
            bytes_plain = plain.stats()["bytes_resident"]
            del plain
            ix = vdbhip.FlatIndex(d, metric, 0)
            ix.set_option("i8_kloop", 1)
            ix.add_device(X.data_ptr(), args.n)
            torch.cuda.synchronize()
            st = ix.stats()
            assert st["has_i8_copy"] == 1, st
            corpus = {"bytes_over_corpus": st["bytes_resident"] / (args.n * d * 4), "bytes_over_corpus_option_off": bytes_plain / (args.n * d * 4)}
            for nq in BATCHES:
                out = {leg: (torch.empty((nq, K), device=dev), torch.empty((nq, K), device=dev, dtype=torch.int64)) for leg in ("i8k", "fp16")}
                times = {"i8k": [], "fp16": []}

                def call(leg):
                    ix.set_option("panel_dtype", 0 if leg == "i8k" else 1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ix.search_device(Q.data_ptr(), nq, K, out[leg][0].data_ptr(), out[leg][1].data_ptr())
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                for step in range(args.warmup + args.steps):
                    for leg in ("i8k", "fp16"):
                        ms = call(leg)
                        if step >= args.warmup:
                            times[leg].append(ms)
                row = {"result_checksum_equal": bool(torch.equal(out["i8k"][1], out["fp16"][1]) and torch.equal(out["i8k"][0], out["fp16"][0])),
                       "result_checksum": int(out["i8k"][1].sum().item())}
                for leg in ("i8k", "fp16"):             # the scan kernels' own time, in a pass of its own
                    ix.set_option("panel_dtype", 0 if leg == "i8k" else 1)
                    ix.set_option("timing", 1)
                    call(leg)
                    s = ix.stats()
                    ix.set_option("timing", 0)
                    med = statistics.median(times[leg])
                    qpad, dpad = (nq + 511) // 512 * 512, (d + 63) // 64 * 64
                    row[leg] = {"ms": med, "ms_min": min(times[leg]), "ms_max": max(times[leg]), "qps": nq / med * 1e3, "scan_ms": s["last_scan_ms"],
                                "scan_rate_of_int8_peak": 2.0 * args.n * dpad * qpad / (s["last_scan_ms"] * 1e-3) / INT8_PEAK if s["last_scan_ms"] > 0 else None,
                                "candidates_per_query": s["last_candidates"] / nq, "fallback_queries": s["last_fallback_queries"], "scan_dtype": s["scan_dtype"]}
                row["speedup"] = row["fp16"]["ms"] / row["i8k"]["ms"]
                result["legs"][f"{args.n}x{d}_{metric}_nq{nq}"] = {**corpus, **row}
            del ix
        del X, Q
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

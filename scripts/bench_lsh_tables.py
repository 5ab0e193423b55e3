"""Hash-table LSH (vdb_lsht_*) in the two configurations the reference publishes for its `lsh` slot, next to the exact flat
search and the sign-LSH Hamming scan of the same rows in the same run.

    --corpus random     the reference's `random` dataset, 20 000 x 64, its 256 selected queries
    --corpus gauss128   Gaussian 1M x 128, 10 000 queries (--n / --nq override)

Configurations, top-20: `l2` = L2 T12 / H4 / w 20, 64 x 20 = 1280 candidates; `cosine` = cosine T24 / H8, 128 x 20 = 2560
candidates (rows and queries normalised, inner-product index); no brute-force fallback.  Everything device-resident; every
figure is the median of `steps` searches timed one by one between two device synchronisations, after `warmup` untimed ones.
Per configuration: QPS of vdb_lsht_search_device, recall@10 against harness.ground_truth, the stage times the library records
(option "timing": prep = query keys + sample, scan = the vote scans, tail = select + re-rank), last_fallback_queries,
last_candidates, the candidate stage alone, and the scan's time per (pair x key word).  On an index of the same rows: the exact
flat search, and the 256-bit sign-LSH search with its scan time per (pair x code word) -- the yardstick the vote scan is held
against.  The result is merged under its corpus name into the JSON file --out (default profiles/r13_bench_lsh_tables.json)
and printed as one line.  One corpus per process; each GPU step under its own time limit:

    timeout -k 10 300 python scripts/bench_lsh_tables.py --corpus random && \\
    timeout -k 10 900 python scripts/bench_lsh_tables.py --corpus gauss128
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "vectordb-retrieval_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

K = 20
CONFIGS = {
    "l2": dict(metric="l2", num_tables=12, hash_size=4, bucket_width=20.0, seed=42, multiplier=64),
    "cosine": dict(metric="cosine", num_tables=24, hash_size=8, bucket_width=4.0, seed=42, multiplier=128),
}


def recall(exact, got, k):
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(exact, got)]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["random", "gauss128"], required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_bench_lsh_tables.json"))
    args = ap.parse_args()
    import torch

    import vdbhip
    from vdbhip import harness
    from vdbhip.algorithms import _safe_normalize
    from vdbhip.lsh_tables import make_tables

    dev = torch.device("cuda:0")
    if args.corpus == "random":
        from lsh_tables_cases import published_queries

        X, Q = published_queries(ROOT / "tests" / "golden")
    else:
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        X = torch.randn((args.n, 128), generator=g, device=dev, dtype=torch.float32).cpu().numpy()
        Q = torch.randn((args.nq, 128), generator=g, device=dev, dtype=torch.float32).cpu().numpy()
    n, d = X.shape
    nq = len(Q)
    stream = torch.cuda.current_stream().cuda_stream
    D_t = torch.empty((nq, K), dtype=torch.float32, device=dev)
    I_t = torch.empty((nq, K), dtype=torch.int64, device=dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def stages(idx, fn):
        idx.set_option("timing", 1)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        st = idx.stats()
        idx.set_option("timing", 0)
        return st

    res = {"config": f"{args.corpus}: {n} x {d}, {nq} queries, top-{K}, median of {args.steps}"}
    for name in args.configs:
        c = CONFIGS[name]
        cos = c["metric"] == "cosine"
        rows, qs = (_safe_normalize(X.copy()), _safe_normalize(Q.copy())) if cos else (X, Q)
        Q_t = torch.from_numpy(qs).to(dev)
        gt = harness.ground_truth(rows, qs, k=K, metric="ip" if cos else "l2")
        P, b = make_tables(d, c["num_tables"], c["hash_size"], c["metric"], c["bucket_width"], c["seed"])
        ncand = K * c["multiplier"]
        words = c["num_tables"] * (c["hash_size"] if b is not None else (c["hash_size"] + 31) // 32)
        idx = vdbhip.FlatIndex(d, "ip" if cos else "l2", 0)
        idx.lsht_set_tables(P, b, c["bucket_width"] if b is not None else 0.0)
        t0 = time.perf_counter()
        idx.add(rows)
        build_s = time.perf_counter() - t0
        r = {"tables": f"T{c['num_tables']} / H{c['hash_size']}" + (f" / w{c['bucket_width']:g}" if b is not None else ""),
             "candidates": ncand, "key_words": words, "build_s": round(build_s, 2)}
        exact_ms = timed(lambda: idx.search_device(Q_t.data_ptr(), nq, K, D_t.data_ptr(), I_t.data_ptr(), stream))
        r["exact_flat"] = {"ms_per_search": round(exact_ms, 3), "qps": round(nq / exact_ms * 1e3, 1),
                           "recall@10": round(recall(gt, I_t.cpu().numpy(), 10), 6)}
        search = lambda: idx.lsht_search_device(Q_t.data_ptr(), nq, K, ncand, False, D_t.data_ptr(), I_t.data_ptr(), stream)  # noqa: E731
        ms = timed(search)
        got = I_t.cpu().numpy()
        st = stages(idx, search)
        r.update({"ms_per_search": round(ms, 3), "qps": round(nq / ms * 1e3, 1), "recall@10": round(recall(gt, got, 10), 6),
                  "recall@1": round(recall(gt, got, 1), 6), "prep_ms": round(st["last_prep_ms"], 3),
                  "scan_ms": round(st["last_scan_ms"], 3), "tail_ms": round(st["last_tail_ms"], 3),
                  "fallback_queries": st["last_fallback_queries"], "candidates_rescored": st["last_candidates"],
                  "scan_ps_per_pair_word": round(st["last_scan_ms"] * 1e9 / (float(nq) * n * words), 4)})
        v_t = torch.empty((nq, ncand), dtype=torch.int32, device=dev)
        c_t = torch.empty((nq, ncand), dtype=torch.int64, device=dev)
        r["candidates_ms"] = round(timed(lambda: idx.lsht_candidates_device(Q_t.data_ptr(), nq, ncand, v_t.data_ptr(), c_t.data_ptr(),
                                                                            stream)), 3)
        r["colliding_rows_at_least"] = int((c_t >= 0).sum(dim=1).min().item())
        st = idx.stats()
        r["bytes_resident"], r["bytes_workspace"] = st["bytes_resident"], st["bytes_workspace"]
        idx.close()
        # the yardstick: the Hamming scan of 256-bit sign codes (8 words) over the same rows, same candidate count
        ham = vdbhip.FlatIndex(d, "ip" if cos else "l2", 0)
        ham.lsh_set_projection(vdbhip.make_projection(d, 256, 0))
        ham.add(rows)
        hsearch = lambda: ham.lsh_search_device(Q_t.data_ptr(), nq, K, ncand, D_t.data_ptr(), I_t.data_ptr(), stream)  # noqa: E731
        hms = timed(hsearch)
        hst = stages(ham, hsearch)
        r["sign_lsh_256"] = {"ms_per_search": round(hms, 3), "scan_ms": round(hst["last_scan_ms"], 3),
                             "recall@10": round(recall(gt, I_t.cpu().numpy(), 10), 6),
                             "scan_ps_per_pair_word": round(hst["last_scan_ms"] * 1e9 / (float(nq) * n * 8), 4)}
        r["scan_per_pair_word_over_hamming"] = round(r["scan_ps_per_pair_word"] / max(r["sign_lsh_256"]["scan_ps_per_pair_word"], 1e-12), 3)
        ham.close()
        res[name] = r
    out = Path(args.out)
    allres = json.loads(out.read_text()) if out.exists() else {}
    allres[args.corpus] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(allres, indent=1) + "\n")
    print(json.dumps({args.corpus: res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

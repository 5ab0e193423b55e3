"""k-NN graph index (degree 32, 64 candidates) against the exact flat search of the same handle, on one corpus.

    --corpus gauss128   Gaussian 1M x 128, l2
    --corpus unit768    unit vectors 2M x 768, ip (the embedding shape; --n overrides the rows)

10 000 queries, k = 10, beams ef 32 / 100 / 256.  Everything device-resident (queries and results in HBM); every search figure
is the median of `steps` searches timed one by one between two device synchronisations, after `warmup` untimed ones.  Reported:
the build time of vdb_knng_build, split into the self-search (the same blocks of rows sent through vdb_search_partial_device
with k = ncand + 1, timed on their own) and the rest (strip + prune: build minus self-search); per ef the QPS of
vdb_knng_search_device, recall@10 against the exact search of the same handle in the same run, rows scored per query, the three
stage times the library records (option "timing": prep = entry scoring, scan = the traversal, tail = writing results); the exact
search's QPS; bytes resident over corpus bytes.  The result is merged under its corpus name into the JSON file --out (default
profiles/r11_bench_knng.json) and printed as one line.  One corpus per process; each GPU step under its own time limit:

    timeout -k 10 900 python scripts/bench_knng.py --corpus gauss128 && \\
    timeout -k 10 1100 python scripts/bench_knng.py --corpus unit768
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
for p in (str(ROOT), str(ROOT / "vectordb-retrieval_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

K, DEGREE, NCAND, BUILD_BLOCK = 10, 32, 64, 65536


def recall(exact, got, k):
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(exact, got)]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["gauss128", "unit768"], required=True)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--efs", type=int, nargs="+", default=[32, 100, 256])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11_bench_knng.json"))
    args = ap.parse_args()
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    d, metric = (128, "l2") if args.corpus == "gauss128" else (768, "ip")
    n = args.n or (1_000_000 if args.corpus == "gauss128" else 2_000_000)
    nq = args.nq
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X_t = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    Q_t = torch.randn((nq, d), generator=g, device=dev, dtype=torch.float32)
    if args.corpus == "unit768":
        X_t /= X_t.norm(dim=1, keepdim=True)
        Q_t /= Q_t.norm(dim=1, keepdim=True)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    idx = vdbhip.KnnGraphIndex(d, metric, 0)
    idx.add_device(X_t.data_ptr(), n, 0, stream)
    torch.cuda.synchronize()
    idx.set_option("knng_build_block", BUILD_BLOCK)
    # the self-search of the build on its own: the same blocks, the same k (one untimed block first sizes the workspace)
    kk = min(NCAND + 1, n)
    keys_t = torch.empty((BUILD_BLOCK, kk), dtype=torch.float64, device=dev)
    ids_t = torch.empty((BUILD_BLOCK, kk), dtype=torch.int64, device=dev)

    def self_search():
        for r0 in range(0, n, BUILD_BLOCK):
            nb = min(BUILD_BLOCK, n - r0)
            idx.search_partial_device(X_t[r0:r0 + nb].data_ptr(), nb, kk, keys_t.data_ptr(), ids_t.data_ptr(), stream)

    idx.search_partial_device(X_t.data_ptr(), min(BUILD_BLOCK, n), kk, keys_t.data_ptr(), ids_t.data_ptr(), stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    self_search()
    torch.cuda.synchronize()
    self_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    idx.knng_build(DEGREE, NCAND)
    build_s = time.perf_counter() - t0
    del keys_t, ids_t
    res = {"config": f"{args.corpus}: {n} x {d}, {nq} queries, k={K}, {metric}, degree {DEGREE}, ncand {NCAND}, median of {args.steps}",
           "build_s": round(build_s, 2), "build_self_search_s": round(self_s, 2), "build_strip_prune_s": round(build_s - self_s, 2)}
    D_t = torch.empty((nq, K), dtype=torch.float32, device=dev)
    I_t = torch.empty((nq, K), dtype=torch.int64, device=dev)
    ms = timed(lambda: idx.search_device(Q_t.data_ptr(), nq, K, D_t.data_ptr(), I_t.data_ptr(), stream))
    exact = I_t.cpu().numpy().copy()
    res["exact_flat"] = {"ms_per_search": round(ms, 3), "qps": round(nq / ms * 1e3, 1)}
    for ef in args.efs:
        search = lambda: idx.knng_search_device(Q_t.data_ptr(), nq, K, ef, D_t.data_ptr(), I_t.data_ptr(), stream)  # noqa: E731
        ms = timed(search)
        got = I_t.cpu().numpy().copy()
        st = idx.stats()
        r = {"ef": ef, "ms_per_search": round(ms, 3), "qps": round(nq / ms * 1e3, 1), "recall@10": round(recall(exact, got, K), 6),
             "recall@1": round(recall(exact, got, 1), 6), "rows_scored_per_query": round(st["last_candidates"] / nq, 1),
             "capped_queries": st["last_fallback_queries"], "qps_over_exact": round(res["exact_flat"]["ms_per_search"] / ms, 3)}
        idx.set_option("timing", 1)
        for _ in range(args.steps):
            search()
        torch.cuda.synchronize()
        st = idx.stats()
        idx.set_option("timing", 0)
        r.update({"prep_ms": round(st["last_prep_ms"], 3), "scan_ms": round(st["last_scan_ms"], 3), "tail_ms": round(st["last_tail_ms"], 3)})
        res[f"ef{ef}"] = r
    st = idx.stats()
    res["bytes_resident"] = st["bytes_resident"]
    res["bytes_workspace"] = st["bytes_workspace"]
    res["graph_bytes"] = n * DEGREE * 4
    res["resident_over_fp32_corpus"] = round((st["bytes_resident"] - st["bytes_workspace"]) / (4.0 * n * d), 4)
    idx.close()
    out = Path(args.out)
    allres = json.loads(out.read_text()) if out.exists() else {}
    allres[args.corpus] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(allres, indent=1) + "\n")
    print(json.dumps({args.corpus: res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Sign-LSH (256 bits) + exact re-rank against the exact flat search and a plain torch candidate stage, on one corpus.

    --corpus gauss128   Gaussian 1M x 128, l2
    --corpus unit768    unit vectors 2M x 768, l2 (the embedding shape; --n overrides the rows)

10 000 queries, k = 10, candidate multipliers 8 and 64 (80 / 640 candidates).  Everything device-resident (queries and
results in HBM); every figure is the median of `steps` searches timed one by one between two device synchronisations, after
`warmup` untimed ones.  Per multiplier: QPS of vdb_lsh_search_device, recall@10 against harness.ground_truth, the three
stage times the library records (option "timing": prep = query codes + sample, scan = the two Hamming scans, tail = select +
re-rank), the candidate stage alone (vdb_lsh_candidates_device), the re-rank alone, and the torch baseline of the candidate
stage on the same codes: +-1 fp16 matrices, Q @ X.T in query chunks, torch.topk(c).  On the same index: the exact
FlatIndex search, and bytes_resident.  The result is merged under its corpus name into the JSON file --out (default
profiles/r06_bench_lsh.json) and printed as one line; the exit status is 1 if the library's candidate stage is slower than
the torch baseline.  One corpus per process; each GPU step under its own time limit:

    timeout -k 10 900 python scripts/bench_lsh.py --corpus gauss128 && \\
    timeout -k 10 900 python scripts/bench_lsh.py --corpus unit768 && \\
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d build/lsh_trace -o lsh -- \\
        python scripts/bench_lsh.py --corpus gauss128 --steps 3 --no-baseline --out build/lsh_trace/bench.json
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

NBITS, K = 256, 10


def recall(exact, got, k):
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(exact, got)]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["gauss128", "unit768"], required=True)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--multipliers", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r06_bench_lsh.json"))
    args = ap.parse_args()
    import torch

    import vdbhip
    from vdbhip import harness

    dev = torch.device("cuda:0")
    d = 128 if args.corpus == "gauss128" else 768
    n = args.n or (1_000_000 if args.corpus == "gauss128" else 2_000_000)
    nq = args.nq
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X_t = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    Q_t = torch.randn((nq, d), generator=g, device=dev, dtype=torch.float32)
    if args.corpus == "unit768":
        X_t /= X_t.norm(dim=1, keepdim=True)
        Q_t /= Q_t.norm(dim=1, keepdim=True)
    X, Q = X_t.cpu().numpy(), Q_t.cpu().numpy()
    del X_t
    gt = harness.ground_truth(X, Q, k=K, metric="l2")

    def timed(fn, steps=args.steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    idx = vdbhip.FlatIndex(d, "l2", 0)
    idx.lsh_set_projection(vdbhip.make_projection(d, NBITS, 0))
    t0 = time.perf_counter()
    idx.add(X)
    build_s = time.perf_counter() - t0
    del X
    stream = torch.cuda.current_stream().cuda_stream
    D_t = torch.empty((nq, K), dtype=torch.float32, device=dev)
    I_t = torch.empty((nq, K), dtype=torch.int64, device=dev)
    res = {"config": f"{args.corpus}: {n} x {d}, {nq} queries, k={K}, l2, {NBITS} bits, median of {args.steps}",
           "build_s": round(build_s, 2)}
    ms = timed(lambda: idx.search_device(Q_t.data_ptr(), nq, K, D_t.data_ptr(), I_t.data_ptr(), stream))
    res["exact_flat"] = {"ms_per_search": round(ms, 3), "qps": round(nq / ms * 1e3, 1),
                         "recall@10": round(recall(gt, I_t.cpu().numpy(), K), 6)}
    if not args.no_baseline:      # +-1 fp16 operands of the torch baseline, from the library's own codes
        shifts = torch.arange(32, device=dev, dtype=torch.int64)

        def pm1(codes_np):
            c = torch.from_numpy(codes_np.astype(np.int64)).to(dev)
            bits = (c.unsqueeze(-1) >> shifts) & 1
            return (bits.reshape(c.shape[0], -1) * 2 - 1).to(torch.float16)

        B = pm1(idx.lsh_codes())
        probe = vdbhip.FlatIndex(d, "l2", 0)                  # the query codes: a second index over the queries
        probe.lsh_set_projection(vdbhip.make_projection(d, NBITS, 0))
        probe.add(Q)
        A = pm1(probe.lsh_codes())
        probe.close()
        chunk = max(1, min(nq, (2 << 30) // (2 * n)))         # <= 2 GiB of fp16 scores per chunk
    ok = True
    for mult in args.multipliers:
        c = K * mult
        ham_t = torch.empty((nq, c), dtype=torch.int32, device=dev)
        ids_t = torch.empty((nq, c), dtype=torch.int64, device=dev)
        search = lambda: idx.lsh_search_device(Q_t.data_ptr(), nq, K, c, D_t.data_ptr(), I_t.data_ptr(), stream)  # noqa: E731
        ms = timed(search)
        idx.set_option("timing", 1)
        for _ in range(args.steps):
            search()
        torch.cuda.synchronize()
        st = idx.stats()
        idx.set_option("timing", 0)
        r = {"candidates": c, "ms_per_search": round(ms, 3), "qps": round(nq / ms * 1e3, 1),
             "recall@10": round(recall(gt, I_t.cpu().numpy(), K), 6),
             "prep_ms": round(st["last_prep_ms"], 3), "scan_ms": round(st["last_scan_ms"], 3),
             "tail_ms": round(st["last_tail_ms"], 3), "fallback_queries": st["last_fallback_queries"]}
        cand_ms = timed(lambda: idx.lsh_candidates_device(Q_t.data_ptr(), nq, c, ham_t.data_ptr(), ids_t.data_ptr(), stream))
        r["candidates_ms"] = round(cand_ms, 3)
        r["rerank_ms"] = round(timed(lambda: idx.rerank_device(Q_t.data_ptr(), nq, ids_t.data_ptr(), c, K, D_t.data_ptr(),
                                                               I_t.data_ptr(), stream)), 3)
        if not args.no_baseline:
            def torch_candidates():
                out = []
                for q0 in range(0, nq, chunk):
                    out.append(torch.topk(A[q0:q0 + chunk] @ B.T, c, dim=1).indices)
                return out

            got = torch.cat(torch_candidates()).cpu().numpy()
            lib = ids_t.cpu().numpy()
            # (the same candidates up to the choice among equal distances at the cut: mean overlap of the first 64 queries)
            r["torch_overlap"] = round(float(np.mean([len(set(a) & set(b)) for a, b in zip(got[:64], lib[:64])])) / c, 4)
            tms = timed(torch_candidates)
            r["torch_candidates_ms"] = round(tms, 3)
            r["torch_over_library"] = round(tms / cand_ms, 3)
            ok = ok and tms >= cand_ms
        res[f"multiplier{mult}"] = r
    st = idx.stats()
    res["bytes_resident"] = st["bytes_resident"]
    res["bytes_workspace"] = st["bytes_workspace"]
    res["resident_over_fp32_corpus"] = round((st["bytes_resident"] - st["bytes_workspace"]) / (4.0 * n * d), 4)
    idx.close()
    out = Path(args.out)
    allres = json.loads(out.read_text()) if out.exists() else {}
    allres[args.corpus] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(allres, indent=1) + "\n")
    print(json.dumps({args.corpus: res}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

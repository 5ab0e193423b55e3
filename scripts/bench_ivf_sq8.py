"""IVF1024,SQ8 vs IVF1024,Flat on the same centroids: QPS, recall@10 and resident footprint.

Gaussian 1M x 128 corpus (non-integer values: IVF-Flat takes its fp16 list scan), 10 000 Gaussian queries, k = 10, l2.
The IVF-Flat index trains the centroids (the library's k-means, 25 iterations, seed 1234); the SQ8 index gets the same
centroids and trains its ranges on the corpus.  Per nprobe: device-resident QPS timed as bench.py's IVF legs (queries and
results in HBM, `warmup` untimed searches, then `steps` timed ones between two device synchronisations), recall@10 against
the exact float64 result, and (bytes_resident - bytes_workspace) / (4 N D).  Prints ONE JSON line.

`--direct`: also the legs of option "ivf_sq8_direct" (the list scan reads the codes themselves) on the SAME SQ8 handle, alternating
option 0 / 1 twice per (batch, nprobe) in one run -- batches of `--nq`, 64 and 1 queries; every leg with its stage times, scan_dtype
(2: fp16 panels made per batch, 4: the direct scan), fallback queries, and the workspace bytes of a handle searched with the option on only.

`--kloop`: instead, the D > 128 legs of option "ivf_sq8_kloop" (kloop_legs below).

    python scripts/bench_ivf_sq8.py [--steps 5] [--warmup 2] [--n 1000000] [--direct | --kloop]
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


def kloop_legs(args) -> None:
    """`--kloop`: option "ivf_sq8_kloop" at D > 128.  Two shapes -- IVF256,SQ8 at nprobe 24 over 1M x 768 Gaussian rows (the
    reference's ivf_sq8 configuration at its msmarco dimension) and IVF100,SQ8 at nprobe 32 over 100 000 x 384 -- with batches of 1, 64
    and 10 000 queries, k = 10, l2.  The centroids are the first nlist rows.  Per leg, alternating twice on the same handle: the K-loop
    scan of the codes against `force_path` = 1 (the exact list scan: what every batch took before the option existed); as a yardstick an
    IVF-Flat handle over the decoded rows on its fp16 K-loop scan.  Recorded: per-call time, stage times, scan_dtype, fallback queries,
    bytes resident, and the add time with the option 0 and 1.  Prints ONE JSON line."""
    import torch

    import vdbhip

    dev = torch.device("cuda:0")
    k = 10
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for n, d, nlist, nprobe in ((args.n, 768, 256, 24), (100_000, 384, 100, 32)):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        X = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32).cpu().numpy()
        Q_t = torch.randn((args.nq, d), generator=g, device=dev, dtype=torch.float32)
        D_t = torch.empty((args.nq, k), dtype=torch.float32, device=dev)
        I_t = torch.empty((args.nq, k), dtype=torch.int64, device=dev)
        C = X[:nlist].copy()
        add_s, handles = {}, {}
        for on in (0, 1):
            ix = vdbhip.IVFSQ8Index(d, nlist, "l2", 0, direct_kloop=bool(on))
            ix.set_centroids(C)
            ix.train_ranges(X)
            t0 = time.perf_counter()
            ix.add(X)
            add_s[f"option{on}"] = round(time.perf_counter() - t0, 3)
            handles[on] = ix
        # (right after the add, before any search has sized the per-batch plan and workspace buffers: what the index itself holds)
        resident = {f"option{on}": (lambda s: s["bytes_resident"] - s["bytes_workspace"])(handles[on].stats()) for on in (0, 1)}
        sq = handles[1]
        lor, (vmin, vdiff) = sq.assignment(), sq.ranges()
        Xh = C[lor] + (vmin + ((sq.codes().astype(np.float32) + np.float32(0.5)) / np.float32(255)) * vdiff)
        handles[0].close()
        fl = vdbhip.IVFFlatIndex(d, nlist, "l2", 0)
        fl.set_centroids(C)
        fl.add(Xh, list_of_row=lor)
        resident["ivf_flat_decoded"] = (lambda s: s["bytes_resident"] - s["bytes_workspace"])(fl.stats())
        del Xh

        def leg(idx, nq, force):
            idx.set_option("force_path", force)
            idx.set_nprobe(nprobe)
            for _ in range(args.warmup):
                idx.search_device(Q_t.data_ptr(), nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            idx.set_option("timing", 1)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                idx.search_device(Q_t.data_ptr(), nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            st = idx.stats()
            idx.set_option("timing", 0)
            idx.set_option("force_path", 0)
            return {"ms_per_search": round(el / args.steps * 1e3, 4), "prep_ms": round(st["last_prep_ms"], 4), "scan_ms": round(st["last_scan_ms"], 4),
                    "tail_ms": round(st["last_tail_ms"], 4), "scan_dtype": st["scan_dtype"], "fallback_queries": st["last_fallback_queries"],
                    "ids": I_t[:nq].cpu().numpy().copy()}

        res = {"add_s": add_s}
        for nq in (1, 64, args.nq):
            legs = [leg(sq, nq, force) for force in (0, 1, 0, 1)]
            flat = leg(fl, nq, 0)
            same = all(np.array_equal(flat["ids"], x.pop("ids")) for x in legs + [flat])
            res[f"nq{nq}"] = {"kloop": legs[0::2], "exact": legs[1::2], "ivf_flat_decoded": flat, "same_ids": same}
        res["bytes_resident_after_add"] = resident
        out[f"IVF{nlist},SQ8 {n}x{d} nprobe{nprobe}"] = res
        sq.close()
        fl.close()
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kloop", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--direct", action="store_true")
    args = ap.parse_args()
    if args.kloop:
        return kloop_legs(args)
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
    D_t = torch.empty((args.nq, k), dtype=torch.float32, device=dev)
    I_t = torch.empty((args.nq, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"config": f"Gaussian {args.n} x {d}, {args.nq} queries, k={k}, l2; IVF{nlist} (own k-means, the same centroids "
                     f"for Flat and SQ8)", "build_s": {"flat": round(t_fl, 2), "sq8": round(t_sq, 2)}}
    for name, idx in (("flat", fl), ("sq8", sq)):
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
    if args.direct:
        def leg(nq, p, on):
            sq.set_option("ivf_sq8_direct", on)
            sq.set_nprobe(p)
            for _ in range(args.warmup):
                sq.search_device(Q_t.data_ptr(), nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            sq.set_option("timing", 1)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                sq.search_device(Q_t.data_ptr(), nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            st = sq.stats()
            sq.set_option("timing", 0)
            return {"qps": round(nq * args.steps / el, 1), "ms_per_search": round(el / args.steps * 1e3, 4), "prep_ms": round(st["last_prep_ms"], 4),
                    "scan_ms": round(st["last_scan_ms"], 4), "tail_ms": round(st["last_tail_ms"], 4), "scan_dtype": st["scan_dtype"],
                    "fallback_queries": st["last_fallback_queries"], "candidates_per_query": round(st["last_candidates"] / nq, 2),
                    "ids": I_t[:nq].cpu().numpy().copy()}

        direct = {}
        for nq in (args.nq, 64, 1):
            for p in args.nprobe:
                legs = [leg(nq, p, on) for on in (0, 1, 0, 1)]
                same = all(np.array_equal(legs[0]["ids"], x.pop("ids")) for x in legs[::-1])
                direct[f"nq{nq}_nprobe{p}"] = {"off": legs[0::2], "on": legs[1::2], "same_ids": same}
        fresh = vdbhip.IVFSQ8Index(d, nlist, "l2", 0, direct_codes=True)       # searched with the option on only: no panel slab
        fresh.set_centroids(fl.centroids())
        fresh.train_ranges(X)
        fresh.add(X)
        fresh.set_nprobe(32)
        fresh.search_device(Q_t.data_ptr(), args.nq, k, D_t.data_ptr(), I_t.data_ptr(), stream)
        torch.cuda.synchronize()
        direct["bytes_workspace"] = {"on_only": fresh.stats()["bytes_workspace"], "after_both": sq.stats()["bytes_workspace"]}
        fresh.close()
        out["sq8_direct"] = direct
    print(json.dumps(out))
    fl.close()
    sq.close()


if __name__ == "__main__":
    main()

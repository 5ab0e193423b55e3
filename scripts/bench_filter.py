"""Filtered k-NN search (vdb_search_filtered_device) against the unfiltered search of the same handle and a torch baseline.

    --corpus gauss128   Gaussian 1M x 128, l2 (fp16 scan)
    --corpus bytes128   byte-valued 1M x 128, l2 (integers 0..255 and integer queries: the int8 scan)
    --corpus unit384    unit vectors 1M x 384, ip (K-loop scan)

Everything is device-resident; k = 10.  Every figure is the median over `steps` calls of the time between two device events, after
`warmup` untimed rounds, and the calls of a leg alternate step by step inside the same run.  Four tables per corpus (--tables):

  masked    the masked scan route (option "force_path" = 2) at densities 1.0 / 0.5 / 0.1 / 0.01, 10 000 queries and 1 query, next to
            vdb_search_device of the same handle and `Q @ X[rows].T` + topk in torch (the gathered rows are made outside the timing);
            and, in a pass of their own under option "timing", the three stage times of the filtered and the unfiltered search
  install   vdb_filter_set (host words) and vdb_filter_set_device, wall clock of the call, at densities 0.5 / 0.01 / 0.001 on both
            handles of the sparse table -- with and without the list of admitted rows, `keeps_list` read from the bytes the handle
            reports -- at this corpus size (and, density 0.5, at --install-n rows)
  contiguous  both routes on one run of 5 000 / 50 000 consecutive rows (fewer than k live superbins: the masked scan's queries may take
            the exhaustive fallback), 1 / 64 / 10 000 queries
  order     one query at densities 1.0 / 0.5: the filtered and the unfiltered call alternating in both orders, without the torch
            leg and with it in front of either
  sparse    the sparse route (option "filter_sparse_pairs" = inf) against the masked scan route (= 0, "force_path" = 2) on the same
            filter, two handles over the same rows: n_allowed = 1e2 .. 1e6 in decades x 1, 64, 10 000 queries; per batch size the
            crossover is the largest measured pair count at which the sparse route is still the faster one

The result is merged under its corpus name into the JSON file --out (default profiles/r21_bench_filter.json) and printed as one line.
One corpus per process, each under its own time limit:

    timeout -k 10 500 python scripts/bench_filter.py --corpus gauss128 && \\
    timeout -k 10 500 python scripts/bench_filter.py --corpus bytes128 && \\
    timeout -k 10 500 python scripts/bench_filter.py --corpus unit384
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

K = 10
DENSITIES = (1.0, 0.5, 0.1, 0.01)
ALLOWED = (100, 1_000, 10_000, 100_000, 1_000_000)
BATCHES = (1, 64, 10_000)
TORCH_MAX_SCORES = 1 << 30          # elements of one Q-block @ X[rows].T


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["gauss128", "bytes128", "unit384"], required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--install-n", type=int, default=0, help="a second corpus size for the install table (e.g. 12500000)")
    ap.add_argument("--tables", default="masked,install,order,sparse,contiguous", help="which tables to measure; the others keep what --out holds")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r21_bench_filter.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import vdbhip
    from vdbhip import _ffi

    tables = set(args.tables.split(","))
    dev = torch.device("cuda:0")
    n, nq_max = args.n, max(BATCHES)
    d, metric = (384, "ip") if args.corpus == "unit384" else (128, "l2")
    g = torch.Generator(device=dev)
    g.manual_seed(0)

    def rows(count):
        if args.corpus == "bytes128":
            return torch.clamp(torch.round(torch.empty((count, d), device=dev).exponential_(1.0 / 30.0, generator=g)), 0, 255)
        x = torch.randn((count, d), generator=g, device=dev, dtype=torch.float32)
        return x / x.norm(dim=1, keepdim=True) if args.corpus == "unit384" else x

    X_t, Q_t = rows(n), rows(nq_max)
    stream = torch.cuda.current_stream().cuda_stream

    def handle(force, pairs, x=X_t):
        idx = vdbhip.FlatIndex(d, metric, 0)
        idx.add_device(x.data_ptr(), x.shape[0], 0, stream)
        torch.cuda.synchronize()
        idx.set_option("force_path", force)
        idx.set_option("filter_sparse_pairs", pairs)
        return idx

    idx_scan, idx_sparse = handle(2, 0.0), handle(0, float("inf"))
    built = idx_scan.stats()
    Dk = torch.empty((nq_max, K), dtype=torch.float32, device=dev)
    Ik = torch.empty((nq_max, K), dtype=torch.int64, device=dev)
    Dk2, Ik2 = torch.empty_like(Dk), torch.empty_like(Ik)
    xn2 = (X_t * X_t).sum(dim=1) if metric == "l2" else None
    rng = np.random.default_rng(0)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def alternate(calls):
        times = {c: [] for c in calls}
        for step in range(args.warmup + args.steps):
            for c, fn in calls.items():
                ms = event_ms(fn)
                if step >= args.warmup:
                    times[c].append(ms)
        return {c: statistics.median(v) for c, v in times.items()}

    def filtered(idx, nq, D=Dk, I=Ik):
        idx.search_filtered_device(Q_t.data_ptr(), nq, K, D.data_ptr(), I.data_ptr(), stream)

    def unfiltered(idx, nq):
        idx.search_device(Q_t.data_ptr(), nq, K, Dk2.data_ptr(), Ik2.data_ptr(), stream)

    def torch_topk(nq, X_sub, xn2_sub):
        block = max(1, min(nq, TORCH_MAX_SCORES // max(1, X_sub.shape[0])))
        for q0 in range(0, nq, block):
            Q = Q_t[q0:q0 + block]
            s = Q @ X_sub.T
            if metric == "l2":
                s = (Q * Q).sum(dim=1, keepdim=True) - 2.0 * s + xn2_sub[None]
            torch.topk(s, min(K, X_sub.shape[0]), dim=1, largest=metric != "l2")

    # ---- masked scan route against the unfiltered search ----------------------------------------------------------------------------
    masked = {}
    for dens in DENSITIES if "masked" in tables else ():
        mask = np.ones(n, np.bool_) if dens == 1.0 else rng.random(n) < dens
        sel = torch.from_numpy(np.flatnonzero(mask)).to(dev)
        X_sub = X_t[sel]
        xn2_sub = xn2[sel] if xn2 is not None else None
        idx_scan.set_filter(mask)
        for nq in (10_000, 1):
            t = alternate({"filtered": lambda: filtered(idx_scan, nq), "unfiltered": lambda: unfiltered(idx_scan, nq),
                           "torch": lambda: torch_topk(nq, X_sub, xn2_sub)})
            st = idx_scan.stats()
            masked[f"density{dens:g}_nq{nq}"] = {
                "nq": nq, "density": dens, "n_allowed": int(mask.sum()), "filtered_ms": t["filtered"], "unfiltered_ms": t["unfiltered"],
                "torch_ms": t["torch"], "filtered_over_unfiltered": t["filtered"] / t["unfiltered"],
                "last_path": st["last_path_name"]}
        del X_sub, sel
    # the stage times, in a pass of their own: setting option "timing" restarts the recording window (and, like every option,
    # drops the filter, which is installed again behind it)
    for dens in DENSITIES if "masked" in tables else ():
        mask = np.ones(n, np.bool_) if dens == 1.0 else np.random.default_rng(1).random(n) < dens
        for nq in (10_000, 1):
            leg = masked[f"density{dens:g}_nq{nq}"]
            for name, fn in (("filtered", lambda: filtered(idx_scan, nq)), ("unfiltered", lambda: unfiltered(idx_scan, nq))):
                idx_scan.set_option("timing", 1)
                idx_scan.set_filter(mask)
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                st = idx_scan.stats()
                leg[name + "_stages"] = {"prep_ms": st["last_prep_ms"], "scan_ms": st["last_scan_ms"], "tail_ms": st["last_tail_ms"]}
    idx_scan.set_option("timing", 0)

    # ---- install ----------------------------------------------------------------------------------------------------------------------
    # Whether an install also builds the list of admitted rows (count, prefix, emit) depends on the handle's option
    # "filter_sparse_pairs" and on the admitted count; `keeps_list` is read from the handle: the bytes the install added against
    # the bytes of words + count + masked bias copies alone.
    def install_times(idx, count, density, label):
        mask = np.random.default_rng(2).random(count) < density
        words = _ffi.pack_allow_bits(mask, count)
        w_t = torch.from_numpy(words.view(np.int32)).to(dev)
        idx.clear_filter()
        st0 = idx.stats()
        span = 1024 if d > 128 else 512
        npad = (count + span - 1) // span * span
        no_list = npad // 8 + 8 + npad * 4 + (2 * npad * 4 if st0["has_i8_copy"] else 0)
        host, device = [], []
        for step in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _ffi.check(idx._lib.vdb_filter_set(idx._handle(), _ffi.ptr(words), count))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            idx.set_filter_device(w_t.data_ptr(), count, stream)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if step >= args.warmup:
                host.append((t1 - t0) * 1e3)
                device.append((t2 - t1) * 1e3)
        added = idx.stats()["bytes_resident"] - st0["bytes_resident"]
        return {"handle": label, "rows": count, "density": density, "n_allowed": int(mask.sum()), "filter_count": idx.filter_count,
                "host_words_ms": statistics.median(host), "device_words_ms": statistics.median(device),
                "bytes_added": int(added), "bytes_without_list": int(no_list), "keeps_list": bool(added > no_list)}

    install = []
    if "install" in tables:
        for idx, label in ((idx_scan, "filter_sparse_pairs=0"), (idx_sparse, "filter_sparse_pairs=inf")):
            for density in (0.5, 0.01, 0.001):
                install.append(install_times(idx, n, density, label))

    # ---- one query, the order of the calls ------------------------------------------------------------------------------------------
    # the alternation of the masked table puts the filtered call behind the torch baseline and the unfiltered call behind the
    # filtered one; here the same two calls alternate without the torch leg, in both orders, and with the torch leg in front of the
    # unfiltered call instead
    order = {}
    if "order" in tables:
        for dens in (1.0, 0.5):
            mask = np.ones(n, np.bool_) if dens == 1.0 else np.random.default_rng(3).random(n) < dens
            sel = torch.from_numpy(np.flatnonzero(mask)).to(dev)
            X_sub = X_t[sel]
            xn2_sub = xn2[sel] if xn2 is not None else None
            idx_scan.set_filter(mask)
            f, u, t = (lambda: filtered(idx_scan, 1)), (lambda: unfiltered(idx_scan, 1)), (lambda: torch_topk(1, X_sub, xn2_sub))
            order[f"density{dens:g}"] = {"filtered_then_unfiltered": alternate({"filtered": f, "unfiltered": u}),
                                         "unfiltered_then_filtered": alternate({"unfiltered": u, "filtered": f}),
                                         "torch_filtered_unfiltered": alternate({"torch": t, "filtered": f, "unfiltered": u}),
                                         "torch_unfiltered_filtered": alternate({"torch": t, "unfiltered": u, "filtered": f})}
            del X_sub, sel

    # ---- sparse route against the masked scan route -------------------------------------------------------------------------------------
    sparse = {}
    for n_allowed in ALLOWED if "sparse" in tables else ():
        if n_allowed > n:
            continue
        mask = np.zeros(n, np.bool_)
        mask[rng.choice(n, n_allowed, replace=False)] = True
        idx_scan.set_filter(mask)
        idx_sparse.set_filter(mask)
        for nq in BATCHES:
            t = alternate({"sparse": lambda: filtered(idx_sparse, nq), "masked": lambda: filtered(idx_scan, nq, Dk2, Ik2)})
            torch.cuda.synchronize()
            same = bool(torch.equal(Ik[:nq], Ik2[:nq]) and torch.equal(Dk[:nq], Dk2[:nq]))
            sparse[f"allowed{n_allowed}_nq{nq}"] = {
                "nq": nq, "n_allowed": n_allowed, "pairs": nq * n_allowed, "sparse_ms": t["sparse"], "masked_ms": t["masked"],
                "sparse_path": idx_sparse.stats()["last_path_name"], "masked_path": idx_scan.stats()["last_path_name"],
                "masked_fallback_queries": int(idx_scan.stats()["last_fallback_queries"]), "same_bytes": same}
    # ---- a contiguous filter: one run of rows (a tenant's range) leaves fewer than k live superbins --------------------------------------
    contiguous = {}
    for n_allowed in (5_000, 50_000) if "contiguous" in tables else ():
        mask = np.zeros(n, np.bool_)
        mask[n // 3:n // 3 + n_allowed] = True
        idx_scan.set_filter(mask)
        idx_sparse.set_filter(mask)
        for nq in BATCHES:
            t = alternate({"sparse": lambda: filtered(idx_sparse, nq), "masked": lambda: filtered(idx_scan, nq, Dk2, Ik2)})
            torch.cuda.synchronize()
            same = bool(torch.equal(Ik[:nq], Ik2[:nq]) and torch.equal(Dk[:nq], Dk2[:nq]))
            contiguous[f"allowed{n_allowed}_nq{nq}"] = {
                "nq": nq, "n_allowed": n_allowed, "pairs": nq * n_allowed, "sparse_ms": t["sparse"], "masked_ms": t["masked"],
                "masked_path": idx_scan.stats()["last_path_name"],
                "masked_fallback_queries": int(idx_scan.stats()["last_fallback_queries"]), "same_bytes": same}
    crossover = {}
    for nq in BATCHES:
        legs = sorted((v for v in sparse.values() if v["nq"] == nq), key=lambda v: v["pairs"])
        wins = [v["pairs"] for v in legs if v["sparse_ms"] < v["masked_ms"]]
        loses = [v["pairs"] for v in legs if v["sparse_ms"] >= v["masked_ms"]]
        crossover[str(nq)] = {"largest_pairs_sparse_wins": max(wins) if wins else 0, "smallest_pairs_masked_wins": min(loses) if loses else None}

    idx_scan.close()
    idx_sparse.close()
    if args.install_n and "install" in tables:
        del X_t
        torch.cuda.empty_cache()
        big = rows(args.install_n)
        for pairs, label in ((0.0, "filter_sparse_pairs=0"), (float("inf"), "filter_sparse_pairs=inf")):
            idx = handle(2, pairs, big)
            install.append(install_times(idx, args.install_n, 0.5, label))
            idx.close()
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    result = merged.get(args.corpus, {})
    result.update({"corpus": args.corpus, "n": n, "dim": d, "metric": metric, "k": K, "steps": args.steps, "warmup": args.warmup,
                   "scan_shape": built["scan_shape"], "has_i8_copy": built["has_i8_copy"]})
    for name, table in (("masked", masked), ("install", install), ("order", order), ("sparse", sparse), ("contiguous", contiguous)):
        if name in tables:
            result[name] = table
    if "sparse" in tables:
        result["crossover"] = crossover
    merged[args.corpus] = result
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

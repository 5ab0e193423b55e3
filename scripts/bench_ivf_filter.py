"""Filtered k-NN search on an IVF-Flat index (vdb_ivf_search_filtered_device) against vdb_ivf_search_device of the same handle.

    --corpus bytes128   byte-valued 1M x 128, l2, IVF1024,Flat, nprobe 8 / 32 / 128, k = 10 (the int8 list scan)
    --corpus gauss128   Gaussian 1M x 128, l2, IVF1024,Flat, nprobe 8 / 32 / 128, k = 10 (the fp16 list scan)
    --corpus unit384    unit vectors 100 000 x 384, ip, IVF100,Flat, nprobe 32, k = 20 (the K-loop list scan)

Everything is device-resident.  Every figure is the median over `steps` calls of the time between two device events, after `warmup`
untimed rounds; the filtered and the unfiltered call of a leg of the `masked` table alternate step by step inside the same run, and
nothing else runs between them (no baseline that would evict the panels from the cache).  The two routes of the `routing` table
cannot alternate -- changing option "force_path" drops the filter -- so they are sequential blocks of warm-up and timed calls on the
same filter, installed again behind each option change.  Tables per corpus (--tables):

  masked    per nprobe, at 10 000 queries and at one query: densities 1.0 / 0.5 / 0.1 / 0.01 with random masks and one mask that clears
            every row of a tenth of the lists; filtered against unfiltered, the route the filtered call took, and -- in a pass of
            their own under option "timing" -- the prep / scan / tail times of both
  install   vdb_ivf_filter_set (host words) and vdb_ivf_filter_set_device, wall clock of the call, densities 0.5 / 0.01
  routing   selective filters on both routes: the exact list scan ("force_path" = 1) against the list-major scan ("force_path" = 2)
            on the same filter, one block of calls each, around the rule's boundary nprobe * n_allowed / nlist = 4 k; which one wins, and what the rule picks

The result is merged under its corpus name into the JSON file --out and printed as one line.  One corpus per process, each under
its own time limit:

    timeout -k 10 500 python scripts/bench_ivf_filter.py --corpus bytes128 && \\
    timeout -k 10 500 python scripts/bench_ivf_filter.py --corpus gauss128 && \\
    timeout -k 10 300 python scripts/bench_ivf_filter.py --corpus unit384
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

DENSITIES = (1.0, 0.5, 0.1, 0.01)
BATCHES = (10_000, 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["bytes128", "gauss128", "unit384"], required=True)
    ap.add_argument("--tables", default="masked,install,routing", help="which tables to measure; the others keep what --out holds")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--niter", type=int, default=8, help="k-means iterations of the index build")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r23_bench_ivf_filter.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import vdbhip
    from vdbhip import _ffi

    tables = set(args.tables.split(","))
    dev = torch.device("cuda:0")
    if args.corpus == "unit384":
        n, d, metric, nlist, nprobes, k = 100_000, 384, "ip", 100, (32,), 20
    else:
        n, d, metric, nlist, nprobes, k = 1_000_000, 128, "l2", 1024, (8, 32, 128), 10
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
    lor = idx.assignment()
    built = idx.stats()
    del X
    Dk = torch.empty((nq_max, k), dtype=torch.float32, device=dev)
    Ik = torch.empty((nq_max, k), dtype=torch.int64, device=dev)
    Dk2, Ik2 = torch.empty_like(Dk), torch.empty_like(Ik)
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

    def filtered(nq, D=Dk, I=Ik):
        idx.search_filtered_device(Q_t.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), stream)

    def unfiltered(nq):
        idx.search_device(Q_t.data_ptr(), nq, k, Dk2.data_ptr(), Ik2.data_ptr(), stream)

    def the_masks():
        out = {}
        for dens in DENSITIES:
            out[f"density{dens:g}"] = np.ones(n, np.bool_) if dens == 1.0 else np.random.default_rng([1, int(dens * 1000)]).random(n) < dens
        cleared = np.random.default_rng(2).choice(nlist, nlist // 10, replace=False)
        out["lists_cleared"] = ~np.isin(lor, cleared)
        return out

    def route_of(st):
        return "list_major" if st["last_candidates"] > 0 or st["last_fallback_queries"] > 0 else "exact_list_scan"

    # ---- filtered against unfiltered ----------------------------------------------------------------------------------------------------
    masked = {}
    if "masked" in tables:
        for name, mask in the_masks().items():
            idx.set_filter(mask)
            for nprobe in nprobes:
                idx.set_nprobe(nprobe)
                for nq in BATCHES:
                    t = alternate({"filtered": lambda: filtered(nq), "unfiltered": lambda: unfiltered(nq)})
                    unfiltered(nq)
                    torch.cuda.synchronize()
                    ust = idx.stats()
                    filtered(nq)
                    torch.cuda.synchronize()
                    st = idx.stats()
                    masked[f"{name}_nprobe{nprobe}_nq{nq}"] = {
                        "mask": name, "nprobe": nprobe, "nq": nq, "n_allowed": int(mask.sum()), "filtered_ms": t["filtered"],
                        "unfiltered_ms": t["unfiltered"], "filtered_over_unfiltered": t["filtered"] / t["unfiltered"],
                        "route": route_of(st), "unfiltered_route": route_of(ust), "fallback_queries": int(st["last_fallback_queries"]),
                        "unfiltered_fallback_queries": int(ust["last_fallback_queries"])}
        # the stage times, in a pass of their own: setting option "timing" restarts the recording window (and, like every option,
        # drops the filter, which is installed again behind it)
        for name, mask in the_masks().items():
            for nprobe in nprobes:
                for nq in BATCHES:
                    leg = masked[f"{name}_nprobe{nprobe}_nq{nq}"]
                    for which, fn in (("filtered", lambda: filtered(nq)), ("unfiltered", lambda: unfiltered(nq))):
                        idx.set_option("timing", 1)
                        idx.set_nprobe(nprobe)
                        idx.set_filter(mask)
                        for _ in range(args.steps):
                            fn()
                        torch.cuda.synchronize()
                        st = idx.stats()
                        leg[which + "_stages"] = {"prep_ms": st["last_prep_ms"], "scan_ms": st["last_scan_ms"], "tail_ms": st["last_tail_ms"]}
        idx.set_option("timing", 0)

    # ---- install ----------------------------------------------------------------------------------------------------------------------
    install = []
    if "install" in tables:
        for density in (0.5, 0.01):
            mask = np.random.default_rng(3).random(n) < density
            words = _ffi.pack_allow_bits(mask, n)
            w_t = torch.from_numpy(words.view(np.int32)).to(dev)
            idx.clear_filter()
            base = idx.stats()["bytes_resident"]
            host, device = [], []
            for step in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                a = time.perf_counter()
                _ffi.check(idx._lib.vdb_ivf_filter_set(idx._handle(), _ffi.ptr(words), n))
                torch.cuda.synchronize()
                b = time.perf_counter()
                idx.set_filter_device(w_t.data_ptr(), n, stream)
                torch.cuda.synchronize()
                c = time.perf_counter()
                if step >= args.warmup:
                    host.append((b - a) * 1e3)
                    device.append((c - b) * 1e3)
            install.append({"rows": n, "density": density, "n_allowed": int(mask.sum()), "filter_count": idx.filter_count,
                            "host_words_ms": statistics.median(host), "device_words_ms": statistics.median(device),
                            "bytes_added": int(idx.stats()["bytes_resident"] - base)})

    # ---- both sides of the routing rule ---------------------------------------------------------------------------------------------------
    routing = {}
    if "routing" in tables:
        nprobe = nprobes[len(nprobes) // 2]
        boundary = 4.0 * k * nlist / nprobe                # n_allowed at which nprobe * n_allowed / nlist = 4 k
        for factor in (0.125, 0.5, 1.0, 2.0, 8.0, 32.0):
            n_allowed = int(min(n, max(1, boundary * factor)))
            mask = np.zeros(n, np.bool_)
            mask[rng.choice(n, n_allowed, replace=False)] = True
            for nq in BATCHES:
                ms, same, fbq = {}, [], {}
                for force, label in ((1, "exact"), (2, "list_major")):
                    idx.set_option("force_path", force)
                    idx.set_nprobe(nprobe)
                    idx.set_filter(mask)
                    ms[label] = alternate({label: lambda: filtered(nq, *((Dk, Ik) if force == 1 else (Dk2, Ik2)))})[label]
                    torch.cuda.synchronize()
                    fbq[label] = int(idx.stats()["last_fallback_queries"])
                same = bool(torch.equal(Ik[:nq], Ik2[:nq]) and torch.equal(Dk[:nq], Dk2[:nq]))
                idx.set_option("force_path", 0)
                idx.set_nprobe(nprobe)
                idx.set_filter(mask)
                filtered(nq)
                torch.cuda.synchronize()
                routing[f"allowed{n_allowed}_nq{nq}"] = {
                    "nprobe": nprobe, "nq": nq, "n_allowed": n_allowed, "rows_probed_admitted": nprobe * n_allowed / nlist, "four_k": 4 * k,
                    "exact_ms": ms["exact"], "list_major_ms": ms["list_major"], "list_major_fallback_queries": fbq["list_major"],
                    "rule_picks": route_of(idx.stats()), "faster": "exact" if ms["exact"] < ms["list_major"] else "list_major", "same_bytes": same}

    idx.close()
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    result = merged.get(args.corpus, {})
    result.update({"corpus": args.corpus, "n": n, "dim": d, "metric": metric, "nlist": nlist, "k": k, "steps": args.steps, "warmup": args.warmup,
                   "niter": args.niter, "build_s": build_s, "has_i8_copy": built["has_i8_copy"]})
    for name, table in (("masked", masked), ("install", install), ("routing", routing)):
        if name in tables:
            result[name] = table
    merged[args.corpus] = result
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

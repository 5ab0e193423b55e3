"""IVF-I8 (lossless int8 lists) against IVF-Flat on the config-4 shape: sift-like bytes 1M x 128, l2, IVF1024, nprobe 8 / 32 / 128,
10 000 queries, k = 10.

Per handle kind (--kinds flat,i8) and nprobe, two batches: integer queries (the int8 list scan on either kind) and the same queries +
0.25 (IVF-Flat: its resident fp16 panels; IVF-I8: one conversion pass over the panel space, then the same scan).  Everything is
device-resident; a figure is the median over `steps` calls of the time between two device events after `warmup` untimed calls, with
the smallest and largest of those calls next to it -- the run's own spread.  The stage times (prep / scan / tail) come from a pass of
their own under option "timing".  On the I8 handle the non-integer batch is measured once more under option "ivf_i8_scratch" = 0 (the
exact list scan serves it), with fewer repeats: that is what the option costs.  Both kinds file the rows under the same centroids
(trained once on the first handle), and with both kinds in one run the results of every leg are compared byte for byte.

The record goes under --label into the JSON file --out.  The same script runs against another build of the package (--pkg DIR, the
directory that holds `vdbhip/`): the parent commit's IVF-Flat times on the same data are the yardstick of the integer batches --

    timeout -k 10 900 python scripts/bench_ivf_i8.py --label this && \\
    timeout -k 10 600 python scripts/bench_ivf_i8.py --label parent --kinds flat --pkg /path/to/parent/vectordb-retrieval_amd
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="flat,i8")
    ap.add_argument("--label", default="this")
    ap.add_argument("--pkg", default=str(ROOT / "vectordb-retrieval_amd"), help="directory that holds the vdbhip package to measure")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--niter", type=int, default=4, help="k-means iterations of the one training run")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r26_bench_ivf_i8.json"))
    args = ap.parse_args()
    for p in (str(ROOT), args.pkg):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch

    import vdbhip

    kinds = args.kinds.split(",")
    dev = torch.device("cuda:0")
    n, d, k, nq, nlist = args.n, 128, 10, args.nq, args.nlist
    g = torch.Generator(device=dev)
    g.manual_seed(0)

    def rows(count):
        return torch.clamp(torch.round(torch.empty((count, d), device=dev).exponential_(1.0 / 30.0, generator=g)), 0, 255)

    X = rows(n).cpu().numpy()
    Qi_t = rows(nq)
    Qf_t = Qi_t + 0.25
    stream = torch.cuda.current_stream().cuda_stream
    D_t = {kind: torch.empty((nq, k), dtype=torch.float32, device=dev) for kind in kinds}
    I_t = {kind: torch.empty((nq, k), dtype=torch.int64, device=dev) for kind in kinds}

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t = [event_ms(fn) for _ in range(steps)]
        return {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "repeats": steps}

    handles, record, centroids = {}, {}, None
    for kind in kinds:
        t0 = time.perf_counter()
        idx = (vdbhip.IVFI8Index if kind == "i8" else vdbhip.IVFFlatIndex)(d, nlist, "l2", 0)
        if centroids is None:
            idx.train(X, niter=args.niter)
            centroids = idx.centroids()
        else:
            idx.set_centroids(centroids)
        idx.add(X)
        build_s = time.perf_counter() - t0
        st = idx.stats()
        handles[kind] = idx
        record[kind] = {"build_s": build_s, "has_i8_copy": st["has_i8_copy"], "upload_blocks": st["upload_blocks"],
                        "index_bytes_after_add": st["bytes_resident"] - st["bytes_workspace"],
                        "index_bytes_over_float32_corpus": (st["bytes_resident"] - st["bytes_workspace"]) / (4.0 * n * d), "legs": {}}
    del X

    def search(kind, q_t):
        handles[kind].search_device(q_t.data_ptr(), nq, k, D_t[kind].data_ptr(), I_t[kind].data_ptr(), stream)

    same = True
    for nprobe in (8, 32, 128):
        for batch, q_t in (("int", Qi_t), ("frac", Qf_t)):
            for kind in kinds:
                idx = handles[kind]
                idx.set_nprobe(nprobe)
                leg = timed(lambda: search(kind, q_t), args.steps, args.warmup)
                torch.cuda.synchronize()
                st = idx.stats()
                leg.update({"scan_dtype": st["scan_dtype"], "candidates": st["last_candidates"], "fallback_queries": st["last_fallback_queries"],
                            "bytes_resident": st["bytes_resident"], "bytes_workspace": st["bytes_workspace"]})
                idx.set_option("timing", 1)
                for _ in range(args.steps):
                    search(kind, q_t)
                torch.cuda.synchronize()
                st = idx.stats()
                idx.set_option("timing", 0)
                leg["stages"] = {"prep_ms": st["last_prep_ms"], "scan_ms": st["last_scan_ms"], "tail_ms": st["last_tail_ms"]}
                record[kind]["legs"][f"nprobe{nprobe}_{batch}"] = leg
            if len(kinds) == 2:
                same = same and bool(torch.equal(I_t[kinds[0]], I_t[kinds[1]]) and torch.equal(D_t[kinds[0]], D_t[kinds[1]]))
    if "i8" in kinds:                                       # what "ivf_i8_scratch" = 0 costs: the exact list scan for the non-integer batch
        idx = handles["i8"]
        keep_D, keep_I = D_t["i8"].clone(), I_t["i8"].clone()
        for nprobe in (8, 32, 128):
            idx.set_nprobe(nprobe)
            idx.set_option("ivf_i8_scratch", 1)
            search("i8", Qf_t)
            torch.cuda.synchronize()
            keep_D.copy_(D_t["i8"])
            keep_I.copy_(I_t["i8"])
            idx.set_option("ivf_i8_scratch", 0)
            leg = timed(lambda: search("i8", Qf_t), 3, 1)
            torch.cuda.synchronize()
            st = idx.stats()
            leg.update({"fallback_queries": st["last_fallback_queries"],
                        "same_bytes_as_scratch_1": bool(torch.equal(keep_I, I_t["i8"]) and torch.equal(keep_D, D_t["i8"]))})
            record["i8"]["legs"][f"nprobe{nprobe}_frac_scratch0"] = leg
        idx.set_option("ivf_i8_scratch", 1)
    for idx in handles.values():
        idx.close()
    result = {"shape": {"n": n, "dim": d, "metric": "l2", "nlist": nlist, "nq": nq, "k": k}, "steps": args.steps, "warmup": args.warmup,
              "niter": args.niter, "kinds": record}
    if len(kinds) == 2:
        result["same_bytes_flat_and_i8"] = same
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[args.label] = result
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Records what the reference's own LSH class (src/algorithms/lsh.py) returns, for tests/test_lsh_tables_host.py and
tests/test_gpu_lsh_tables.py:

  lsh_tables_published.json   the reference's published `lsh` point on its `random` dataset, its parameters, and the small cases
  lsh_tables_published.npz    P, b of that run (what np.random.RandomState(seed) gives) and the reference's 256 x 20 ids
  lsh_tables_cases.npz        the reference's ids of the small cases

    python tests/golden/make_lsh_tables_golden.py --reference <checkout of Human-Augment-Analytics/vectordb-retrieval>

The reference's package imports faiss at import time; the LSH classes do not use it, so a stub module stands in.  Every case is
kept only if the NumPy restatement of the library's contract (tests/lsh_tables_restatement.py) returns the reference's ids on
every query: the script asserts it.  Tests never run this script and never read the reference.
"""
from __future__ import annotations

import argparse
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent / "vectordb-retrieval_amd"))

import lsh_tables_restatement as ref  # noqa: E402
from lsh_tables_cases import case_data, preprocess, published_queries  # noqa: E402
from vdbhip.lsh_tables import candidate_cap, make_tables  # noqa: E402
from vdbhip.metrics import recall_at_k  # noqa: E402

PUBLISHED = {
    "source": "benchmark_results/benchmark_20260305_070532/random/lsh_results.json + random_config.yaml (dataset options and "
              "query selection: manifest.json published_points.random_ivf_flat)",
    "metric": "l2", "num_tables": 12, "hash_size": 4, "bucket_width": 20.0, "seed": 42,
    "candidate_multiplier": 64.0, "max_candidates": None, "fallback_to_bruteforce": False, "topk": 20,
    "recall@10": 0.31914062499999996, "recall@1": 0.34765625,
}

# small cases: rows / queries are default_rng(seed).standard_normal, scaled; every parameter of the reference's LSH class
CASES = {
    "l2_t6_h3_w2": dict(n=3000, dim=16, nq=200, data_seed=101, scale=1.0, metric="l2", num_tables=6, hash_size=3, bucket_width=2.0,
                        seed=42, candidate_multiplier=3.0, max_candidates=None, fallback_to_bruteforce=False, topk=10),
    "cosine_t8_h16_fallback": dict(n=4000, dim=32, nq=200, data_seed=102, scale=1.5, metric="cosine", num_tables=8, hash_size=16,
                                   bucket_width=4.0, seed=7, candidate_multiplier=4.0, max_candidates=None,
                                   fallback_to_bruteforce=True, topk=10),
    "cosine_t8_h16_no_fallback": dict(n=4000, dim=32, nq=200, data_seed=102, scale=1.5, metric="cosine", num_tables=8, hash_size=16,
                                      bucket_width=4.0, seed=7, candidate_multiplier=4.0, max_candidates=None,
                                      fallback_to_bruteforce=False, topk=10),
    "cosine_t24_h8": dict(n=3000, dim=32, nq=200, data_seed=103, scale=1.0, metric="cosine", num_tables=24, hash_size=8,
                          bucket_width=4.0, seed=42, candidate_multiplier=128.0, max_candidates=None, fallback_to_bruteforce=False,
                          topk=20),
}


def restated(x, q, c):
    """(ids int64 (nq, topk), colliding rows per query) of the library's contract, preprocessing as the plugins do it"""
    p, b = make_tables(x.shape[1], c["num_tables"], c["hash_size"], c["metric"], c["bucket_width"], c["seed"])
    x, q = preprocess(x, q, c["metric"])
    cap = candidate_cap(c["topk"], c["candidate_multiplier"], c["max_candidates"])
    rk, qk = ref.keys(x, p, b, c["bucket_width"]), ref.keys(q, p, b, c["bucket_width"])
    _, cand, count = ref.candidates(qk, rk, c["num_tables"], cap)
    ids = ref.search(x, q, cand, c["topk"], "l2" if c["metric"] == "l2" else "ip", c["fallback_to_bruteforce"])
    return ids, count, p, b


def reference_ids(lsh_cls, x, q, c):
    algo = lsh_cls("lsh", x.shape[1], metric=c["metric"], num_tables=c["num_tables"], hash_size=c["hash_size"],
                   bucket_width=c["bucket_width"], candidate_multiplier=c["candidate_multiplier"], max_candidates=c["max_candidates"],
                   fallback_to_bruteforce=c["fallback_to_bruteforce"], seed=c["seed"])
    algo.build_index(x)
    _, ids = algo.batch_search(q, c["topk"])
    return ids.astype(np.int64), algo


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.modules.setdefault("faiss", types.ModuleType("faiss"))
    sys.path.insert(0, args.reference)
    from src.algorithms.lsh import LSH  # noqa: E402

    man = json.loads((HERE / "manifest.json").read_text())["published_points"]["random_ivf_flat"]
    opt = man["dataset_options"]
    train, q = published_queries(HERE)
    gt = np.stack([np.argsort(((train.astype(np.float64) - v.astype(np.float64)) ** 2).sum(axis=1), kind="stable")[:opt["ground_truth_k"]]
                   for v in q])
    pub = dict(PUBLISHED, n=len(train), dim=opt["dimensions"], nq=len(q))
    ids, algo = reference_ids(LSH, train, q, pub)
    r10, r1 = recall_at_k(gt, ids, 10), recall_at_k(gt, ids, 1)
    assert abs(r10 - pub["recall@10"]) < 1e-12 and abs(r1 - pub["recall@1"]) < 1e-12, (r10, r1)
    mine, count, p, b = restated(train, q, pub)
    assert np.array_equal(mine, ids), int((mine != ids).any(axis=1).sum())
    assert p.tobytes() == algo.searcher.projections.tobytes() and b.tobytes() == algo.searcher.offsets.tobytes()
    print(f"published: recall@10 {r10} recall@1 {r1}; colliding rows {count.min()}..{count.max()}; restatement equal on {len(q)} queries")
    pub_colliding = [int(count.min()), int(count.max())]
    np.savez_compressed(HERE / "lsh_tables_published.npz", projections=p, offsets=b, ids=ids.astype(np.int32))

    out_cases, arrays = {}, {}
    for name, c in CASES.items():
        x, qq = case_data(c)
        ids, _ = reference_ids(LSH, x, qq, c)
        mine, count, _, _ = restated(x, qq, c)
        assert np.array_equal(mine, ids), (name, int((mine != ids).any(axis=1).sum()))
        cap = candidate_cap(c["topk"], c["candidate_multiplier"], c["max_candidates"])
        out_cases[name] = dict(c, colliding_min=int(count.min()), colliding_max=int(count.max()),
                               queries_without_candidates=int((count == 0).sum()), queries_below_cap=int((count < cap).sum()), cap=cap)
        arrays[name] = ids.astype(np.int32)
        print(name, out_cases[name])
    np.savez_compressed(HERE / "lsh_tables_cases.npz", **arrays)
    doc = {"_comment": "The reference's published `lsh` point on its random dataset and four small cases of its LSH class "
                       "(src/algorithms/lsh.py), recorded by tests/golden/make_lsh_tables_golden.py: the ids are in "
                       "lsh_tables_published.npz / lsh_tables_cases.npz.  The NumPy restatement of the library's contract "
                       "returned the reference's ids on every query of every case when they were recorded, so the tests demand "
                       "equality.",
           "published": {k: v for k, v in pub.items()},
           "published_colliding_rows": pub_colliding,
           "cases": out_cases}
    (HERE / "lsh_tables_published.json").write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()

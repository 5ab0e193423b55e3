"""Inputs of the recorded hash-table LSH cases (tests/golden/lsh_tables_published.json), shared by the generator of the fixtures
and by the host and GPU tests.  Test infrastructure only."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "vectordb-retrieval_amd"))


def case_data(c):
    """rows and queries of a small case: default_rng(data_seed).standard_normal, scaled"""
    rng = np.random.default_rng(c["data_seed"])
    x = (rng.standard_normal((c["n"], c["dim"])) * c["scale"]).astype(np.float32)
    q = (rng.standard_normal((c["nq"], c["dim"])) * c["scale"]).astype(np.float32)
    return x, q


def preprocess(x, q, metric):
    """what the reference does to rows and queries before hashing: nothing for L2; for cosine the rows by _normalize_rows and
    every query by _normalize_vector (the 1-D norm), zero vectors staying zero"""
    if metric != "cosine":
        return x, q
    norms = np.linalg.norm(x, axis=1, keepdims=True)
    x = np.divide(x, norms, out=np.zeros_like(x), where=norms > 0)
    q = np.stack([v / np.linalg.norm(v) if np.linalg.norm(v) != 0 else np.zeros_like(v) for v in q])
    return x, q


def published_queries(golden_dir: Path):
    """(train, the 256 selected queries) of the reference's `random` dataset, manifest.json published_points.random_ivf_flat"""
    from vdbhip import datasets

    man = json.loads((Path(golden_dir) / "manifest.json").read_text())["published_points"]["random_ivf_flat"]
    opt = man["dataset_options"]
    train, test = datasets.random_reference(opt["dimensions"], opt["train_size"], opt["test_size"], opt["seed"])
    state = np.random.get_state()
    try:
        np.random.seed(man["config_seed"])
        sel = np.random.choice(len(test), man["n_queries"], replace=False)
    finally:
        np.random.set_state(state)
    return train, test[sel]

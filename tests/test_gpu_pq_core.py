"""The product-quantizer core across the commit that folded the IVF-PQ copy of it back into the flat one.

tests/golden/pq_core/ was written on an MI355X by the commit BEFORE the fold (tests/golden/manifest.json, "pq_core", names it and
the snippet): the sha256 of the codebooks its two trainers returned, and one artifact each of HipPQSearch, HipIVFPQSearch and
HipApproximateSearch with a 5-query search beside them (searches.npz).  The shared trainer must return the same bytes, and the
shared persistence code must load what the three copies of the protocol wrote and answer as they did.
"""
from __future__ import annotations

import hashlib
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_trainers_return_the_codebooks_of_the_parent(vdb, golden_dir):
    want = json.loads((golden_dir / "pq_core" / "trainer_sha256.json").read_text())
    X = np.random.default_rng(17).standard_normal((2000, 16)).astype(np.float32)
    pq = vdb.PQIndex(16, 4, "l2", 0)
    ivfpq = vdb.IVFPQIndex(16, 4, 4, "l2", 0)
    try:
        pq.train(X, niter=5, seed=1234)
        ivfpq.train(X, niter=5, seed=1234)
        assert hashlib.sha256(pq.codebooks().tobytes()).hexdigest() == want["pq_d16_M4"]
        assert hashlib.sha256(ivfpq.codebooks().tobytes()).hexdigest() == want["ivfpq_d16_nlist4_M4"]
    finally:
        pq.close()
        ivfpq.close()


@pytest.mark.parametrize("name,cls,key", [("pq", "HipPQSearch", "PQ2"), ("ivfpq", "HipIVFPQSearch", "IVF4,PQ2"),
                                          ("ivfflat", "HipApproximateSearch", "IVF4,Flat")])
def test_artifacts_of_the_parent_load_and_answer_as_recorded(vdb, golden_dir, name, cls, key):
    rec = np.load(golden_dir / "pq_core" / "searches.npz")
    algo = vdb.get_algorithm_instance(cls, 8, name=name, index_type=key, metric="l2")
    info = algo.load_index(str(golden_dir / "pq_core" / name))
    assert info["manifest_path"] == str(golden_dir / "pq_core" / name / "manifest.json") and info["build_time_s"] == 0.0
    try:
        assert algo.index.ntotal == 300
        D, I = algo.batch_search(rec["Q"], 5)          # (the IVF artifacts carry nprobe = 2 in their manifests)
        np.testing.assert_array_equal(I, rec[name + "_I"])
        np.testing.assert_array_equal(D, rec[name + "_D"])
    finally:
        algo.index.close()

"""vdbhip/persist.py without a GPU: what it writes equals, key for key and byte for byte, the manifests under tests/golden/pq_core/
(written by the three copies of the protocol that the algorithm classes carried before it existed), and it refuses what they
refused, in their words."""
from __future__ import annotations

import json
import re

import numpy as np
import pytest

from vdbhip import persist
from vdbhip.ivf import _fingerprint

# artifact -> the fields the algorithm class puts between "metric" and "config_hash", and the arrays in the order it names them
CASES = {"pq": (("M", "id_base", "n_vectors"), ("codebooks", "codes")),
         "ivfpq": (("nlist", "M", "nprobe", "id_base", "n_vectors"), ("centroids", "codebooks", "codes", "list_of_row")),
         "ivfflat": (("nlist", "nprobe", "n_vectors"), ("vectors", "centroids", "list_of_row"))}
HEAD = ("format", "algorithm", "dimension", "index_type", "metric")


def _committed(golden_dir, name):
    src = golden_dir / "pq_core" / name
    text = (src / "manifest.json").read_text(encoding="utf-8")
    committed = json.loads(text)
    fields, files = CASES[name]
    arrays = {f: np.load(src / f"{f}.npy") for f in files}
    manifest = {key: committed[key] for key in HEAD + fields}
    fingerprint = _fingerprint(*arrays.values()) if name == "ivfflat" else None
    return text, committed, manifest, arrays, fingerprint


@pytest.mark.parametrize("name", sorted(CASES))
def test_written_manifest_equals_the_committed_one(golden_dir, tmp_path, name):
    text, committed, manifest, arrays, fingerprint = _committed(golden_dir, name)
    info = persist.write_artifact(str(tmp_path / "a"), None, manifest, arrays, fingerprint)
    assert info == {"artifact_dir": str(tmp_path / "a"), "manifest_path": str(tmp_path / "a" / "manifest.json"), "build_time_s": 0.0}
    got = json.loads((tmp_path / "a" / "manifest.json").read_text(encoding="utf-8"))
    assert list(got) == list(committed)
    for key in committed:
        assert got[key] == committed[key], key
    assert list(got["sha256"]) == list(committed["sha256"]) and list(got["files"]) == list(committed["files"])
    assert (tmp_path / "a" / "manifest.json").read_text(encoding="utf-8") == text
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(p.name for p in (golden_dir / "pq_core" / name).iterdir())
    for f in arrays:
        assert (tmp_path / "a" / f"{f}.npy").read_bytes() == (golden_dir / "pq_core" / name / f"{f}.npy").read_bytes()
    assert (tmp_path / "a" / "WRITE_COMPLETE").read_text() == "ok\n" and (tmp_path / "a" / "build_metrics.json").read_text() == "{}"
    # what was written reads back, with the context's metrics and hash
    persist.write_artifact(str(tmp_path / "b"), {"build_metrics": {"build_time_s": 1.5}, "config_hash": "abc"}, manifest, arrays)
    want = {key: committed[key] for key in ("format", "dimension", "index_type", "metric")}
    back, load, info = persist.read_artifact(str(tmp_path / "b"), {"config_hash": "abc"}, committed["algorithm"], **want)
    assert back["config_hash"] == "abc" and info["build_time_s"] == 1.5 and info["artifact_dir"] == str(tmp_path / "b")
    for f, arr in arrays.items():
        np.testing.assert_array_equal(load(f), arr)
    persist.check_sha256(back, arrays)
    assert isinstance(load(next(iter(arrays)), mmap_mode="r"), np.memmap)


def test_read_refuses_what_the_classes_refused(golden_dir, tmp_path):
    _, committed, manifest, arrays, _ = _committed(golden_dir, "ivfpq")
    want = {key: committed[key] for key in ("format", "dimension", "index_type", "metric")}
    with pytest.raises(FileNotFoundError, match=re.escape(f"Persisted HipIVFPQSearch artifact directory not found: {tmp_path / 'none'}")):
        persist.read_artifact(str(tmp_path / "none"), None, "HipIVFPQSearch", **want)
    persist.write_artifact(str(tmp_path / "a"), {"config_hash": "abc"}, manifest, arrays)
    for key, other in (("format", "vdbhip-pq-v1"), ("dimension", 16), ("index_type", "IVF4,PQ4"), ("metric", "ip")):
        message = f"Persisted index mismatch for '{key}': artifact has {committed[key]!r}, this instance expects {other!r}"
        with pytest.raises(ValueError, match=re.escape(message)):
            persist.read_artifact(str(tmp_path / "a"), None, "HipIVFPQSearch", **dict(want, **{key: other}))
    with pytest.raises(ValueError, match=re.escape("Persisted index was built with a different configuration (config_hash mismatch)")):
        persist.read_artifact(str(tmp_path / "a"), {"config_hash": "zzz"}, "HipIVFPQSearch", **want)
    persist.read_artifact(str(tmp_path / "a"), {"config_hash": "abc"}, "HipIVFPQSearch", **want)
    persist.read_artifact(str(tmp_path / "a"), None, "HipIVFPQSearch", **want)      # (a reader without a hash takes any)
    bad = dict(arrays, codes=arrays["codes"] ^ 1)
    with pytest.raises(ValueError, match=re.escape("Persisted index files do not belong together (fingerprint mismatch: codes)")):
        persist.check_sha256(committed, bad)
    (tmp_path / "a" / "WRITE_COMPLETE").unlink()
    with pytest.raises(FileNotFoundError, match=re.escape(f"Artifact is incomplete or corrupted (missing WRITE_COMPLETE): {tmp_path / 'a'}")):
        persist.read_artifact(str(tmp_path / "a"), None, "HipIVFPQSearch", **want)


def test_write_keeps_an_existing_target_and_leaves_no_temp_dir(golden_dir, tmp_path):
    _, _, manifest, arrays, _ = _committed(golden_dir, "pq")
    persist.write_artifact(str(tmp_path / "a"), None, manifest, arrays)
    before = (tmp_path / "a" / "manifest.json").read_text()
    message = f"Artifact directory already exists: {tmp_path / 'a'}. Set persistence.force_rebuild=true to overwrite."
    with pytest.raises(FileExistsError, match=re.escape(message)):
        persist.write_artifact(str(tmp_path / "a"), {"config_hash": "new"}, manifest, arrays)
    assert (tmp_path / "a" / "manifest.json").read_text() == before
    persist.write_artifact(str(tmp_path / "a"), {"config_hash": "new", "force_rebuild": True}, manifest, arrays)
    assert json.loads((tmp_path / "a" / "manifest.json").read_text())["config_hash"] == "new"
    # a failing write (an object array cannot be saved without pickle) raises, and neither a target nor a temp dir remains
    with pytest.raises(ValueError):
        persist.write_artifact(str(tmp_path / "b"), None, manifest, dict(arrays, codes=np.array([object()], dtype=object)))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a"]

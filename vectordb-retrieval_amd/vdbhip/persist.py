"""The artifact protocol of the persisting algorithm classes (HipApproximateSearch, HipPQSearch, HipIVFPQSearch).

Layout and protocol follow the reference's only implementation (covertree_v2_2.py:101-182, 184-282): a temp dir beside the
target, the arrays as .npy files, manifest.json, build_metrics.json, the WRITE_COMPLETE sentinel written last, one atomic
rename; reading refuses an incomplete artifact or a manifest that does not match the instance that reads it.
"""
from __future__ import annotations

import hashlib
import json
import shutil
import tempfile
from pathlib import Path
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np


def sha256(arr: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def _result(path: Path, metrics: dict) -> dict:
    return {"artifact_dir": str(path), "manifest_path": str(path / "manifest.json"),
            "build_time_s": float(metrics.get("build_time_s", 0.0) or 0.0)}


def write_artifact(artifact_dir: str, context: Optional[dict], manifest: Dict[str, Any], arrays: Dict[str, np.ndarray],
                   fingerprint: Optional[dict] = None) -> dict:
    """Write `arrays` (name -> array, saved as <name>.npy) and the manifest: the caller's fields, then `config_hash` of
    the context, `sha256` (one digest per array, or the caller's `fingerprint` in their place) and `files`.  An existing
    target is replaced only under context["force_rebuild"]; a failing write leaves no temp dir behind."""
    context = context or {}
    target = Path(artifact_dir)
    target.parent.mkdir(parents=True, exist_ok=True)
    if target.exists():
        if not bool(context.get("force_rebuild", False)):
            raise FileExistsError(f"Artifact directory already exists: {target}. "
                                  "Set persistence.force_rebuild=true to overwrite.")
        shutil.rmtree(target)
    tmp = Path(tempfile.mkdtemp(prefix=f".{target.name}.tmp.", dir=str(target.parent)))
    try:
        for name, arr in arrays.items():
            np.save(tmp / f"{name}.npy", arr, allow_pickle=False)
        build_metrics = dict(context.get("build_metrics", {}))
        manifest = dict(manifest, config_hash=context.get("config_hash"),
                        sha256=fingerprint if fingerprint is not None else {name: sha256(arr) for name, arr in arrays.items()},
                        files={name: f"{name}.npy" for name in arrays})
        (tmp / "manifest.json").write_text(json.dumps(manifest, indent=2), encoding="utf-8")
        (tmp / "build_metrics.json").write_text(json.dumps(build_metrics, indent=2), encoding="utf-8")
        (tmp / "WRITE_COMPLETE").write_text("ok\n", encoding="utf-8")
        tmp.rename(target)
    except Exception:
        shutil.rmtree(tmp, ignore_errors=True)
        raise
    return _result(target, build_metrics)


def read_artifact(artifact_dir: str, context: Optional[dict], algorithm: str, *, format: str, dimension: int, index_type: str,
                  metric: str) -> Tuple[dict, Callable[..., np.ndarray], dict]:
    """Open the artifact of class `algorithm`: its manifest must hold this format, dimension, index_type and metric and,
    when both sides name one, the context's config_hash.  Returns the manifest, load(name, **kwargs) for the files it
    names (np.load) and the result dict of load_index."""
    path = Path(artifact_dir)
    if not path.is_dir():
        raise FileNotFoundError(f"Persisted {algorithm} artifact directory not found: {path}")
    if not (path / "WRITE_COMPLETE").is_file():
        raise FileNotFoundError(f"Artifact is incomplete or corrupted (missing WRITE_COMPLETE): {path}")
    manifest = json.loads((path / "manifest.json").read_text(encoding="utf-8"))
    for key, want in (("format", format), ("dimension", dimension), ("index_type", index_type), ("metric", metric)):
        if manifest.get(key) != want:
            raise ValueError(f"Persisted index mismatch for '{key}': artifact has {manifest.get(key)!r}, "
                             f"this instance expects {want!r}")
    expected_hash = (context or {}).get("config_hash")
    if expected_hash and manifest.get("config_hash") and manifest["config_hash"] != expected_hash:
        raise ValueError("Persisted index was built with a different configuration (config_hash mismatch)")
    metrics = {}
    bm = path / "build_metrics.json"
    if bm.is_file():
        metrics = json.loads(bm.read_text(encoding="utf-8"))

    def load(name: str, **kwargs: Any) -> np.ndarray:
        return np.load(path / manifest["files"][name], **kwargs)

    return manifest, load, _result(path, metrics)


def check_sha256(manifest: dict, arrays: Dict[str, np.ndarray]) -> None:
    """The arrays must be the ones that were written together: every digest the manifest records is compared."""
    want = manifest.get("sha256") or {}
    for name, arr in arrays.items():
        if want.get(name) and sha256(arr) != want[name]:
            raise ValueError(f"Persisted index files do not belong together (fingerprint mismatch: {name})")

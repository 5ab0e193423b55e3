"""Shared assertions, value distributions and codec restatements for parity tests."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def assert_same_neighbours_modulo_ties(ids_a, ids_b, keys_a, keys_b, rtol=0.0):
    """Rows must hold the same ids; inside a group of equal keys any order is accepted
    (the reference's argpartition/argsort leaves the order of exact ties unspecified)."""
    ids_a, ids_b = np.asarray(ids_a), np.asarray(ids_b)
    assert ids_a.shape == ids_b.shape
    for r in range(ids_a.shape[0]):
        if np.array_equal(ids_a[r], ids_b[r]):
            continue
        ka, kb = np.asarray(keys_a[r], np.float64), np.asarray(keys_b[r], np.float64)
        np.testing.assert_allclose(ka, kb, rtol=max(rtol, 1e-6), atol=1e-6)
        # group by key value of row a; the id multisets per group must agree except at the cut
        vals = np.unique(ka)
        for v in vals[:-1]:
            sa = set(ids_a[r][ka == v].tolist())
            sb = set(ids_b[r][np.isclose(kb, v, rtol=max(rtol, 1e-6), atol=1e-6)].tolist())
            assert sa == sb, f"row {r}: tie group {v} differs: {sa} vs {sb}"


def tie_band_mismatch_report(ids_test, ids_ref, keys64_of_test, keys64_of_ref, band=1e-6):
    """For rows whose id lists differ, verify every differing position lies in a near-tie band of the
    exact float64 keys (|ka-kb| <= band*max(1,|k|)).  Returns number of differing rows."""
    bad_rows = 0
    for r in range(ids_test.shape[0]):
        if np.array_equal(ids_test[r], ids_ref[r]):
            continue
        bad_rows += 1
        ka, kb = keys64_of_test[r], keys64_of_ref[r]
        diff = ids_test[r] != ids_ref[r]
        scale = np.maximum(1.0, np.abs(kb[diff]))
        assert np.all(np.abs(ka[diff] - kb[diff]) <= band * scale), (
            f"row {r}: neighbour mismatch outside the tie band: {ka[diff]} vs {kb[diff]}")
    return bad_rows


def values(rng, kind, shape):
    """Value distributions of the fuzz sweep and the error-bound tests (float64; the caller casts)."""
    if kind == "gauss":
        return rng.standard_normal(shape)
    if kind == "ints":            # SIFT-like: exact in fp16, unscaled
        return np.clip(np.rint(rng.gamma(0.6, 40.0, size=shape)), 0, 218)
    if kind == "bigints":         # integers beyond the unscaled fp16 range
        return np.rint(rng.standard_normal(shape) * 3000.0)
    if kind == "tiny":
        return rng.standard_normal(shape) * 1e-4
    if kind == "huge":
        return rng.standard_normal(shape) * 1e5
    if kind == "heavy":           # heavy tails: a few coordinates dominate the norms
        return np.clip(rng.standard_cauchy(shape), -1e3, 1e3)
    if kind == "sparse":          # mostly zeros
        return rng.standard_normal(shape) * (rng.random(shape) < 0.05)
    if kind == "offset":          # large common offset, small spread (cancellation in ||x||^2 - 2 q.x)
        return 50.0 + rng.standard_normal(shape) * 0.1
    if kind == "bytes":           # the whole uint8 range: int8 scan copy, largest accumulator magnitudes
        return rng.integers(0, 256, size=shape).astype(np.float64)
    if kind == "sbytes":          # the whole int8 range (s8 window)
        return rng.integers(-128, 128, size=shape).astype(np.float64)
    raise AssertionError(kind)


# ---- NumPy restatement of the IVF-SQ8 codec (every operation float32, rounded as written) ----
def np_ranges(X, C, lor):
    R = X - C[lor]
    vmin = R.min(axis=0)
    return vmin, R.max(axis=0) - vmin


def np_encode(X, C, lor, vmin, vdiff):
    R = X - C[lor]
    safe = np.where(vdiff != 0, vdiff, F32(1))
    U = np.where(vdiff != 0, (R - vmin) / safe, F32(0)).astype(F32)
    U = np.clip(U, F32(0), F32(1))
    return (F32(255) * U).astype(np.uint8)


def np_decode(codes, C, lor, vmin, vdiff):
    return C[lor] + (vmin + ((codes.astype(F32) + F32(0.5)) / F32(255)) * vdiff)

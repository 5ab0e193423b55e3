"""Inputs of the IVF-I8 tests (tests/test_gpu_ivf_i8.py, tests/test_ivf_i8_host.py) and a NumPy restatement of the rules of
csrc/ivf_i8_plan.hpp.  No GPU and no library: the host test checks the inputs themselves (byte test, list sizes)."""
from __future__ import annotations

import numpy as np

F32 = np.float32
N, NLIST, ID_BASE = 20000, 32, 1000
WINDOWS = {"u8": (0, 255, 128), "s8": (-128, 127, 0)}          # lo, hi, cx
DIMS = (50, 64, 100, 128)
# the lists the issue asks for: an empty one, exactly one span (256 rows), one row more, several spans (> 1024 rows)
FIXED_SIZES = {0: 0, 1: 256, 2: 257, 3: 1500}


def np_window(x):
    """cx of a row set, or -1: ivf_i8_window over (min, max, all values finite integers).  0..255 wins where both windows fit."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return -1
    if not np.isfinite(x).all() or (x != np.rint(x)).any():
        return -1
    lo, hi = x.min(), x.max()
    if lo >= 0 and hi <= 255:
        return 128
    if lo >= -128 and hi <= 127:
        return 0
    return -1


def np_pitch(dim):
    return 64 if dim <= 64 else 128


def np_panel_rows(list_sizes):
    """slots of the list-padded panel space: every list padded to whole 256-row spans"""
    return int(sum((int(s) + 255) // 256 * 256 for s in list_sizes))


def np_i8_bytes(n, panel_rows, dim):
    """ivf_i8_bytes: rows8 + rowstat8 + ids per row; panels8 + bias8 (two windows) + fp16-scan bias per panel row; two span tables"""
    p = np_pitch(dim)
    return n * (p + 8 + 8) + panel_rows * (p + 8 + 4) + panel_rows // 256 * 8


def np_slab_bytes(panel_rows, dim):
    return panel_rows * np_pitch(dim) * 2


def list_of_row(seed=5):
    """int32 (N,): lists 0..3 have the fixed sizes, the other rows spread over lists 4..31; shuffled, so every list's rows are
    scattered over the insertion order"""
    rng = np.random.default_rng(seed)
    lor = np.concatenate([np.full(s, l, np.int32) for l, s in FIXED_SIZES.items()])
    rest = N - len(lor)
    lor = np.concatenate([lor, rng.integers(4, NLIST, rest).astype(np.int32)])
    rng.shuffle(lor)
    return lor


def corpus(dim, window, seed=0):
    """(X float32 (N, dim), C float32 (NLIST, dim), lor int32 (N,)): uniform integers over the whole window, both window edges present
    (in the first and in the last valid dimension)"""
    lo, hi, _ = WINDOWS[window]
    rng = np.random.default_rng(1000 * dim + seed + (7 if window == "s8" else 0))
    X = rng.integers(lo, hi + 1, (N, dim)).astype(F32)
    X[0, 0], X[1, 0], X[2, dim - 1], X[3, dim - 1] = lo, hi, lo, hi
    C = rng.uniform(lo, hi, (NLIST, dim)).astype(F32)
    return X, C, list_of_row()


def queries(dim, window, nq=96, seed=1):
    """(integer queries inside the window, the same + 0.25)"""
    lo, hi, _ = WINDOWS[window]
    rng = np.random.default_rng(77 * dim + seed)
    Qi = rng.integers(lo, hi + 1, (nq, dim)).astype(F32)
    return Qi, (Qi + F32(0.25)).astype(F32)

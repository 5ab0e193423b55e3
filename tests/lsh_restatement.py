"""NumPy restatement of the sign-LSH contract of include/vdbhip.h (bits, codes, Hamming distance, candidate order) and of the
reference's re-rank loop.  Test infrastructure only: nothing in the product imports it.

  bits        s_j(x) = sum_d float64(x[d]) * float64(R[j][d]), accumulated from 0.0 with d ascending, one rounding per step
              (the product of two float32 values is exact in float64); bit j = (s_j >= 0): -0.0 / 0.0 -> 1, NaN -> 0
  codes       nbits / 32 little-endian uint32 words per row, bit j = bit j % 32 of word j / 32
  candidates  the min(ncand, ntotal) rows smallest under (Hamming distance, id), in that order; padding id -1, INT32_MAX
"""
from __future__ import annotations

import numpy as np

INT32_MAX = np.iinfo(np.int32).max


def sign_bits(x: np.ndarray, r: np.ndarray, block: int = 8192) -> np.ndarray:
    """bool (n, nbits)"""
    x = np.asarray(x, dtype=np.float32)
    r64 = np.asarray(r, dtype=np.float32).astype(np.float64)
    n, dim = x.shape
    out = np.empty((n, r64.shape[0]), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, n, block):
            xb = x[r0:r0 + block].astype(np.float64)
            s = np.zeros((xb.shape[0], r64.shape[0]), dtype=np.float64)
            for d in range(dim):                       # d ascending, one rounding (the add) per step
                s += xb[:, d:d + 1] * r64[:, d][None, :]
            out[r0:r0 + block] = s >= 0
    return out


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """uint32 (n, nbits / 32)"""
    assert bits.shape[1] % 32 == 0
    b = np.packbits(bits, axis=1, bitorder="little")                     # byte i holds bits 8i .. 8i + 7, LSB first
    return np.ascontiguousarray(b).view("<u4").astype(np.uint32)


def encode(x: np.ndarray, r: np.ndarray) -> np.ndarray:
    return pack_bits(sign_bits(x, r))


def unpack_codes(codes: np.ndarray) -> np.ndarray:
    """bool (n, 32 * words)"""
    b = np.ascontiguousarray(codes.astype("<u4")).view(np.uint8)
    return np.unpackbits(b, axis=1, bitorder="little").astype(bool)


def hamming(qcodes: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """int32 (nq, n).  Through +-1 float32 matrices: <a, b> = nbits - 2 * hamming, every partial sum an integer below 2^24."""
    a = np.where(unpack_codes(qcodes), np.float32(1), np.float32(-1))
    b = np.where(unpack_codes(codes), np.float32(1), np.float32(-1))
    nbits = a.shape[1]
    dot = a @ b.T
    return ((nbits - dot) / 2).astype(np.int32)


def candidates(qcodes: np.ndarray, codes: np.ndarray, ncand: int, id_base: int = 0, qblock: int = 64):
    """(ham int32 (nq, ncand), ids int64 (nq, ncand))"""
    nq, n = qcodes.shape[0], codes.shape[0]
    c = min(ncand, n)
    ham_out = np.full((nq, ncand), INT32_MAX, dtype=np.int32)
    ids_out = np.full((nq, ncand), -1, dtype=np.int64)
    rows = np.arange(n, dtype=np.int64)
    for q0 in range(0, nq, qblock):
        h = hamming(qcodes[q0:q0 + qblock], codes).astype(np.int64)
        key = h * n + rows[None, :]                                      # order (distance, row)
        if c < n:
            part = np.argpartition(key, c - 1, axis=1)[:, :c]
            key = np.take_along_axis(key, part, axis=1)
        key = np.sort(key, axis=1)[:, :c]
        ham_out[q0:q0 + qblock, :c] = (key // n).astype(np.int32)
        ids_out[q0:q0 + qblock, :c] = key % n + id_base
    return ham_out, ids_out


def reference_rerank(base: np.ndarray, queries: np.ndarray, cand_ids: np.ndarray, k: int, metric: str):
    """FaissSearcher._batch_search_lsh_rerank's loop (modular.py:479-534) over given candidate ids, float32 NumPy as there;
    `base` / `queries` already normalised for cosine.  Ties are left to a stable order by (value, candidate position)."""
    nq = queries.shape[0]
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        valid = cand_ids[i][cand_ids[i] >= 0]
        if valid.size == 0:
            continue
        vecs = base[valid]
        if metric == "l2":
            vals = np.sum((vecs - queries[i:i + 1]) ** 2, axis=1)
        else:
            vals = -(queries[i:i + 1] @ vecs.T).ravel()
        limit = min(k, vals.shape[0])
        order = np.argsort(vals, kind="stable")[:limit]
        dist[i, :limit] = (np.sqrt(vals[order]) if metric == "l2" else vals[order]).astype(np.float32)
        ids[i, :limit] = valid[order]
    return dist, ids

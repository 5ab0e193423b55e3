"""NumPy restatement of the hash-table LSH contract of include/vdbhip.h (keys, votes / first, candidate order, search).  Test
infrastructure only: nothing in the product imports it.

  projection  s[t][h](x) = sum_d float64(x[d]) * float64(P[t][h][d]), accumulated from 0.0 with d ascending, one rounding per step
  key words   uint32, T * W per vector.  sign (W = ceil(H / 32)): bit h of table t = bit h % 32 of word t W + h / 32, set iff
              s >= 0 (-0.0 -> 1, NaN -> 0).  E2 (W = H): word t W + h = int32 floor((s + float64(b)) / float64(w)), saturated,
              NaN -> INT32_MIN
  votes       tables whose W words all agree; first = the smallest of them
  candidates  the rows with votes >= 1 under ((T - votes) T + first, id), the first min(ncand, their number); padding id -1, votes 0
  search      the k best candidates under (float64 key, id); fallback: a query without a colliding row gets the exact top-k
"""
from __future__ import annotations

import numpy as np

INT32_MIN, INT32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def projections(x: np.ndarray, p: np.ndarray, block: int = 8192) -> np.ndarray:
    """float64 (n, T, H)"""
    x = np.asarray(x, dtype=np.float32)
    T, H, dim = p.shape
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64).reshape(T * H, dim)
    out = np.empty((x.shape[0], T * H), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, x.shape[0], block):
            xb = x[r0:r0 + block].astype(np.float64)
            s = np.zeros((xb.shape[0], T * H), dtype=np.float64)
            for d in range(dim):                       # d ascending, one rounding (the add) per step
                s += xb[:, d:d + 1] * p64[:, d][None, :]
            out[r0:r0 + block] = s
    return out.reshape(x.shape[0], T, H)


def words_per_table(hash_size: int, mode: int) -> int:
    return hash_size if mode == 1 else (hash_size + 31) // 32


def keys(x: np.ndarray, p: np.ndarray, b=None, w: float = 0.0) -> np.ndarray:
    """uint32 (n, T * W): sign keys when b is None, else E2 keys"""
    s = projections(x, p)
    n, T, H = s.shape
    if b is None:
        W = (H + 31) // 32
        bits = np.zeros((n, T, W * 32), dtype=bool)
        bits[:, :, :H] = s >= 0
        packed = np.packbits(bits.reshape(n, T * W * 32), axis=1, bitorder="little")
        return np.ascontiguousarray(packed).view("<u4").astype(np.uint32).reshape(n, T * W)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor((s + np.asarray(b, np.float32).astype(np.float64)[None]) / np.float64(np.float32(w)))
    nan = np.isnan(f)
    code = np.clip(np.where(nan, 0.0, f), float(INT32_MIN), float(INT32_MAX)).astype(np.int64)
    code[nan] = INT32_MIN
    return code.astype(np.int32).view(np.uint32).reshape(n, T * H)


def votes_first(qkey: np.ndarray, rkeys: np.ndarray, T: int):
    """one query's (votes int (n), first int (n)) over the rows"""
    n = rkeys.shape[0]
    eq = (rkeys.reshape(n, T, -1) == qkey.reshape(1, T, -1)).all(axis=2)
    return eq.sum(axis=1), eq.argmax(axis=1)


def candidates(qkeys: np.ndarray, rkeys: np.ndarray, T: int, ncand: int, id_base: int = 0):
    """(votes int32 (nq, ncand), ids int64 (nq, ncand), colliding rows int64 (nq))"""
    nq = qkeys.shape[0]
    v_out = np.zeros((nq, ncand), dtype=np.int32)
    i_out = np.full((nq, ncand), -1, dtype=np.int64)
    count = np.zeros(nq, dtype=np.int64)
    for i in range(nq):
        votes, first = votes_first(qkeys[i], rkeys, T)
        rows = np.flatnonzero(votes > 0)
        cls = (T - votes[rows]) * T + first[rows]
        order = np.argsort(cls, kind="stable")[:ncand]              # (class, id): rows is ascending
        v_out[i, :order.size] = votes[rows[order]]
        i_out[i, :order.size] = rows[order] + id_base
        count[i] = rows.size
    return v_out, i_out, count


def exact_keys(base: np.ndarray, q: np.ndarray, metric: str) -> np.ndarray:
    """float64 order keys of one query against rows: squared L2, or minus the inner product"""
    b64, q64 = base.astype(np.float64), q.astype(np.float64)
    if metric == "l2":
        return ((b64 - q64[None, :]) ** 2).sum(axis=1)
    return -(b64 @ q64)


def search(base: np.ndarray, queries: np.ndarray, cand_ids: np.ndarray, k: int, metric: str, fallback: bool, id_base: int = 0):
    """ids int64 (nq, k) of the k best candidates under (float64 key, id), -1 padded; `fallback`: all rows for a query without
    candidates"""
    nq = queries.shape[0]
    out = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        rows = cand_ids[i][cand_ids[i] >= 0] - id_base
        if rows.size == 0:
            if not fallback:
                continue
            rows = np.arange(base.shape[0], dtype=np.int64)
        key = exact_keys(base[rows], queries[i], metric)
        order = np.lexsort((rows, key))[:k]
        out[i, :order.size] = rows[order] + id_base
    return out

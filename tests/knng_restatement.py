"""NumPy restatement of the k-NN graph contract of include/vdbhip.h (candidates, prune, beam search), on the canonical float64
keys of the CPU oracle.  Test infrastructure only: nothing in the product imports it.

  key(u, v)    canonical float64 order key (L2: squared distance, IP: -score), row u as the query, row v as the row; compared
               through its sortable 64-bit pattern, as the device compares it.  Every order is (key, local row number)
  candidates   of row i: the first ncand of all rows j != i
  prune        walk the candidates in order; e is selected if |S| < degree and no s in S has key(e, s) < key(i, e) (strict); the
               row is S, then the rejected candidates in candidate order until degree entries exist, then -1
  search       L = at most ef (key, id, expanded).  Init: the distinct rows floor(j N / nentry), j < min(nentry, ef, N).  Step: first
               unexpanded entry (none: stop), mark it, score its neighbours that are not in L, L <- best ef of (L u scored).  At most
               max_iters steps.  `forget=False` keeps an exact visited set and never scores a row twice; `forget=True` forgets
               everything but L and re-scores.  Both return the same lists (the visited structure is a cache).
"""
from __future__ import annotations

import bisect

import numpy as np

from oracle import c_oracle

FLT_MAX = np.finfo(np.float32).max


def sortable(keys: np.ndarray) -> np.ndarray:
    """uint64 pattern whose unsigned order is the order of the float64 keys (sortable_u64 of the library)."""
    u = np.ascontiguousarray(keys, dtype=np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def candidates(X: np.ndarray, ncand: int, metric: str = "l2", rows=None):
    """Candidates of `rows` (default: all): (cand int64 (len(rows), ncand) local rows, -1 tail; keys float64, inf tail)"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    k = min(ncand + 1, n)
    _, ids, keys = c_oracle.knn(X, X[rows], k, metric, return_keys=True)
    cand = np.full((rows.size, ncand), -1, np.int64)
    ckeys = np.full((rows.size, ncand), np.inf, np.float64)
    for i, r in enumerate(rows):
        hit = np.nonzero(ids[i] == r)[0]
        drop = int(hit[0]) if hit.size else k - 1          # duplicates of row r with smaller ids pushed it out: drop the last
        keep = np.delete(np.arange(k), drop)
        cand[i, :k - 1] = ids[i, keep]
        ckeys[i, :k - 1] = keys[i, keep]
    return cand, ckeys


def prune(X: np.ndarray, cand: np.ndarray, ckeys: np.ndarray, degree: int, metric: str = "l2", chunk: int = 128) -> np.ndarray:
    """int32 (len(cand), degree): the neighbours of the rows whose candidates (and keys key(i, e)) are given."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    m, nc = cand.shape
    out = np.full((m, degree), -1, np.int32)
    for r0 in range(0, m, chunk):
        c = cand[r0:r0 + chunk]                                             # (b, nc)
        safe = np.where(c >= 0, c, 0)
        # G[i, a, b] = key(c[i, a], c[i, b]): query row c[i, a], row c[i, b]
        G = c_oracle.pair_keys(X, X[safe.ravel()], np.repeat(c, nc, axis=0), metric).reshape(c.shape[0], nc, nc)
        Gs, ks = sortable(G), sortable(ckeys[r0:r0 + chunk])
        for i in range(c.shape[0]):
            sel, rej = [], []
            for a in range(nc):
                if c[i, a] < 0:
                    break
                if len(sel) < degree and not any(Gs[i, a, s] < ks[i, a] for s in sel):
                    sel.append(a)
                else:
                    rej.append(a)
            row = (sel + rej)[:degree]
            out[r0 + i, :len(row)] = c[i, row]
    return out


def build(X: np.ndarray, degree: int, ncand: int, metric: str = "l2", rows=None) -> np.ndarray:
    cand, ckeys = candidates(X, ncand, metric, rows)
    return prune(X, cand, ckeys, degree, metric)


def entry_rows(n: int, ef: int, nentry: int):
    return sorted({(j * n) // nentry for j in range(min(nentry, ef, n))})


def search_one(order_key, nbrs, n: int, ef: int, nentry: int, max_iters: int, forget: bool):
    """order_key[row] = (sortable key << 32) | row as a Python int.  Returns (L, rows scored, stopped by the cap)."""
    L = sorted(order_key[r] for r in entry_rows(n, ef, nentry))[:ef]
    in_l = {v & 0xffffffff for v in L}
    visited = set(in_l)
    expanded = set()
    scored = len(L)
    p = 0                                   # every entry in front of L[p] is expanded
    steps = 0
    while True:
        while p < len(L) and (L[p] & 0xffffffff) in expanded:
            p += 1
        if p == len(L):
            return L, scored, False
        if steps == max_iters:
            return L, scored, True
        steps += 1
        node = L[p] & 0xffffffff
        expanded.add(node)
        new = [int(v) for v in nbrs[node] if v >= 0 and int(v) not in (in_l if forget else visited)]
        if not new:
            continue
        scored += len(new)
        visited.update(new)
        fresh = sorted(order_key[v] for v in new)
        p = min(p, bisect.bisect_left(L, fresh[0]))
        merged = sorted(L + fresh)
        L = merged[:ef]
        in_l.update(new)
        for v in merged[ef:]:
            in_l.discard(v & 0xffffffff)


def search(X, nbrs, Q, k: int, ef: int, metric: str = "l2", nentry: int = 32, max_iters=None, id_base: int = 0, forget: bool = False,
           qchunk: int = 64):
    """(D float32 (nq, k), I int64 (nq, k), scored int64 (nq), capped bool (nq)) in flat conventions."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, X.shape[1])
    nbrs = np.asarray(nbrs)
    n, nq = X.shape[0], Q.shape[0]
    max_iters = 8 * ef if max_iters is None else max_iters
    D = np.full((nq, k), FLT_MAX if metric == "l2" else -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    scored = np.zeros(nq, np.int64)
    capped = np.zeros(nq, bool)
    all_rows = np.arange(n, dtype=np.int64)
    nb_list = [row[row >= 0].tolist() for row in nbrs]
    for q0 in range(0, nq, qchunk):
        qs = Q[q0:q0 + qchunk]
        keys = c_oracle.pair_keys(X, qs, np.tile(all_rows, (qs.shape[0], 1)), metric)          # (m, n)
        sk = sortable(keys)
        for j in range(qs.shape[0]):
            order_key = [(int(s) << 32) | r for r, s in enumerate(sk[j].tolist())]
            L, scored[q0 + j], capped[q0 + j] = search_one(order_key, nb_list, n, ef, nentry, max_iters, forget)
            ids = np.array([v & 0xffffffff for v in L[:k]], np.int64)
            kk = keys[j, ids]
            D[q0 + j, :ids.size] = (kk if metric == "l2" else -kk).astype(np.float32)
            I[q0 + j, :ids.size] = ids + id_base
    return D, I, scored, capped

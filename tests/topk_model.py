"""Plain-Python restatement of what `WaveTopK<KPL>::offer` (csrc/topk.hpp) DECIDES for a stream of (key, id, valid) triples.

The kernel keeps the k best pairs, ordered by (sortable_u64(key), id), striped over 64 lanes x KPL registers.  Every offer
takes 64 triples.  The pairs that beat the k-th entry (all valid pairs while the list holds fewer than k) are counted; from
`kBatchMin` accepted pairs on the offer goes through `merge_batch`, below that each accepted pair is re-checked against the
moving threshold and inserted serially (`insert_uniform`).  The model repeats those decisions on a sorted Python list and
counts which route served which state of the list, so that a test case can state -- and the host test can assert -- which
code it reaches.  It models decisions and results, not lanes: the lane work is what the GPU tests compare against it.
"""
from __future__ import annotations

import bisect
import re
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

TOPK_HPP = Path(__file__).resolve().parents[1] / "vectordb-retrieval_amd" / "csrc" / "topk.hpp"
_SIGN = np.uint64(1 << 63)


def batch_min_from_header() -> int:
    """`kBatchMin` as the library is built with it: the branch conditions of the cases hold for THAT value."""
    m = re.search(r"kBatchMin\s*=\s*(\d+)\s*;", TOPK_HPP.read_text())
    assert m, "kBatchMin not found in csrc/topk.hpp"
    return int(m.group(1))


def kpl_for(k: int) -> int:
    kpl = 1
    while kpl * 64 < k:
        kpl *= 2
    return kpl


def sortable_u64(keys: np.ndarray) -> np.ndarray:
    """common.hpp: order-preserving map float64 -> uint64 (orders -0.0 below +0.0)."""
    u = np.ascontiguousarray(keys, np.float64).view(np.uint64)
    return np.where(u & _SIGN, ~u, u | _SIGN)


def unsortable_f64(u: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(u, np.uint64)
    return np.where(u & _SIGN, u & ~_SIGN, ~u).view(np.float64)


@dataclass
class Counts:
    batch_empty: int = 0      # merge_batch with n == 0
    batch_partial: int = 0    # merge_batch with 0 < n < k
    batch_full: int = 0       # merge_batch with n == k
    serial_partial: int = 0   # insert_uniform with n < k
    serial_full: int = 0      # insert_uniform with n == k
    serial_cross: int = 0     # insert_uniform whose position lies in a lower register than the last occupied slot
    accepted_full: set = field(default_factory=set)   # accepted pairs per offer, offers into a full list only

    def as_tuple(self):
        return (self.batch_empty, self.batch_partial, self.batch_full, self.serial_partial, self.serial_full, self.serial_cross)


def offer_stream(keys, ids, valid, k: int, batch_min: int = 12):
    """Run the stream (offered 64 at a time, in array order) through the model.

    Returns (keys float64 (n,), ids int64 (n,), Counts): the final list, n <= k entries ascending by (key, id)."""
    uk = sortable_u64(np.asarray(keys, np.float64).ravel())
    ids = np.ascontiguousarray(ids, np.int64).ravel()
    valid = np.ascontiguousarray(valid, bool).ravel()
    lst: list = []            # sorted (ukey, id) pairs, at most k
    c = Counts()
    for base in range(0, len(uk), 64):
        cu, ci, cv = uk[base:base + 64], ids[base:base + 64], valid[base:base + 64]
        n = len(lst)
        if n < k:
            want = cv
        else:
            tk, ti = lst[k - 1]
            want = cv & ((cu < np.uint64(tk)) | ((cu == np.uint64(tk)) & (ci < ti)))
        cnt = int(want.sum())
        if cnt == 0:
            continue
        if n == k:
            c.accepted_full.add(cnt)
        pairs = list(zip(cu[want].tolist(), ci[want].tolist()))     # ascending lane order
        if cnt >= batch_min:
            if n == 0:
                c.batch_empty += 1
            elif n < k:
                c.batch_partial += 1
            else:
                c.batch_full += 1
            lst = sorted(lst + pairs)[:k]
            continue
        for pr in pairs:
            n = len(lst)
            if n == k and not pr < lst[k - 1]:
                continue
            pos = bisect.bisect_left(lst, pr)
            last = n if n < k else k - 1                           # last occupied slot after the insertion
            if n < k:
                c.serial_partial += 1
            else:
                c.serial_full += 1
            if (pos >> 6) < (last >> 6):
                c.serial_cross += 1
            lst.insert(pos, pr)
            del lst[k:]
    out_k = unsortable_f64(np.array([p[0] for p in lst], np.uint64)) if lst else np.empty((0,), np.float64)
    out_i = np.array([p[1] for p in lst], np.int64)
    return out_k, out_i, c


def merge_stream(keys: np.ndarray, ids: np.ndarray, q: int):
    """The order in which merge_kernel offers query q of (nparts, nq, k) partial lists: element i = p * k + j."""
    kq = np.ascontiguousarray(keys[:, q, :]).ravel()
    iq = np.ascontiguousarray(ids[:, q, :]).ravel()
    return kq, iq, iq >= 0


def final_rows(list_keys: np.ndarray, list_ids: np.ndarray, k: int, metric: str):
    """The list as the entry points return it: float32 distances (ip: scores), -1 / +-FLT_MAX padding."""
    fmax = np.finfo(np.float32).max
    D = np.full((k,), fmax if metric == "l2" else -fmax, np.float32)
    I = np.full((k,), -1, np.int64)
    n = len(list_ids)
    with np.errstate(over="ignore"):
        D[:n] = (list_keys if metric == "l2" else -list_keys).astype(np.float32)
    I[:n] = list_ids
    return D, I


def lexsort_rows(keys: np.ndarray, ids: np.ndarray, k: int, metric: str):
    """Reference of the whole merge: np.lexsort over the valid entries of every query of (nparts, nq, k) lists."""
    nparts, nq, _ = keys.shape
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    for q in range(nq):
        kq, iq, v = merge_stream(keys, ids, q)
        kq, iq = kq[v], iq[v]
        o = np.lexsort((iq, kq))[:k]
        D[q], I[q] = final_rows(kq[o], iq[o], k, metric)
    return D, I

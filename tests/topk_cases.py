"""Synthetic partial lists for the select on its own (tests/test_gpu_topk.py), checked on the host by tests/test_topk_host.py.

Every case keeps the contract of the merge entry points: a part is ascending by (key, id), missing entries are
(+inf, -1) at its tail, and the ids of one query are distinct across the parts.  `ip` keys are negated scores, so the ip
cases hold negative and mixed-sign keys.  Zeros come with one sign per metric (+0.0 under l2, -0.0 under ip, as the kernels
produce them); mixed signed zeros are outside the contract and are not generated.

A case may carry `require`: the least branch counts (tests/topk_model.py) that EVERY query of it must reach.  The plain
orders (ascending, descending, shuffled parts) reach the serial route into a full list 0 to 5 times per query, so the
branch cases place, part by part, a chosen number of entries below the running threshold.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np

from .topk_model import kpl_for

KS = (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)
METRICS = ("l2", "ip")
JUNK = 1.0e6            # keys of entries that never enter a full list
IP_SHIFT = 5500.0       # l2-style keys live in about [3000, 6000); the ip form subtracts this: mixed signs


@dataclass
class Case:
    name: str
    metric: str
    k: int
    keys: np.ndarray                 # (nparts, nq, k) float64
    ids: np.ndarray                  # (nparts, nq, k) int64
    require: Optional[dict] = None   # least model counts of every query; "accepted": counts that must occur
    model: bool = True               # the host test runs the model over it (off for the 16 392-query case)

    @property
    def nparts(self):
        return self.keys.shape[0]

    @property
    def nq(self):
        return self.keys.shape[1]


def _seed(*parts) -> int:
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (2**31 - 1)
    return s


def assemble(queries, k: int):
    """queries[q][p] = (keys, ids) of at most k entries in any order -> padded (nparts, nq, k) arrays, parts sorted."""
    nq = len(queries)
    nparts = len(queries[0]) if nq else 0
    keys = np.full((nparts, nq, k), np.inf, np.float64)
    ids = np.full((nparts, nq, k), -1, np.int64)
    for q, parts in enumerate(queries):
        assert len(parts) == nparts
        for p, (pk, pi) in enumerate(parts):
            pk, pi = np.asarray(pk, np.float64), np.asarray(pi, np.int64)
            assert len(pk) == len(pi) <= k
            o = np.lexsort((pi, pk))
            keys[p, q, :len(pk)] = pk[o]
            ids[p, q, :len(pk)] = pi[o]
    return keys, ids


def check_contract(c: Case) -> None:
    """What the entry points document about their input."""
    for q in range(c.nq):
        seen = []
        for p in range(c.nparts):
            kk, ii = c.keys[p, q], c.ids[p, q]
            nv = int((ii >= 0).sum())
            assert (ii[:nv] >= 0).all() and (ii[nv:] == -1).all() and np.isposinf(kk[nv:]).all(), (c.name, q, p)
            assert not np.isnan(kk).any()
            a, b = kk[:nv], ii[:nv]
            assert ((a[1:] > a[:-1]) | ((a[1:] == a[:-1]) & (b[1:] > b[:-1]))).all(), (c.name, q, p)
            seen.append(b)
        allids = np.concatenate(seen) if seen else np.empty((0,), np.int64)
        assert len(np.unique(allids)) == len(allids), (c.name, q)
        z = c.keys[:, q][c.keys[:, q] == 0]
        assert len(z) == 0 or np.signbit(z).all() or not np.signbit(z).any(), (c.name, q)


# ---- branch cases ----------------------------------------------------------------------------------------------------------
# accepted pairs aimed at per head part (parts 2, 4, ..., 62); 11, 12 and 13 sit on both sides of kBatchMin
_TARGETS = (11, 12, 13, 3, 7, 1, 10, 30, 5, 2, 9, 64, 4, 8, 6, 20, 11, 12, 13, 1, 5, 3, 48, 2, 7, 9, 16, 4, 6, 10, 8)


def _branch_query(k: int, rng, nparts: int = 64):
    """k >= 63.  Part 0 fills the list partly (its tail is padding), part 1 fills it; every second later part opens with a
    head of entries that beat the running threshold -- sized so that the 64-pair offer that holds the head's chunk accepts
    the aimed count, the part's offset (p * k) mod 64 taken into account -- and goes on with entries that never enter."""
    pool = rng.permutation(nparts * k).astype(np.int64) + 7
    nid = 0
    parts = []
    top = []                                  # sorted (key, id): the k best of everything placed so far
    junk = JUNK
    ti = 0
    for p in range(nparts):
        if p < 2:
            m = k - k // 3 if p == 0 else k
            pk = 5000.0 + 1000.0 * rng.random(m)
            if p == 1:                        # part 1 repeats some keys of part 0: ties across parts, decided by id
                pk[: k // 8] = rng.choice(parts[0][0], k // 8, replace=False)
        else:
            a = 0
            if p % 2 == 0 and ti < len(_TARGETS):
                c = _TARGETS[ti]
                ti += 1
                off = (p * k) % 64
                if off + c <= 64:
                    a = c
                elif (64 - off) + c <= k // 2:
                    a = (64 - off) + c         # the first chunk takes 64 - off, the next one the aimed count
                else:
                    a = min(c, k // 2)
            lim = top[k - a][0] if a else 0.0   # heads stay below this key: they beat the threshold whenever they are offered
            head = top[0][0] - 40.0 + (lim - top[0][0] + 40.0) * rng.random(a)
            below = [t[0] for t in top[: k - a] if t[0] < lim]
            for j in range(a):                 # some heads repeat a key of the list
                if below and rng.random() < 0.2:
                    head[j] = below[int(rng.integers(len(below)))]
            pk = np.concatenate([head, junk + np.arange(k - a)])
            junk += k
        pi = pool[nid:nid + len(pk)]
        nid += len(pk)
        parts.append((pk, pi))
        top = sorted(top + list(zip(pk.tolist(), pi.tolist())))[:k]
    return parts


def _branch_query_small(k: int, rng, nchunks: int = 8):
    """k < 12: a 64-pair offer spans 64 / k parts, so the accepted count is set per offer: that many entries of the chunk
    lie below everything before them, the rest never enter."""
    counts = (64, 12, 3, 13, 11, 1, 20, 5)[:nchunks]
    n = 64 * nchunks
    keys = np.empty((n,), np.float64)
    lo = 5000.0
    for c, m in enumerate(counts):
        ck = JUNK + 64.0 * c + np.arange(64)
        if c == 0:
            ck = 5000.0 + 1000.0 * rng.random(64)
        else:
            lanes = rng.choice(64, m, replace=False)
            ck[lanes] = lo - 1.0 - 40.0 * rng.random(m)
        lo = min(lo, ck.min())
        keys[64 * c:64 * (c + 1)] = ck
    ids = rng.permutation(n).astype(np.int64) + 7
    return [(keys[p * k:(p + 1) * k], ids[p * k:(p + 1) * k]) for p in range(n // k)]


def branch_case(k: int, metric: str) -> Case:
    rng = np.random.default_rng(_seed("branch", k, metric))
    nq = 3
    if k >= 63:
        queries = [_branch_query(k, rng) for _ in range(nq)]
        require = dict(batch_full=4, batch_partial=1, serial_full=32, accepted=(11, 12, 13))
        if kpl_for(k) >= 2:
            require["serial_cross"] = 8
    else:
        queries = [_branch_query_small(k, rng) for _ in range(nq)]
        require = dict(batch_empty=1, batch_full=3, serial_full=3, accepted=(11, 12, 13))
    keys, ids = assemble(queries, k)
    if metric == "ip":
        keys = np.where(ids >= 0, keys - IP_SHIFT, keys)
    return Case(f"branch-k{k}-{metric}", metric, k, keys, ids, require)


# ---- the threshold slot ----------------------------------------------------------------------------------------------------
def threshold_case(k: int, metric: str) -> Case:
    """Entries that fall between slot k - 2 and slot k - 1 of the running list, offered right after the threshold was set:
    by a serial insertion into a full list (q0), by a batch merge into a full list (q1), by the serial insertion that fills
    the list (q2) and by the batch merge that fills it (q3).  Each such entry must enter; a threshold read one slot early
    rejects it.  Parts 1 to 3 hold these few entries and padding."""
    rng = np.random.default_rng(_seed("threshold", k, metric))
    shift = 0.0 if metric == "l2" else 5.0 * k + 100.0
    queries = []
    for q in range(4):
        ids = iter((rng.permutation(2 * k + 64) + 3).tolist())
        n0 = k if q < 2 else (k - 1 if q == 2 or k < 24 else k - 12)
        parts = [(100.0 + 10.0 * np.arange(n0) - shift, [next(ids) for _ in range(n0)])]
        top = sorted(zip(parts[0][0].tolist(), parts[0][1]))

        def probe():
            return [(top[k - 2][0] + top[k - 1][0]) / 2 if k >= 2 else top[0][0] - 1.0]

        def heads(m):                     # m entries low in the list, between its existing keys
            return (95.0 + 10.0 * np.arange(m) - shift).tolist()

        plan = {0: ("probe", "probe", "probe"), 1: ("heads", "probe", "none"), 2: ("fill", "probe", "probe"),
                3: ("fill", "probe", "none")}[q]
        for what in plan:
            if what == "probe" and len(top) >= k:
                pk = probe()
            elif what == "heads":
                pk = heads(min(12, k))
            elif what == "fill":
                pk = heads(k - n0)
            else:
                pk = []
            pi = [next(ids) for _ in pk]
            parts.append((pk, pi))
            top = sorted(top + list(zip(pk, pi)))[:k]
        queries.append(parts)
    keys, ids = assemble(queries, k)
    return Case(f"threshold-k{k}-{metric}", metric, k, keys, ids)


# ---- ties ------------------------------------------------------------------------------------------------------------------
def _deal(rng, nparts: int, k: int, n: int) -> np.ndarray:
    """Part of each of n <= nparts * k entries, at most k per part, in random order."""
    slots = np.repeat(np.arange(nparts), k)
    return rng.permutation(slots)[:n]


def ties_case(k: int, metric: str) -> Case:
    """Query 0 and 1: every key equal, ids alone decide.  Query 2 and 3: runs of 48 equal keys over the global order,
    placed so that one run straddles slot k - 1; 48 divides no multiple of 64 below 192, so runs straddle the 64-slot
    register boundaries, and every run is dealt over the parts at random."""
    rng = np.random.default_rng(_seed("ties", k, metric))
    nparts, sign = 5, (1.0 if metric == "l2" else -1.0)
    queries = []
    for q in range(4):
        n = nparts * k if q % 2 == 0 else nparts * k - k // 2 - 1
        ids = rng.permutation(4 * nparts * k)[:n].astype(np.int64)
        if q < 2:
            keys = np.full((n,), sign * 1.5)
        else:
            rank = np.argsort(np.argsort(ids))           # global order inside a run is the id order
            keys = ((rank - k + 24 + 48 * 64) // 48).astype(np.float64) * 0.25 - (0.0 if metric == "l2" else 16.125)
        part = _deal(rng, nparts, k, n)
        queries.append([(keys[part == p], ids[part == p]) for p in range(nparts)])
    keys, ids = assemble(queries, k)
    return Case(f"ties-k{k}-{metric}", metric, k, keys, ids)


# ---- short and empty lists -------------------------------------------------------------------------------------------------
def _rand_keys(rng, n: int, metric: str) -> np.ndarray:
    return rng.standard_normal(n) * 30.0 if metric == "ip" else rng.random(n) * 900.0


def short_case(k: int, metric: str) -> Case:
    """q0: every part's tail is padding.  q1: whole parts empty.  q2: fewer than k valid entries in total.  q3: none at all.
    q4: exactly k valid entries."""
    rng = np.random.default_rng(_seed("short", k, metric))
    nparts = 4
    lens = [
        [max(1, k - 1), k // 2, min(k, 3), k - k // 3],
        [0, k, 0, (k + 1) // 2],
        [k // 4, 0, k // 4, max(0, k // 4 - 1)],
        [0, 0, 0, 0],
        [k - 3 * (k // 4), k // 4, k // 4, k // 4],
    ]
    assert sum(lens[2]) < k and sum(lens[4]) == k
    queries = []
    for ln in lens:
        ids = rng.permutation(8 * k + 64)[:sum(ln)].astype(np.int64)
        keys = _rand_keys(rng, sum(ln), metric)
        cut = np.cumsum([0] + ln)
        queries.append([(keys[cut[p]:cut[p + 1]], ids[cut[p]:cut[p + 1]]) for p in range(nparts)])
    keys, ids = assemble(queries, k)
    return Case(f"short-k{k}-{metric}", metric, k, keys, ids)


def identity_case(k: int, metric: str) -> Case:
    """nparts = 1: the output is the input (its padding rewritten as +-FLT_MAX / -1)."""
    rng = np.random.default_rng(_seed("identity", k, metric))
    n = k - k // 5
    keys, ids = assemble([[(_rand_keys(rng, n, metric), rng.permutation(3 * k)[:n])]], k)
    return Case(f"identity-k{k}-{metric}", metric, k, keys, ids)


def noparts_case(k: int, metric: str) -> Case:
    return Case(f"noparts-k{k}-{metric}", metric, k, np.empty((0, 3, k), np.float64), np.empty((0, 3, k), np.int64))


# ---- key values ------------------------------------------------------------------------------------------------------------
def values_case(k: int, metric: str) -> Case:
    """q0: +inf (and -inf under ip) as real keys with valid ids among ordinary ones.  q1: subnormals.  q2: neighbours in the
    last bit.  q3: zeros of the metric's sign among keys of the sign(s) the metric produces."""
    rng = np.random.default_rng(_seed("values", k, metric))
    nparts, ip = 3, metric == "ip"
    n = nparts * k - k // 3
    sub = np.float64(5e-324)
    queries = []
    for q in range(4):
        if q == 0:
            keys = _rand_keys(rng, n, metric)
            keys[0::3] = np.inf
            if ip:
                keys[1::4] = -np.inf
        elif q == 1:
            keys = rng.integers(1, 40, n).astype(np.float64) * sub
            keys[1::5] = (20.0 if ip else 0.0) * sub
            if ip:
                keys = keys - 20.0 * sub
                keys = np.where(keys == 0, -0.0, keys)
        elif q == 2:
            base = -1.0 if ip else 1.0
            keys = np.full((n,), base)
            for _ in range(6):
                up = rng.random(n) < 0.5
                keys = np.where(up, np.nextafter(keys, np.inf), np.nextafter(keys, -np.inf))
        else:
            keys = _rand_keys(rng, n, metric)
            keys[0::2] = -0.0 if ip else 0.0
        ids = rng.permutation(4 * n + 8)[:n].astype(np.int64)
        part = _deal(rng, nparts, k, n)
        queries.append([(keys[part == p], ids[part == p]) for p in range(nparts)])
    keys, ids = assemble(queries, k)
    return Case(f"values-k{k}-{metric}", metric, k, keys, ids)


# ---- launch shape ----------------------------------------------------------------------------------------------------------
def many_queries_case() -> Case:
    """16 385 + 7 queries: the merge grid is capped at 4096 workgroups of 4 waves, so the slot loop takes a second trip and
    the last workgroup is partly idle.  k = 3, two parts; small integer keys, so ties abound."""
    rng = np.random.default_rng(_seed("many"))
    nq, k = 16385 + 7, 3
    keys = rng.integers(0, 5, (2, nq, k)).astype(np.float64)
    perm = np.argsort(rng.random((nq, 2 * k)), axis=1) + (np.arange(nq)[:, None] % 9)
    ids = np.stack([perm[:, :k], perm[:, k:]]).astype(np.int64)
    short = rng.random((2, nq)) < 0.2                       # some lists are short
    ids[short, k - 1] = -1
    o = np.lexsort((ids, np.where(ids >= 0, keys, np.inf)), axis=-1)
    keys, ids = np.take_along_axis(keys, o, -1), np.take_along_axis(ids, o, -1)
    keys[ids < 0] = np.inf
    return Case("many-queries-k3-l2", "l2", k, keys, ids, model=False)


KINDS = dict(branch=branch_case, threshold=threshold_case, ties=ties_case, short=short_case, identity=identity_case,
             noparts=noparts_case, values=values_case)


def case_names():
    names = []
    for k in KS:
        for metric in METRICS:
            names += [f"{kind}-k{k}-{metric}" for kind in KINDS]
    return names + ["many-queries-k3-l2"]


@lru_cache(maxsize=None)
def case_by_name(name: str) -> Case:
    if name.startswith("many"):
        return many_queries_case()
    kind, kk, metric = name.split("-")
    return KINDS[kind](int(kk[1:]), metric)

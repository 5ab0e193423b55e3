"""Call sequences on ONE long-lived handle, the host model that says what every call must answer, the generator of the committed
sequences, the driver that runs them, and two fake indexes that can be told to keep one piece of state too long.
Shared by tests/test_sequence_host.py and tests/test_gpu_sequences.py.  NumPy only; nothing here needs a GPU.

A step is (op, args).  The MODEL holds what include/vdbhip.h calls the state of a handle -- the rows so far, id_base, centroids, list
of every row, nprobe, the installed mask or None, the last range result or None -- updates it by the header's rules and answers every
step from a reference that exists already: oracle.knn / ivf_search / pair_keys, range_cases.expected, filter_cases.reference,
ivf_filter_cases.reference, ivf_range_cases.full_lists + cut.  It holds no arithmetic of its own.

The queries of a sequence are prefixes of two fixed batches, A and B (`qset` 0 / 1), so that a batch size can repeat with other
queries; on the byte-valued flat shape A is an integer batch and B is not, so the scan dtype alternates per call.

The DRIVER calls the methods of vdbhip.FlatIndex / IVFFlatIndex by name; the device forms, the raw vdb_range_results call and the
packed filter words with their tail bits set go through torch and vdbhip._ffi.  On a fake index they take the host form of the same
call: a fake has no device.  The fakes answer by brute force over float64 keys made with NumPy (the chain of
filter_cases.brute_reference, all queries at once) and keep their own state by the same contract."""
from __future__ import annotations

import os
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from tests import filter_cases as fc
from tests import ivf_filter_cases as ic
from tests import ivf_range_cases as irc
from tests import range_cases as rc

F32 = np.float32
NQS = (1, 5, 16, 17, 64, 130)
NQMAX = max(NQS)
KS = (1, 10, 100)
NPROBES = (1, 8, 16)
RANKS = ("0", "10", "half")
ID_BASES = (0, 1_000_003)
STEPS = 40
MASK_K = 10                                     # the k that places filter_cases' admits-(k - 1 / k / k + 1) masks
FLAT_MASKS = ("all-ones", "all-zeros", "row-0", "row-last", "word-edges", "alternating", "bin-cleared", "chunk-cleared",
              "last-span-only", "random-0.5", "random-0.1", "random-0.01", "admits--1", "admits-+0", "admits-+1")
IVF_MASKS = ("all-ones", "all-zeros", "random-0.5", "random-0.1", "random-0.01", "id-run", "three-lists-cleared", "one-list-only",
             "single-row", "last-row")
FILTER_FORMS = ("bool", "ids", "words")
SPARSE_DEFAULT = float(1 << 13)                 # kFilterSparsePairsDefault (csrc/filter_plan.hpp)
FLAT_OPTIONS = (("force_path", (0, 1, 2)), ("small_batch", (0, 1)), ("fused_stats", (0, 1)), ("scan_pair", (0, 1)),
                ("spans_per_chunk", (0, 2, 4)), ("panel_dtype", (0, 1)), ("range_bitmap_mb", (0, 1)),
                ("filter_sparse_pairs", (0.0, SPARSE_DEFAULT, float("inf"))), ("timing", (1,)))
IVF_OPTIONS = (("force_path", (0, 1, 2, 3)), ("ivf_part", (0, 1, 4)), ("ivf_nw", (0, 2, 4, 8)), ("ivf_min_batch", (1, 32, 100000)),
               ("range_bitmap_mb", (0, 1)), ("i8_ring", (0, 2, 4, 8)), ("small_batch", (0, 1)), ("timing", (1,)))

NOT_BUILT, NO_FILTER, NO_RANGE = "not been built", "no filter", "no range result"


# ---- steps and shapes ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Step:
    op: str
    args: Tuple = ()

    def line(self) -> str:
        return f"{self.op}({', '.join(repr(a) for a in self.args)})"


@dataclass(frozen=True)
class Shape:
    kind: str                       # "flat" | "ivf"
    name: str
    n: int
    d: int
    blocks: Tuple[int, ...]         # rows of the index after the add and after each append
    rows: str = "gauss"             # "gauss" | "bytes" (integers 0..255)
    qkinds: Tuple[str, str] = ("gauss", "gauss")      # query batches A and B: "gauss" | "int" | "float" (bytes + noise)
    force: int = 2                  # flat: option "force_path" before the first add (filter_cases.Route.force)
    span: int = 512                 # flat: rows per span of the scan copies (filter_cases.masks)
    nlist: int = 0
    metrics: Tuple[str, ...] = ("l2", "ip")
    first_centroids: bool = True

    @property
    def id(self):
        return self.name

    def reduced(self) -> "Shape":
        """a few hundred rows for the host tests: the same blocks, forty (IVF: fifty) times smaller"""
        f = 50 if self.kind == "ivf" else (10 if self.n <= 5000 else 40)
        blocks = tuple(max(b // f, 70 + 10 * i) for i, b in enumerate(self.blocks))
        return replace(self, n=blocks[-1], blocks=blocks, nlist=min(self.nlist, 16))


FLAT_SHAPES = (
    Shape("flat", "x16-f16", 20000, 32, (12000, 16000, 20000)),
    Shape("flat", "x16-i8", 20000, 32, (12000, 16000, 20000), "bytes", ("int", "float")),
    Shape("flat", "p16-kloop", 4100, 136, (1500, 4100), span=1024),       # (the first block is below the 2048 rows of the K-loop scan)
    Shape("flat", "dense", 3000, 16, (1000, 2000, 3000), force=0),
    Shape("flat", "s32-small", 9000, 24, (4000, 9000)),
    Shape("flat", "x16-f16-d30", 20000, 30, (15000, 20000)),               # (D no multiple of 4: padded queries)
)
IVF_SHAPES = (
    Shape("ivf", "f16-d64", 20000, 64, (12000, 16000, 20000), nlist=64),
    Shape("ivf", "i8-d64-int", 20000, 64, (12000, 16000, 20000), "bytes", ("int", "int"), nlist=64),
    Shape("ivf", "i8-d64-float", 20000, 64, (12000, 20000), "bytes", ("float", "float"), nlist=64),
    Shape("ivf", "kloop-d200", 30000, 200, (20000, 30000), nlist=64, metrics=("l2",), first_centroids=False),
)
SHAPES = {"flat": FLAT_SHAPES, "ivf": IVF_SHAPES}
SEEDS = {"flat": 6, "ivf": 6}      # (five IVF seeds leave two ordered pairs unseen)


def shape_of(kind: str, name: str) -> Shape:
    return next(s for s in SHAPES[kind] if s.name == name)


def metric_of(shape: Shape, seed: int) -> str:
    """both metrics where the shape lists both: they alternate with the seed"""
    return shape.metrics[seed % len(shape.metrics)]


def committed(kind: str):
    """[(shape, seed)] in the order the generator walks them (its coverage state runs through this list)"""
    return [(s, seed) for s in SHAPES[kind] for seed in range(SEEDS[kind])]


def _bytes(rng, n, d):
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(F32)


@lru_cache(maxsize=4)
def data(shape: Shape):
    """(X (n, d), (QA, QB) (130, d) each, (C0, C1) centroid sets or None), read-only"""
    rng = np.random.default_rng([73, shape.n, shape.d, shape.rows == "bytes", len(shape.qkinds[1])])
    X = _bytes(rng, shape.n, shape.d) if shape.rows == "bytes" else rng.standard_normal((shape.n, shape.d)).astype(F32)
    Q = []
    for qk in shape.qkinds:
        if qk == "gauss":
            Q.append(rng.standard_normal((NQMAX, shape.d)).astype(F32))
        else:
            q = _bytes(rng, NQMAX, shape.d)
            Q.append(q if qk == "int" else q + 3 * rng.standard_normal((NQMAX, shape.d)).astype(F32))
    C = None
    if shape.kind == "ivf":
        first = shape.blocks[0]
        pick = np.arange(2 * shape.nlist) if shape.first_centroids else np.sort(rng.choice(first, 2 * shape.nlist, replace=False))
        C = (X[pick[0::2]].copy(), X[pick[1::2]].copy())
        for c in C:
            c.flags.writeable = False
    for a in [X] + Q:
        a.flags.writeable = False
    return X, tuple(Q), C


# ---- what a step is expected to answer -------------------------------------------------------------------------------------------------
@dataclass
class Plan:
    """what the driver passes to the call (`inputs`) and what the call must answer: ("arrays", (a, ...)) | ("value", v) |
    ("error", "state" | "invalid", message fragment) | ("none",); "arrays" hold None in a model without references (the generator's)"""
    inputs: dict
    expect: tuple


def _err(cls, fragment):
    return ("error", cls, fragment)


def _rank(rank: str, count: int) -> int:
    return {"0": 0, "10": 10, "half": count // 2}[rank]


def radius_at(keys_of_query, metric, rank):
    """test_gpu_range._radius_at: the float32 distance of the query's rank-th nearest row (0-based)"""
    d = np.sort((keys_of_query if metric == "l2" else -keys_of_query).astype(F32))
    rank = min(rank, len(d) - 1)
    return float(d[rank] if metric == "l2" else d[::-1][rank])


def rerank_candidates(n: int, id_base: int, nq: int, ncand: int, salt: int):
    """(nq, ncand) int64: distinct rows per query, one slot in ten empty (-1)"""
    rng = np.random.default_rng([79, n, nq, ncand, salt])
    cand = np.stack([rng.permutation(n)[:ncand] for _ in range(nq)]).astype(np.int64)
    if cand.shape[1] < ncand:
        cand = np.concatenate([cand, np.full((nq, ncand - cand.shape[1]), -1, np.int64)], axis=1)
    cand = np.where(cand >= 0, cand + id_base, -1)
    cand[rng.random(cand.shape) < 0.1] = -1
    return cand


def rerank_reference(pair_keys, X, Q, cand, k, metric, id_base):
    """top k by (canonical float64 key, id) among the candidates (tests/test_gpu_large_k._rerank_reference)"""
    ok = cand >= 0
    keys = pair_keys(X, Q, np.where(ok, cand - id_base, 0), metric)
    D = np.full((len(Q), k), fc.pad_value(metric), F32)
    I = np.full((len(Q), k), -1, np.int64)
    for q in range(len(Q)):
        kq, iq = keys[q][ok[q]], cand[q][ok[q]]
        o = np.lexsort((iq, kq))[:k]
        D[q, :len(o)] = (kq[o] if metric == "l2" else -kq[o]).astype(F32)
        I[q, :len(o)] = iq[o]
    return D, I


def _with_hundred(masks, n):
    """+ "hundred": a hundred seeded rows, few enough for the sparse list of a flat filter (the directed sequences install it)"""
    m = np.zeros(n, np.bool_)
    m[np.random.default_rng([89, n]).choice(n, min(100, n), replace=False)] = True
    m.flags.writeable = False
    return dict(masks, hundred=m)


class _Model:
    """what both kinds of handle share: the data, the query batches, the filter and the range result"""

    def __init__(self, shape: Shape, metric: str, refs=None):
        self.shape, self.metric, self.refs = shape, metric, refs
        self.X, self.Q, self.C = data(shape)
        self.n = 0                      # rows a search covers
        self.stat_n = 0                 # vdb_stats.ntotal
        self.id_base = 0
        self.block = 0                  # blocks of the shape that are in
        self.mask = None                # the installed filter: a bool mask, or None
        self.range = None               # the last range result (lims, D, I), or None
        self.ranges = 0                 # range searches so far
        self.empty_search_used = False
        self.max_nq = 0
        self._cache = {}

    def queries(self, nq, qset):
        return self.Q[qset][:nq]

    def _cached(self, key, make):
        if key not in self._cache:
            if len(self._cache) > 6:
                self._cache.pop(next(iter(self._cache)))
            self._cache[key] = make()
        return self._cache[key]

    def _drop(self, filt=True, rng=True):
        if filt:
            self.mask = None
        if rng:
            self.range = None

    def _arrays(self, make):
        return ("arrays", make() if self.refs is not None else None)

    def _set_mask(self, name):
        self.mask = self.masks()[name] if self.refs is not None else name

    def _filter_inputs(self, name, form):
        if self.refs is None:
            return {"form": form}
        m = self.masks()[name]
        if form == "ids":
            return {"form": form, "allowed": np.flatnonzero(m).astype(np.int64) + self.id_base}
        if form in ("words", "device"):
            return {"form": form, "words": fc.tail_set_words(m), "nbits": len(m)}
        return {"form": form, "allowed": m}

    def _count(self):
        return int(self.mask.sum()) if self.refs is not None else None

    def apply(self, step: Step) -> Plan:
        plan = getattr(self, "_" + step.op)(*step.args)
        if step.op in BATCH_OPS or step.op == "reserve":
            if plan.expect[0] != "error":
                self.max_nq = max(self.max_nq, step.args[0])
        return plan


class FlatModel(_Model):
    def __init__(self, shape, metric, refs=None):
        super().__init__(shape, metric, refs)
        self.lsh = False

    @property
    def live(self):
        return self.n > 0

    def allowed(self, op: str) -> bool:
        if op == "add":
            return self.n == 0
        if op == "append":
            return self.n > 0 and self.block < len(self.shape.blocks)
        if op in ("reset", "set_option", "search_filtered", "range_results_again", "filter_count"):
            return True
        if op == "search":
            return self.n > 0 or not self.empty_search_used
        if op == "become_lsh":
            return self.n > 0 and not self.lsh
        return self.n > 0

    def masks(self):
        return self._cached(("masks", self.n), lambda: _with_hundred(fc.masks(self.n, MASK_K, self.shape.span), self.n))

    def keys(self, qset):
        def make():
            rows = np.tile(np.arange(self.n, dtype=np.int64), (NQMAX, 1))
            return self.refs.pair_keys(self.X[:self.n], self.Q[qset], rows, self.metric)
        return self._cached(("keys", self.n, qset), make)

    # -- rows
    def _add(self, id_base):
        end = self.shape.blocks[0]
        self.n = self.stat_n = end
        self.block, self.id_base = 1, id_base
        self._drop()
        return Plan({"rows": self.X[:end], "id_base": id_base}, ("none",))

    def _append(self):
        a, b = self.n, self.shape.blocks[self.block]
        self.n = self.stat_n = b
        self.block += 1
        self._drop()
        return Plan({"rows": self.X[a:b], "id_base": self.id_base}, ("none",))

    def _append_empty(self):
        self._drop()                    # (an empty append is an add that passed its checks)
        return Plan({"rows": self.X[:0], "id_base": self.id_base}, ("none",))

    def _add_refused(self):
        return Plan({"rows": self.X[:7], "id_base": self.id_base + 5}, _err("invalid", "id base"))     # (changes nothing)

    def _reset(self):
        self.n = self.stat_n = self.block = 0
        self._drop()
        return Plan({}, ("none",))

    def _become_lsh(self):
        self.lsh = True
        self._drop(rng=False)           # (a change of kind drops the filter; the range result is already materialised)
        return Plan({"nbits": 64, "seed": 5}, ("none",))

    def _set_option(self, name, value):
        self._drop()
        return Plan({}, ("none",))

    def _reserve(self, nq, k):
        return Plan({}, ("none",))

    # -- searches
    def _search(self, nq, k, qset):
        Q = self.queries(nq, qset)
        if self.n == 0:
            self.empty_search_used = True
            return Plan({"Q": Q}, _err("state", NOT_BUILT))
        return Plan({"Q": Q}, self._arrays(lambda: self.refs.knn(self.X[:self.n], Q, k, self.metric, id_base=self.id_base)))

    _search_device_pair = _search

    def _rerank(self, nq, ncand, k, qset):
        Q = self.queries(nq, qset)
        cand = rerank_candidates(self.n, self.id_base, nq, ncand, k + qset)
        return Plan({"Q": Q, "cand": cand},
                    self._arrays(lambda: rerank_reference(self.refs.pair_keys, self.X[:self.n], Q, cand, k, self.metric, self.id_base)))

    def _range_search(self, nq, rank, qset):
        Q = self.queries(nq, qset)
        self.ranges += 1
        if self.refs is None:
            self.range = True
            return Plan({"Q": Q, "radius": 0.0}, ("arrays", None))
        keys = self.keys(qset)
        radius = radius_at(keys[0], self.metric, _rank(rank, self.n))
        self.range = rc.expected(keys[:nq], radius, self.metric, self.id_base)
        return Plan({"Q": Q, "radius": radius}, ("arrays", self.range))

    _range_search_device = _range_search

    def _range_results_again(self):
        if self.range is None:
            return Plan({"total": 0}, _err("state", NO_RANGE))
        if self.refs is None:
            return Plan({"total": 0}, ("arrays", None))
        return Plan({"total": int(self.range[0][-1])}, ("arrays", self.range[1:]))

    # -- filter
    def _set_filter(self, name, form):
        inputs = self._filter_inputs(name, form)
        self._set_mask(name)
        return Plan(inputs, ("none",))

    def _set_filter_device(self, name):
        return self._set_filter(name, "device")

    def _set_filter_refused(self):
        words = np.zeros((self.n + 31) // 32, np.uint32)
        return Plan({"words": words, "nbits": self.n - 1}, _err("invalid", "nbits"))                  # (keeps an installed filter)

    def _clear_filter(self):
        self._drop(rng=False)
        return Plan({}, ("none",))

    def _filter_count(self):
        if self.mask is None:
            return Plan({}, _err("state", NO_FILTER))
        return Plan({}, ("value", self._count()))

    def _search_filtered(self, nq, k, qset):
        Q = self.queries(nq, qset)
        if self.n == 0:
            return Plan({"Q": Q}, _err("state", NOT_BUILT))
        if self.mask is None:
            return Plan({"Q": Q}, _err("state", NO_FILTER))
        mask = self.mask
        return Plan({"Q": Q}, self._arrays(lambda: fc.reference(self.refs.knn, self.X[:self.n], Q, k, self.metric, mask, self.id_base)))


class IvfModel(_Model):
    """IVF-Flat with injected centroids.  What ivf.inc does to rows that are already filed:
      vdb_ivf_set_centroids   keeps them in memory (vdb_stats.ntotal stays) but the index is no longer built: every IVF call answers
                              "not built" until the next vdb_ivf_add, which replaces them (it does not append);
      vdb_add                 replaces them by its own rows in insertion order; vdb_search answers over those rows, the IVF calls
                              answer "not built", and the next vdb_ivf_add replaces them again."""

    def __init__(self, shape, metric, refs=None):
        super().__init__(shape, metric, refs)
        self.cset = 0
        self.nprobe = 1
        self.lor = None
        self.epoch = 0                  # counts the adds: the lists changed
        self.flat_n = 0                 # rows of a vdb_add on this handle
        self.flat_id_base = 0

    @property
    def live(self):
        return self.n > 0

    def allowed(self, op: str) -> bool:
        if op in ("add", "add_assigned"):
            return not self.live
        if op == "append":
            return self.live and self.block < len(self.shape.blocks)
        if op in ("reset", "set_nprobe", "set_option", "set_centroids", "flat_search", "search_filtered", "range_results_again",
                  "filter_count"):
            return True
        if op == "search":
            return self.live or not self.empty_search_used
        return self.live

    @property
    def centroids(self):
        return self.C[self.cset]

    def _assign(self, rows):
        if self.refs is None:
            return None
        return self.refs.ivf_assign(self.centroids, rows, self.metric)

    def probed(self):
        order = ic.nearest_lists(self.centroids, self.Q[0][0], self.metric, self.shape.nlist)
        sizes = np.bincount(self.lor, minlength=self.shape.nlist)
        return np.array([l for l in order if sizes[l] > 0][:3])

    def masks(self):
        return self._cached(("masks", self.epoch), lambda: _with_hundred(ic.masks(self.n, self.lor, self.probed()), self.n))

    def full(self, qset):
        key = ("full", self.epoch, self.cset, self.nprobe, qset)
        return self._cached(key, lambda: irc.full_lists(self.refs.ivf_search, self.X[:self.n], self.centroids, self.lor, self.Q[qset],
                                                        self.nprobe, self.metric))

    # -- rows
    def _filed(self, end, id_base, lor):
        self.n = self.stat_n = end
        self.id_base, self.lor = id_base, lor
        self.flat_n = 0
        self.epoch += 1
        self._drop()

    def _add(self, id_base):
        end = self.shape.blocks[0]
        self.block = 1
        self._filed(end, id_base, self._assign(self.X[:end]))
        return Plan({"rows": self.X[:end], "id_base": id_base, "lor": None}, ("none",))

    def _add_assigned(self, id_base):
        end = self.shape.blocks[0]
        self.block = 1
        lor = self._assign(self.X[:end])
        if lor is not None:             # (any list is legal: every seventh row moves one list on)
            lor = lor.copy()
            lor[::7] = (lor[::7] + 1) % self.shape.nlist
        self._filed(end, id_base, lor)
        return Plan({"rows": self.X[:end], "id_base": id_base, "lor": lor}, ("none",))

    def _append(self):
        a, b = self.n, self.shape.blocks[self.block]
        self.block += 1
        new = self._assign(self.X[a:b])
        self._filed(b, self.id_base, None if new is None else np.concatenate([self.lor, new]))
        return Plan({"rows": self.X[a:b], "id_base": self.id_base, "lor": None}, ("none",))

    def _append_empty(self):
        self._drop()
        return Plan({"rows": self.X[:0], "id_base": self.id_base, "lor": None}, ("none",))

    def _add_refused(self, form):
        if form == "id_base":
            return Plan({"rows": self.X[:7], "id_base": self.id_base + 5, "lor": None}, _err("invalid", "id base"))
        lor = np.zeros(7, np.int32)
        lor[3] = self.shape.nlist
        return Plan({"rows": self.X[:7], "id_base": self.id_base, "lor": lor}, _err("invalid", "could not be assigned"))

    def _reset(self):
        self.n = self.stat_n = self.block = self.flat_n = 0
        self._drop()
        return Plan({}, ("none",))

    def _set_nprobe(self, nprobe):
        self.nprobe = nprobe            # (keeps the filter and the range result)
        return Plan({}, ("none",))

    def _set_centroids(self):
        self.cset ^= 1
        self.n = self.block = 0         # (the filed rows linger until the next add replaces them: stat_n stays)
        self._drop()
        return Plan({"C": self.centroids}, ("none",))

    def _flat_add(self, id_base):
        end = self.shape.blocks[0]
        self.n = self.block = 0
        self.flat_n = self.stat_n = end
        self.flat_id_base = id_base
        self._drop()
        return Plan({"rows": self.X[:end], "id_base": id_base}, ("none",))

    def _set_option(self, name, value):
        self._drop()
        return Plan({}, ("none",))

    # -- searches
    def _flat_search(self, nq, k, qset):
        Q = self.queries(nq, qset)
        if self.flat_n == 0:
            return Plan({"Q": Q}, _err("state", NOT_BUILT))
        n, base = self.flat_n, self.flat_id_base
        return Plan({"Q": Q}, self._arrays(lambda: self.refs.knn(self.X[:n], Q, k, self.metric, id_base=base)))

    def _search(self, nq, k, qset):
        Q = self.queries(nq, qset)
        if not self.live:
            self.empty_search_used = True
            return Plan({"Q": Q}, _err("state", NOT_BUILT))
        return Plan({"Q": Q}, self._arrays(lambda: self.refs.ivf_search(self.X[:self.n], self.centroids, self.lor, Q, k, self.nprobe,
                                                                        self.metric, id_base=self.id_base)))

    _search_device_pair = _search

    def _range_search(self, nq, rank, qset):
        Q = self.queries(nq, qset)
        self.ranges += 1
        if self.refs is None:
            self.range = True
            return Plan({"Q": Q, "radius": 0.0}, ("arrays", None))
        d, i = self.full(qset)
        count = int((i[0] >= 0).sum())
        radius = float(d[0, min(_rank(rank, count), count - 1)]) if count else 0.0
        self.range = irc.cut((d[:nq], i[:nq]), self.lor, radius, self.metric, self.id_base)
        return Plan({"Q": Q, "radius": radius}, ("arrays", self.range))

    _range_search_device = _range_search

    def _range_results_again(self):
        if not self.live:
            return Plan({"total": 0}, _err("state", NOT_BUILT))
        if self.range is None:
            return Plan({"total": 0}, _err("state", NO_RANGE))
        if self.refs is None:
            return Plan({"total": 0}, ("arrays", None))
        return Plan({"total": int(self.range[0][-1])}, ("arrays", self.range[1:]))

    # -- filter
    def _set_filter(self, name, form):
        inputs = self._filter_inputs(name, form)
        self._set_mask(name)
        return Plan(inputs, ("none",))

    def _set_filter_device(self, name):
        return self._set_filter(name, "device")

    def _set_filter_refused(self):
        words = np.zeros((self.n + 31) // 32, np.uint32)
        return Plan({"words": words, "nbits": self.n - 1}, _err("invalid", "nbits"))

    def _clear_filter(self):
        self._drop(rng=False)
        return Plan({}, ("none",))

    def _filter_count(self):
        if not self.live:
            return Plan({}, _err("state", NOT_BUILT))
        if self.mask is None:
            return Plan({}, _err("state", NO_FILTER))
        return Plan({}, ("value", self._count()))

    def _search_filtered(self, nq, k, qset):
        Q = self.queries(nq, qset)
        if not self.live:
            return Plan({"Q": Q}, _err("state", NOT_BUILT))
        if self.mask is None:
            return Plan({"Q": Q}, _err("state", NO_FILTER))
        mask = self.mask
        return Plan({"Q": Q}, self._arrays(lambda: ic.reference(self.refs.ivf_search, self.X[:self.n], self.centroids, self.lor, Q, k,
                                                                self.nprobe, self.metric, mask, self.id_base)))


def model_for(shape: Shape, metric: str, refs=None):
    return (FlatModel if shape.kind == "flat" else IvfModel)(shape, metric, refs)


# ---- vocabularies and the coverage conditions -----------------------------------------------------------------------------------------
OPS = {
    "flat": ("add", "append", "append_empty", "add_refused", "reset", "search", "search_device_pair", "range_search",
             "range_search_device", "range_results_again", "set_filter", "set_filter_device", "set_filter_refused", "clear_filter",
             "filter_count", "search_filtered", "rerank", "reserve", "set_option", "become_lsh"),
    "ivf": ("add", "add_assigned", "append", "append_empty", "add_refused", "reset", "set_nprobe", "set_centroids", "flat_add",
            "flat_search", "search", "search_device_pair", "search_filtered", "range_search", "range_search_device",
            "range_results_again", "set_filter", "set_filter_device", "set_filter_refused", "clear_filter", "filter_count", "set_option"),
}
BATCH_OPS = ("search", "search_device_pair", "search_filtered", "range_search", "range_search_device", "rerank", "flat_search")
INSTALLS = ("set_filter", "set_filter_device")
RANGE_SEARCHES = ("range_search", "range_search_device")
PROBES = ("search_filtered", "range_results_again", "filter_count")
# the ops that drop the filter, the range result or both -- and set_nprobe, which must keep both: each is followed by every probe
# somewhere in the seed set, and it counts only where the op ran while the state the probe asks about was there to lose
DROPPERS = {"flat": ("append", "append_empty", "reset", "set_option", "become_lsh", "clear_filter"),
            "ivf": ("append", "append_empty", "reset", "set_option", "set_centroids", "flat_add", "clear_filter", "set_nprobe")}
# state an op leaves behind, whatever came before it: "rows" (a searchable index) or "empty"; the others leave what they found
_AFTER = {"flat": {"rows": ("add", "append", "append_empty", "add_refused", "search_device_pair", "range_search", "range_search_device",
                            "set_filter", "set_filter_device", "set_filter_refused", "clear_filter", "rerank", "reserve", "become_lsh"),
                   "empty": ("reset",)},
          "ivf": {"rows": ("add", "add_assigned", "append", "append_empty", "add_refused", "search_device_pair", "range_search",
                           "range_search_device", "set_filter", "set_filter_device", "set_filter_refused", "clear_filter"),
                  "empty": ("reset", "set_centroids", "flat_add")}}
_NEEDS = {"flat": {"empty": ("add",),
                   "rows": tuple(o for o in OPS["flat"] if o not in ("add", "reset", "search", "search_filtered", "range_results_again",
                                                                     "filter_count", "set_option"))},
          "ivf": {"empty": ("add", "add_assigned"),
                  "rows": ("append", "append_empty", "add_refused", "flat_add", "search_device_pair", "range_search", "range_search_device",
                           "set_filter", "set_filter_device", "set_filter_refused", "clear_filter")}}


def feasible_pairs(kind: str):
    """every ordered pair (a, b) of op classes that the preconditions allow somewhere: b must not need what a has just ruled out"""
    out = set()
    for a in OPS[kind]:
        for b in OPS[kind]:
            if a in _AFTER[kind]["rows"] and b in _NEEDS[kind]["empty"]:
                continue
            if a in _AFTER[kind]["empty"] and b in _NEEDS[kind]["rows"]:
                continue
            if a == b == "become_lsh":          # (a handle becomes an LSH index once)
                continue
            out.add((a, b))
    return out


@dataclass
class Coverage:
    pairs: set
    probes: dict                    # dropper -> probes seen after it, before the next install or range search (see `note`)

    @staticmethod
    def empty(kind):
        return Coverage(set(), {d: set() for d in DROPPERS[kind]})

    def copy(self):
        return Coverage(set(self.pairs), {d: set(p) for d, p in self.probes.items()})

    @staticmethod
    def note(probes, open_droppers, op):
        """a probe counts for an open dropper that ran while the state it asks about was held"""
        for d, (had_filter, had_range) in open_droppers.items():
            if had_range if op == "range_results_again" else had_filter:
                probes[d].add(op)

    def add(self, kind, steps, installed, ranged):
        """`installed`, `ranged`: dry_run's flags, the state before every step"""
        open_droppers = {}
        for i, s in enumerate(steps):
            if i:
                self.pairs.add((steps[i - 1].op, s.op))
            if s.op in INSTALLS or s.op in RANGE_SEARCHES:
                open_droppers = {}
            if s.op in PROBES:
                Coverage.note(self.probes, open_droppers, s.op)
            if s.op in DROPPERS[kind]:
                open_droppers[s.op] = (installed[i], ranged[i])
        return self


def same_size_pair(steps, answers):
    """index of the first step that repeats its predecessor's batch size with the other query batch, both answering; None"""
    for i in range(1, len(steps)):
        a, b = steps[i - 1], steps[i]
        if a.op in BATCH_OPS and b.op in BATCH_OPS and a.op != "rerank" and b.op != "rerank" and answers[i - 1] and answers[i] \
                and a.args[0] == b.args[0] and a.args[-1] != b.args[-1]:
            return i
    return None


def regrowth_step(steps, answers, installed):
    """index of the first answering batch larger than every earlier batch while a filter is installed; None"""
    top = 0
    for i, s in enumerate(steps):
        nq = s.args[0] if (s.op in BATCH_OPS or s.op == "reserve") and answers[i] else 0
        if nq > top:
            if top and installed[i] and s.op in BATCH_OPS:
                return i
            top = nq
    return None


def dry_run(shape: Shape, metric: str, steps):
    """(answers, installed, ranged): per step, does it answer (no expected refusal), is a filter installed / a range result held BEFORE it"""
    m = model_for(shape, metric)
    answers, installed, ranged = [], [], []
    for s in steps:
        installed.append(m.mask is not None)
        ranged.append(m.range is not None)
        answers.append(m.apply(s).expect[0] != "error")
    return answers, installed, ranged


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
_WEIGHT = {"search": 3.0, "search_filtered": 3.0, "range_search": 2.0, "set_filter": 3.0, "search_device_pair": 1.5, "rerank": 1.5,
           "range_results_again": 2.0, "filter_count": 1.5, "reset": 0.5, "set_centroids": 0.7, "flat_add": 0.7, "become_lsh": 0.5}


def _draw_args(rng, kind, op, m, nq_choices):
    def batch():
        return int(rng.choice(nq_choices)), int(rng.choice(KS)), int(rng.integers(2))
    if op in ("search", "search_device_pair", "search_filtered", "flat_search"):
        return batch()
    if op in RANGE_SEARCHES:
        nq, _, qset = batch()
        return nq, str(rng.choice(RANKS)), qset
    if op == "rerank":
        nq, k, qset = batch()
        return nq, int(rng.choice((8, 40, 150))), k, qset
    if op == "reserve":
        return int(rng.choice(nq_choices)), int(rng.choice(KS))
    if op in ("add", "add_assigned", "flat_add"):
        return (int(rng.choice(ID_BASES)),)
    if op == "add_refused" and kind == "ivf":
        return (str(rng.choice(("id_base", "list"))),)
    if op == "set_filter":
        return str(rng.choice(FLAT_MASKS if kind == "flat" else IVF_MASKS)), str(rng.choice(FILTER_FORMS))
    if op == "set_filter_device":
        return (str(rng.choice(FLAT_MASKS if kind == "flat" else IVF_MASKS)),)
    if op == "set_option":
        name, values = (FLAT_OPTIONS if kind == "flat" else IVF_OPTIONS)[int(rng.integers(len(FLAT_OPTIONS if kind == "flat" else IVF_OPTIONS)))]
        return name, float(values[int(rng.integers(len(values)))])
    if op == "set_nprobe":
        return (int(rng.choice(NPROBES)),)
    return ()


def generate(shape: Shape, seed: int, steps: int, cov: Coverage):
    """`steps` steps; `cov` (updated in place) is what the sequences before this one covered: the next op class is drawn with more
    weight where the ordered pair (previous class, class) is new, and, after an op that drops state, where a probe of that op is."""
    kind = shape.kind
    rng = np.random.default_rng([83, kind == "ivf", [s.name for s in SHAPES[kind]].index(shape.name), seed, steps])
    m = model_for(shape, metric_of(shape, seed))
    out, pairs, probes = [], cov.pairs, cov.probes
    pair_done = grow_done = False
    open_droppers = {}
    epilogue = steps - 6
    feas = feasible_pairs(kind)

    def emit(op, args):
        nonlocal pair_done, grow_done, open_droppers
        s = Step(op, tuple(args))
        had_filter, had_range, top = m.mask is not None, m.range is not None, m.max_nq
        plan = m.apply(s)
        answers = plan.expect[0] != "error"
        if out:
            pairs.add((out[-1].op, op))
            p = out[-1]
            if op in BATCH_OPS and p.op in BATCH_OPS and "rerank" not in (op, p.op) and answers and out_answers[-1] \
                    and p.args[0] == s.args[0] and p.args[-1] != s.args[-1]:
                pair_done = True
        if op in BATCH_OPS and answers and had_filter and top and s.args[0] > top:
            grow_done = True
        if op in INSTALLS or op in RANGE_SEARCHES:
            open_droppers = {}
        if op in PROBES:
            Coverage.note(probes, open_droppers, op)
        if op in DROPPERS[kind]:
            open_droppers[op] = (had_filter, had_range)
        out.append(s)
        out_answers.append(answers)

    out_answers = []
    while len(out) < steps:
        i = len(out)
        if i >= epilogue and not (pair_done and grow_done):            # the obligations of every sequence, if chance has not met them
            if not m.live:
                emit("add", (0,))
                continue
            if not grow_done:
                if m.mask is None:
                    emit("set_filter", ("random-0.5", "bool"))
                    continue
                if not m.max_nq:
                    emit("search", (1, 10, 0))
                    continue
                bigger = [q for q in NQS if q > m.max_nq]               # (never empty: batches stay at 64 and below until this is met)
                emit("search_filtered", (bigger[0], 10, 0))
                continue
            if i + 2 <= steps:
                emit("search", (5, 10, 0))
                emit("search", (5, 10, 1))
                continue
        prev = out[-1].op if out else None
        allowed = [op for op in OPS[kind] if m.allowed(op)]
        if not out:
            allowed = ["add"]
        w = np.array([_WEIGHT.get(op, 1.0) for op in allowed])
        for j, op in enumerate(allowed):
            if prev is not None and (prev, op) not in pairs:
                w[j] *= 30.0
            if op in PROBES and any(op not in probes[d] and (hr if op == "range_results_again" else hf)
                                    for d, (hf, hr) in open_droppers.items()):
                w[j] *= 6.0
            w[j] *= 1.0 + sum((op, b) in feas and (op, b) not in pairs for b in OPS[kind]) * 3.0     # (classes with successors still to see)
        op = allowed[int(rng.choice(len(allowed), p=w / w.sum()))]
        # batches stay at 64 and below until one has outgrown the others under a filter
        small = [q for q in NQS if q <= 64] if not grow_done else list(NQS)
        args = list(_draw_args(rng, kind, op, m, small))
        if op in BATCH_OPS and m.live:
            if not grow_done and m.mask is not None and m.max_nq and rng.random() < 0.5:
                bigger = [q for q in NQS if q > m.max_nq]
                if bigger:
                    args[0] = bigger[0]
            elif not pair_done and prev in BATCH_OPS and "rerank" not in (op, prev) and out_answers[-1] and rng.random() < 0.5:
                args[0], args[-1] = out[-1].args[0], 1 - out[-1].args[-1]
        emit(op, args)
    return tuple(out[:steps])


@lru_cache(maxsize=None)
def _chain(kind: str, index: int, steps: int):
    """(steps of the index-th committed sequence, coverage after it)"""
    cov = _chain(kind, index - 1, steps)[1].copy() if index else Coverage.empty(kind)
    shape, seed = committed(kind)[index]
    return generate(shape, seed, steps, cov), cov


def sequence(kind: str, shape: str, seed: int, steps: int = STEPS):
    """the steps of one sequence: deterministic.  A committed (shape, seed) continues the coverage of the committed sequences before
    it; any other pair starts from no coverage."""
    order = [(s.name, sd) for s, sd in committed(kind)]
    if (shape, seed) in order:
        return _chain(kind, order.index((shape, seed)), steps)[0]
    return generate(shape_of(kind, shape), seed, steps, Coverage.empty(kind))


def replay(kind: str, shape: str, seed: int, upto: int, steps: int = STEPS):
    """exactly the prefix of `sequence` that ends with step `upto`: run it on a fresh index with a fresh model"""
    return sequence(kind, shape, seed, steps)[:upto + 1]


def pair_matrix(kind: str, pairs) -> str:
    """rows = the first op class, columns = the second (numbered); '#' seen, '.' feasible and missing, ' ' infeasible"""
    ops, feas = OPS[kind], feasible_pairs(kind)
    head = " " * 24 + "".join(f"{j % 100:>3d}" for j in range(len(ops)))
    rows = [f"{i:>2d} {a:<20s} " + "".join("  " + ("#" if (a, b) in pairs else "." if (a, b) in feas else " ") for b in ops)
            for i, a in enumerate(ops)]
    return "\n".join([head] + rows)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------
class SequenceMismatch(AssertionError):
    def __init__(self, message, step):
        super().__init__(message)
        self.step = step


def _is_fake(index):
    return isinstance(index, _Fake)


def _raw(index, status):
    from vdbhip import _ffi

    _ffi.check(status, build_time=True)


def _device_pair(index, Q, k):
    """two searches on torch's current stream into different outputs, no synchronise between them, one after"""
    if _is_fake(index):
        return index.search(Q, k), index.search(Q, k)
    import torch

    q = torch.from_numpy(np.array(Q, dtype=F32)).cuda()
    outs = [(torch.empty((len(Q), k), dtype=torch.float32, device="cuda"), torch.empty((len(Q), k), dtype=torch.int64, device="cuda"))
            for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for d, i in outs:
            index.search_device(q.data_ptr(), len(Q), k, d.data_ptr(), i.data_ptr(), stream)
    finally:
        torch.cuda.synchronize()
    return tuple((d.cpu().numpy(), i.cpu().numpy()) for d, i in outs)


def _range_device(index, Q, radius):
    if _is_fake(index):
        return index.range_search(Q, radius)
    import torch

    q = torch.from_numpy(np.array(Q, dtype=F32)).cuda()
    lims = torch.empty((len(Q) + 1,), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    total = index.range_search_device(q.data_ptr(), len(Q), radius, lims.data_ptr(), stream)
    d = torch.empty((max(total, 1),), dtype=torch.float32, device="cuda")
    i = torch.empty((max(total, 1),), dtype=torch.int64, device="cuda")
    index.range_results_device(d.data_ptr(), i.data_ptr(), stream)
    torch.cuda.synchronize()
    return lims.cpu().numpy(), d.cpu().numpy()[:total], i.cpu().numpy()[:total]


def _range_again(index, kind, total):
    """a raw vdb_range_results / vdb_ivf_range_results call into buffers of the size the model expects"""
    if _is_fake(index):
        return index.range_results()
    from vdbhip import _ffi

    D, I = np.empty((max(total, 1),), F32), np.empty((max(total, 1),), np.int64)
    call = index._lib.vdb_range_results if kind == "flat" else index._lib.vdb_ivf_range_results
    _raw(index, call(index._handle(), _ffi.ptr(D), _ffi.ptr(I)))
    return D[:total], I[:total]


def _filter_words(index, kind, words, nbits, device=False):
    """the packed words as they are (tail bits set), through the C ABI; `device`: from device memory on torch's current stream"""
    if _is_fake(index):
        return index.set_filter(words, nbits=nbits)
    from vdbhip import _ffi

    index._filter_key = None
    lib, h = index._lib, index._handle()
    if device:
        import torch

        w = torch.from_numpy(words.view(np.int32)).cuda()
        call = lib.vdb_filter_set_device if kind == "flat" else lib.vdb_ivf_filter_set_device
        status = call(h, w.data_ptr(), int(nbits), torch.cuda.current_stream().cuda_stream or None)
        torch.cuda.synchronize()
    else:
        call = lib.vdb_filter_set if kind == "flat" else lib.vdb_ivf_filter_set
        status = call(h, _ffi.ptr(words), int(nbits))
    _raw(index, status)


def _flat_search(index, Q, k):
    """vdb_search on an IVF handle (IVFFlatIndex has no method for it)"""
    if _is_fake(index):
        return index.flat_search(Q, k)
    from vdbhip import _ffi

    Q = np.ascontiguousarray(Q, F32)
    D, I = np.empty((len(Q), k), F32), np.empty((len(Q), k), np.int64)
    _raw(index, index._lib.vdb_search(index._handle(), _ffi.ptr(Q), len(Q), k, _ffi.ptr(D), _ffi.ptr(I)))
    return D, I


def _flat_add(index, rows, id_base):
    """vdb_add on an IVF handle"""
    if _is_fake(index):
        return index.flat_add(rows, id_base)
    from vdbhip import _ffi

    rows = np.ascontiguousarray(rows, F32)
    index._filter_key = None
    _raw(index, index._lib.vdb_add(index._handle(), _ffi.ptr(rows), len(rows), int(id_base)))


def _execute(index, kind, step: Step, p: dict):
    op, a = step.op, step.args
    if op in ("add", "add_assigned", "append", "append_empty", "add_refused"):
        if kind == "ivf":
            return index.add(p["rows"], id_base=p["id_base"], list_of_row=p["lor"])
        return index.add(p["rows"], id_base=p["id_base"])
    if op == "flat_add":
        return _flat_add(index, p["rows"], p["id_base"])
    if op == "reset":
        return index.reset()
    if op == "search":
        return index.search(p["Q"], a[1])
    if op == "flat_search":
        return _flat_search(index, p["Q"], a[1])
    if op == "search_device_pair":
        first, second = _device_pair(index, p["Q"], a[1])
        return first + second
    if op == "search_filtered":
        return index.search_filtered(p["Q"], a[1])
    if op == "rerank":
        return index.rerank(p["Q"], p["cand"], a[2])
    if op == "range_search":
        return index.range_search(p["Q"], p["radius"])
    if op == "range_search_device":
        return _range_device(index, p["Q"], p["radius"])
    if op == "range_results_again":
        return _range_again(index, kind, p["total"])
    if op in ("set_filter", "set_filter_device"):
        if p["form"] in ("words", "device"):
            return _filter_words(index, kind, p["words"], p["nbits"], device=p["form"] == "device")
        return index.set_filter(p["allowed"])
    if op == "set_filter_refused":
        return _filter_words(index, kind, p["words"], p["nbits"])
    if op == "clear_filter":
        return index.clear_filter()
    if op == "filter_count":
        return index.filter_count
    if op == "reserve":
        return index.reserve(a[0], a[1])
    if op == "set_option":
        return index.set_option(a[0], a[1])
    if op == "set_nprobe":
        return index.set_nprobe(a[0])
    if op == "set_centroids":
        return index.set_centroids(p["C"])
    if op == "become_lsh":
        return index.lsh_set_projection(np.random.default_rng(p["seed"]).standard_normal((p["nbits"], index.dim)).astype(F32))
    raise ValueError(f"unknown op {op}")


def _compare(got, expect):
    """None, or what differs"""
    tag = expect[0]
    if tag == "none":
        return None
    if tag == "value":
        return None if got == expect[1] else f"returned {got!r}, expected {expect[1]!r}"
    want = expect[1]
    if tag == "arrays":
        if len(want) * 2 == len(got):           # (a device pair: both results against the one expectation)
            want = tuple(want) * 2
        if not isinstance(got, tuple) or len(got) != len(want):
            return f"returned {type(got).__name__} of {len(got) if isinstance(got, tuple) else '-'} arrays, expected {len(want)}"
        for j, (g, w) in enumerate(zip(got, want)):
            if g.dtype != w.dtype or g.shape != w.shape:
                return f"array {j}: {g.dtype} {g.shape}, expected {w.dtype} {w.shape}"
            if g.tobytes() != w.tobytes():
                bad = np.flatnonzero(g.reshape(-1).view(np.uint8 if g.itemsize == 1 else f"u{g.itemsize}")
                                     != w.reshape(-1).view(np.uint8 if w.itemsize == 1 else f"u{w.itemsize}"))[:5]
                return (f"array {j} differs at flat positions {bad.tolist()}: got {g.reshape(-1)[bad].tolist()}, "
                        f"expected {w.reshape(-1)[bad].tolist()}")
        return None
    raise ValueError(tag)


def run(index, steps, model, log=None, label="", first=0):
    """Execute step by step against the model.  Every returned array is compared in dtype, shape and bytes, every expected refusal in
    class and message fragment, and vdb_stats.ntotal after every step.  A mismatch raises SequenceMismatch with `label` (kind, shape,
    seed), the step number, the trace up to that step and the first differing positions.  `log`: a list that receives
    (step number, line, seconds) per step.  With VDBHIP_SEQUENCE_TRACE naming a file, each step's line is appended to it and flushed
    before the step runs.  `first`: the number of steps[0], for a caller that runs one sequence in several pieces."""
    import time

    kind = model.shape.kind
    path = os.environ.get("VDBHIP_SEQUENCE_TRACE")
    trace_file = open(path, "a") if path else None
    trace = []
    try:
        for i, step in enumerate(steps, first):
            line = f"{label} step {i}: {step.line()}"
            trace.append(line)
            if trace_file:
                trace_file.write(line + "\n")
                trace_file.flush()
            plan = model.apply(step)
            t0 = time.perf_counter()
            problem, got = None, None
            try:
                got = _execute(index, kind, step, plan.inputs)
                if plan.expect[0] == "error":
                    problem = f"answered {type(got).__name__} where {plan.expect[1]} error '{plan.expect[2]}' was expected"
            except (RuntimeError, ValueError) as e:
                if plan.expect[0] != "error":
                    problem = f"raised {type(e).__name__}: {e}"
                else:
                    cls = ValueError if plan.expect[1] == "invalid" else RuntimeError
                    if not isinstance(e, cls) or plan.expect[2] not in str(e):
                        problem = f"raised {type(e).__name__}: {e}; expected {cls.__name__} naming '{plan.expect[2]}'"
            if problem is None and plan.expect[0] != "error":
                problem = _compare(got, plan.expect)
            if problem is None:
                ntotal = int(index.stats()["ntotal"])
                if ntotal != model.stat_n:
                    problem = f"stats ntotal = {ntotal}, the model holds {model.stat_n}"
            if log is not None:
                log.append((i, step.line(), time.perf_counter() - t0))
            if problem is not None:
                raise SequenceMismatch(f"{label}: step {i} {step.line()}: {problem}\n" + "\n".join(trace), i)
    finally:
        if trace_file:
            trace_file.close()


def open_index(vdb, shape: Shape, metric: str):
    """a fresh handle in the state every sequence starts from"""
    if shape.kind == "flat":
        index = vdb.FlatIndex(shape.d, metric, 0)
        try:
            index.set_option("force_path", shape.force)
        except Exception:
            index.close()
            raise
        return index
    index = vdb.IVFFlatIndex(shape.d, shape.nlist, metric, 0)
    try:
        index.set_centroids(data(shape)[2][0])
    except Exception:
        index.close()
        raise
    return index


# ---- the fakes ----------------------------------------------------------------------------------------------------------------------------
FAULTS = {
    "filter-kept-across-append": ("flat", "ivf"),
    "filter-kept-across-set-option": ("flat", "ivf"),
    "filter-kept-across-kind-change": ("flat", "ivf"),        # become_lsh / set_centroids (IVF: no call looks at a filter before the rows
                                                              # are filed again, so the fake keeps it across that add as well)
    "range-kept-across-append": ("flat", "ivf"),
    "range-dropped-by-search": ("flat", "ivf"),
    "range-results-previous-but-one": ("flat", "ivf"),
    "stats-reused-at-equal-batch-size": ("flat", "ivf"),
    "unfiltered-without-filter": ("flat", "ivf"),
    "nprobe-drops-filter": ("ivf",),
    "refused-add-changes-ntotal": ("flat", "ivf"),
}


def np_keys(X, Q, metric):
    """float64 keys (nq, n): d ascending, one step each (filter_cases.brute_reference's chain, all queries at once)"""
    X64, Q64 = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    acc = np.zeros((len(Q64), len(X64)))
    for d in range(X64.shape[1]):
        if metric == "l2":
            t = X64[None, :, d] - Q64[:, d, None]
            acc = t * t + acc
        else:
            acc = Q64[:, d, None] * X64[None, :, d] + acc
    return acc if metric == "l2" else -acc


def _top(keys_q, rows, k, metric, id_base):
    """one query: the k rows of `rows` smallest under (key, id), padded"""
    D = np.full(k, fc.pad_value(metric), F32)
    I = np.full(k, -1, np.int64)
    order = np.lexsort((rows, keys_q[rows]))[:k]
    I[:len(order)] = rows[order] + id_base
    kd = keys_q[rows[order]]
    D[:len(order)] = (kd if metric == "l2" else -kd).astype(F32)
    return D, I


class _Fake:
    """state and refusals that both fakes share, kept by include/vdbhip.h's contract -- except for the one `fault`"""

    def __init__(self, dim, metric, fault=None):
        assert fault is None or fault in FAULTS, fault
        self.dim, self.metric, self.fault = dim, metric, fault
        self.X = np.zeros((0, dim), F32)
        self.id_base = 0
        self.mask = None
        self.range = None
        self.range_before = None
        self.last_q = None
        self.extra_ntotal = 0

    def _on(self, fault):
        return self.fault == fault

    def _drop(self, filt=True, rng=True):
        if filt:
            self.mask = None
        if rng:
            self.range = None

    def _q(self, Q):
        """the queries a search works on"""
        Q = np.ascontiguousarray(Q, F32)
        use = Q
        if self._on("stats-reused-at-equal-batch-size") and self.last_q is not None and len(self.last_q) == len(Q):
            use = self.last_q
        self.last_q = Q
        return use

    def _install(self, allowed, nbits, ntotal):
        if nbits is not None:
            if nbits != ntotal:
                raise ValueError(f"a filter has one bit per row: nbits must equal ntotal = {ntotal}, got {nbits}")
            w = np.asarray(allowed, np.uint32)
            mask = ((w[np.arange(ntotal) // 32] >> (np.arange(ntotal) % 32).astype(np.uint32)) & 1).astype(np.bool_)
        else:
            a = np.asarray(allowed)
            if a.dtype == np.bool_:
                if a.shape != (ntotal,):
                    raise ValueError(f"expected a bool mask of length ntotal = {ntotal}")
                mask = a.copy()
            else:
                mask = np.zeros(ntotal, np.bool_)
                mask[a.astype(np.int64) - self.id_base] = True
        self.mask = mask

    def _keep_range(self, result):
        self.range_before, self.range = self.range, result
        return result

    def range_results(self):
        if self.range is None:
            raise RuntimeError("vdb_range_results: " + NO_RANGE + " on this handle")
        out = self.range
        if self._on("range-results-previous-but-one") and self.range_before is not None:
            out = self.range_before
        return out[1], out[2]

    def clear_filter(self):
        self.mask = None

    def set_option(self, name, value):
        self._drop(filt=not self._on("filter-kept-across-set-option"))

    def reserve(self, nq, k=10):
        pass

    def close(self):
        pass


class FakeFlatIndex(_Fake):
    def __init__(self, dim, metric="l2", fault=None):
        super().__init__(dim, metric, fault)
        self.lsh = False

    def stats(self):
        return {"ntotal": len(self.X) + self.extra_ntotal}

    def add(self, vectors, id_base=0):
        x = np.ascontiguousarray(vectors, F32)
        if len(self.X) and id_base != self.id_base:
            if self._on("refused-add-changes-ntotal"):
                self.extra_ntotal += len(x)
            raise ValueError(f"add appends to the rows of this index, whose id base is {self.id_base}")
        appended = len(self.X) > 0 and len(x) > 0
        self._drop(filt=not (appended and self._on("filter-kept-across-append")),
                   rng=not (appended and self._on("range-kept-across-append")))
        self.X = np.concatenate([self.X, x]) if len(self.X) else x.copy()
        self.id_base = id_base

    def reset(self):
        self.X = np.zeros((0, self.dim), F32)
        self.extra_ntotal = 0
        self._drop()

    def lsh_set_projection(self, projection):
        if not self.lsh:
            self._drop(filt=not self._on("filter-kept-across-kind-change"), rng=False)
        self.lsh = True

    def _built(self):
        if len(self.X) == 0:
            raise RuntimeError("Index has " + NOT_BUILT + " yet.")

    def _knn(self, Q, k, rows):
        keys = np_keys(self.X, Q, self.metric)
        out = [_top(keys[q], rows, k, self.metric, self.id_base) for q in range(len(Q))]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def search(self, Q, k):
        self._built()
        if self._on("range-dropped-by-search"):
            self.range = None
        return self._knn(self._q(Q), k, np.arange(len(self.X)))

    def set_filter(self, allowed, nbits=None):
        self._built()
        self._install(allowed, nbits, len(self.X))

    @property
    def filter_count(self):
        if self.mask is None:
            raise RuntimeError("vdb_filter_count: " + NO_FILTER + " on this handle")
        return int(self.mask.sum())

    def search_filtered(self, Q, k):
        self._built()
        if self.mask is None:
            if self._on("unfiltered-without-filter"):
                return self._knn(self._q(Q), k, np.arange(len(self.X)))
            raise RuntimeError("vdb_search_filtered: " + NO_FILTER + " on this handle")
        rows = np.flatnonzero(self.mask[:len(self.X)])           # (a filter kept across an append has fewer bits than rows)
        return self._knn(self._q(Q), k, rows)

    def rerank(self, Q, cand, k):
        self._built()
        Q = np.ascontiguousarray(Q, F32)
        keys = np_keys(self.X, Q, self.metric)
        out = []
        for q in range(len(Q)):
            rows = cand[q][cand[q] >= 0] - self.id_base
            out.append(_top(keys[q], rows, k, self.metric, self.id_base))
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def range_search(self, Q, radius):
        self._built()
        return self._keep_range(rc.expected(np_keys(self.X, self._q(Q), self.metric), radius, self.metric, self.id_base))


class FakeIVFFlatIndex(_Fake):
    def __init__(self, dim, nlist, metric="l2", fault=None):
        super().__init__(dim, metric, fault)
        self.nlist, self.nprobe = nlist, 1
        self.C = None
        self.lor = np.zeros(0, np.int32)
        self.built = False
        self.lingering = 0              # rows a set_centroids left in memory
        self.flat = None                # (rows, id_base) of a vdb_add
        self.stale = None

    def stats(self):
        n = len(self.flat[0]) if self.flat is not None else (len(self.X) if self.built else self.lingering)
        return {"ntotal": n + self.extra_ntotal}

    def set_centroids(self, C):
        self.C = np.ascontiguousarray(C, F32)
        if self.built:
            self.lingering = len(self.X)
        self.built = False
        self.stale = self.mask if self._on("filter-kept-across-kind-change") else None
        self._drop()

    def set_nprobe(self, nprobe):
        self.nprobe = nprobe
        if self._on("nprobe-drops-filter"):
            self.mask = None

    def assignment(self):
        return self.lor.copy()

    def add(self, x, id_base=0, list_of_row=None):
        x = np.ascontiguousarray(x, F32)
        append = self.built and len(self.X) > 0
        refusal = None
        if append and id_base != self.id_base:
            refusal = f"add appends to the rows of this index, whose id base is {self.id_base}"
        elif list_of_row is not None and len(x) and (np.min(list_of_row) < 0 or np.max(list_of_row) >= self.nlist):
            refusal = "row could not be assigned to a list"
        if refusal:
            if self._on("refused-add-changes-ntotal"):
                self.extra_ntotal += len(x)
            raise ValueError(refusal)
        grew = append and len(x) > 0
        self._drop(filt=not (grew and self._on("filter-kept-across-append")), rng=not (grew and self._on("range-kept-across-append")))
        if append and len(x) == 0:
            return
        lor = ic.host_assign(self.C, x, self.metric) if list_of_row is None else np.asarray(list_of_row, np.int32)
        if append:
            self.X, self.lor = np.concatenate([self.X, x]), np.concatenate([self.lor, lor])
        else:
            self.X, self.lor = x.copy(), lor.astype(np.int32)
        self.id_base, self.built, self.flat, self.lingering = id_base, True, None, 0
        if not append and self.stale is not None:
            self.mask, self.stale = self.stale, None

    def flat_add(self, rows, id_base):
        self.flat = (np.ascontiguousarray(rows, F32).copy(), id_base)
        self.built = False
        self.X, self.lor = np.zeros((0, self.dim), F32), np.zeros(0, np.int32)
        self._drop()

    def flat_search(self, Q, k):
        if self.flat is None:
            raise RuntimeError("Index has " + NOT_BUILT + " yet.")
        X, base = self.flat
        keys = np_keys(X, np.ascontiguousarray(Q, F32), self.metric)
        out = [_top(keys[q], np.arange(len(X)), k, self.metric, base) for q in range(len(Q))]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def reset(self):
        self.X, self.lor = np.zeros((0, self.dim), F32), np.zeros(0, np.int32)
        self.built, self.flat, self.lingering, self.extra_ntotal = False, None, 0, 0
        self._drop()

    def _built(self):
        if not self.built or len(self.X) == 0:
            raise RuntimeError("Index has " + NOT_BUILT + " yet.")

    def _probed(self, Q, mask):
        """per query: (float64 keys of every row, the admitted rows of its probed lists in (list, id) order)"""
        keys = np_keys(self.X, Q, self.metric)
        perm, offsets = ic.list_order(self.lor) if len(self.lor) else (np.zeros(0, np.int64), np.zeros(1, np.int64))
        for q in range(len(Q)):
            lists = np.sort(ic.nearest_lists(self.C, Q[q], self.metric, self.nprobe))
            lists = lists[lists + 1 < len(offsets)]
            rows = np.concatenate([perm[offsets[l]:offsets[l + 1]] for l in lists] + [np.zeros(0, np.int64)]).astype(np.int64)
            yield keys[q], rows[mask[rows]]

    def _knn(self, Q, k, mask):
        out = [_top(keys, rows, k, self.metric, self.id_base) for keys, rows in self._probed(Q, mask)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def search(self, Q, k):
        self._built()
        if self._on("range-dropped-by-search"):
            self.range = None
        return self._knn(self._q(Q), k, np.ones(len(self.X), np.bool_))

    def set_filter(self, allowed, nbits=None):
        self._built()
        self._install(allowed, nbits, len(self.X))

    @property
    def filter_count(self):
        self._built()
        if self.mask is None:
            raise RuntimeError("vdb_ivf_filter_count: " + NO_FILTER + " on this handle")
        return int(self.mask.sum())

    def search_filtered(self, Q, k):
        self._built()
        if self.mask is None:
            if self._on("unfiltered-without-filter"):
                return self._knn(self._q(Q), k, np.ones(len(self.X), np.bool_))
            raise RuntimeError("vdb_ivf_search_filtered: " + NO_FILTER + " on this handle")
        mask = np.zeros(len(self.X), np.bool_)
        m = min(len(mask), len(self.mask))
        mask[:m] = self.mask[:m]
        return self._knn(self._q(Q), k, mask)

    def range_search(self, Q, radius):
        self._built()
        lims, D, I = [0], [], []
        r = F32(radius)
        for keys, rows in self._probed(self._q(Q), np.ones(len(self.X), np.bool_)):
            with np.errstate(over="ignore", invalid="ignore"):
                d = (keys[rows] if self.metric == "l2" else -keys[rows]).astype(F32)
                hit = d < r if self.metric == "l2" else d > r
            D.append(d[hit])
            I.append(rows[hit] + self.id_base)
            lims.append(lims[-1] + int(hit.sum()))
        return self._keep_range((np.asarray(lims, np.int64), np.concatenate(D).astype(F32), np.concatenate(I).astype(np.int64)))

    def range_results(self):
        self._built()
        return super().range_results()


def open_fake(shape: Shape, metric: str, fault: Optional[str] = None):
    if shape.kind == "flat":
        return FakeFlatIndex(shape.d, metric, fault)
    index = FakeIVFFlatIndex(shape.d, shape.nlist, metric, fault)
    index.set_centroids(data(shape)[2][0])
    return index


def fault_trigger(fault: str, shape: Shape, metric: str, steps) -> Optional[int]:
    """the first step at which the planted fault can change what the handle does (its effect shows at that step or later); None: never"""
    answers, installed, ranged = dry_run(shape, metric, steps)
    kind = shape.kind
    nranges = 0
    for i, s in enumerate(steps):
        nranges += s.op in RANGE_SEARCHES and answers[i]
        hit = {
            "filter-kept-across-append": s.op == "append" and installed[i],
            "filter-kept-across-set-option": s.op == "set_option" and installed[i],
            "filter-kept-across-kind-change": s.op == ("become_lsh" if kind == "flat" else "set_centroids") and installed[i],
            "range-kept-across-append": s.op == "append" and ranged[i],
            "range-dropped-by-search": s.op == "search" and ranged[i] and answers[i],
            "range-results-previous-but-one": nranges >= 2,
            "stats-reused-at-equal-batch-size": i > 0 and s.op in BATCH_OPS and steps[i - 1].op in BATCH_OPS and answers[i] and answers[i - 1]
                                                and s.args[0] == steps[i - 1].args[0] and s.args[-1] != steps[i - 1].args[-1],
            "unfiltered-without-filter": s.op == "search_filtered" and not installed[i],
            "nprobe-drops-filter": s.op == "set_nprobe" and installed[i],
            "refused-add-changes-ntotal": s.op == "add_refused",
        }[fault]
        if hit:
            return i
    return None

"""Hostile values on every search path: ids and distances equal the CPU oracle's, bit for bit, whatever the input holds.

The cases are those of tests/hostile_cases.py, built at the smallest size at which each kernel family is still chosen (the
thresholds are those of search_batch / build_derived in csrc and of csrc/scan_plan.hpp; every test checks the path it meant to
take with stats()).  One index per (path, corpus, metric) serves all the query batches of its corpus.  Every comparison is
np.testing.assert_array_equal against oracle/knn_oracle.c (restricted to the probed lists by oracle.ivf_search on IVF indexes,
over the reconstructed rows of tests/*_restatement.py on the coded kinds); nothing is compared with the code under test and no
tolerance appears.  (assert_array_equal counts two NaNs as equal: the distances of a NaN query are NaN on both sides, their
payload is not compared.)

Path assertions, from the labels of hostile_cases.batch_label (tests/test_hostile_host.py derives them): a "must" batch -- scales
unusable, or a non-finite query in it -- reports last_fallback_queries == nq on the scan paths and every finite query of it
still returns the oracle's bits; a non-finite corpus ("exact") is never served by "mfma_scan"; a "may" batch is served by
"mfma_scan", and the number of its queries that fell back on their own is recorded in FALLBACKS, not asserted."""
from __future__ import annotations

import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Tuple

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from tests import hostile_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu

FALLBACKS: Dict[str, int] = {}          # "may" searches: queries that took the exhaustive pass on their own (recorded, not asserted)
_ORACLE: Dict[tuple, tuple] = {}        # the oracle's answers, computed once and shared by the paths that search the same inputs
_FLAT_FAMILIES = [f for f in hc.FAMILIES if f != "bytes"]


@dataclass(frozen=True)
class Path_:
    id: str
    d: int
    n: int
    opts: Tuple[Tuple[str, float], ...] = ()
    nq: int = hc.NQ            # queries per search: the batch as it is (8 or 1), its first query (1), or tiled to 64 (dense paths)
    name: str = "mfma_scan"    # last_path_name of a finite corpus
    shape: int = 16            # scan_shape of a finite corpus
    devices: object = 0
    families: Tuple[str, ...] = tuple(_FLAT_FAMILIES)


FLAT_PATHS = [
    # dense small-corpus path: Npad <= 15 360 rows, >= 64 queries, too few pairs for the scan
    Path_("dense", 16, 3000, (), nq=64, shape=32),
    # layout x16 needs Npad > kDenseMaxRows = 15 360; below 32 768 rows a batch of 8 takes the scan only when forced
    Path_("x16", 16, 15872, (("force_path", 2),)),
    Path_("x16-nq1", 16, 15872, (("force_path", 2),), nq=1),
    Path_("x16-unfused-stats", 16, 15872, (("fused_stats", 0), ("force_path", 2))),
    Path_("32x32", 16, 15872, (("flat_shape", 32), ("force_path", 2)), shape=32),
    # D > 128: p16 panels and the K-loop scan above 2048 rows (its standard geometry wants 4 k superbins of 256 rows: ten
    # 1024-row spans at k = 10; at 2100 rows search_batch takes the exhaustive kernels, force_path or not), the dense path's
    # K-loop scores + register select below
    Path_("kloop", 136, 9300, (("force_path", 2),), shape=0),
    Path_("kloop-streamed", 136, 9300, (("stream_panels", 1), ("force_path", 2)), shape=0),
    Path_("dense-register-select", 136, 600, (), nq=64, shape=0),
    Path_("exhaustive-blocked", 16, 3000, (("force_path", 1),), name="exact_scan", shape=32),
    Path_("exhaustive-per-wave", 16, 3000, (("force_path", 3),), name="exact_scan", shape=32),
    Path_("list-cap-1", 16, 15872, (("force_path", 2), ("list_cap", 1))),
    Path_("two-shards", 16, 31744, (("multi_stage_all", 1), ("force_path", 2)), devices=(0, 0)),
    Path_("int8-x16", 16, 15872, (("force_path", 2),), families=("bytes",)),
    Path_("int8-32x32", 16, 15872, (("flat_shape", 32), ("force_path", 2)), shape=32, families=("bytes",)),
    Path_("int8-exhaustive", 16, 3000, (("force_path", 1),), name="exact_scan", shape=32, families=("bytes",)),
]
_POST = {"force_path", "list_cap", "fused_stats"}        # options of the search; the others shape the scan copies: set before add


def _flat_params():
    return [pytest.param(p, f, id=f"{p.id}-{f}") for p in FLAT_PATHS for f in p.families]


def _queries(Q, nq):
    if nq == 1:
        return np.ascontiguousarray(Q[:1])
    if nq == 64:
        return np.ascontiguousarray(np.tile(Q, (64 // len(Q), 1)))
    return Q


def _want(oracle, corpus, n, batch, Q, metric, k, make=None):
    key = (corpus.name, n, corpus.X.shape[1], batch.name, len(Q), metric, k, make is not None and make[0])
    if key not in _ORACLE:
        _ORACLE[key] = make[1]() if make else oracle.knn(corpus.X, Q, k, metric)
    return _ORACLE[key]


def _equal(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"ids of {what}")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"distances of {what}")


class _Findings:
    """every search of a test is checked, then the test fails with all of its findings (one GPU run shows every failing cell)"""

    def __init__(self):
        self.lines = []

    def check(self, what, fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            self.lines.append(f"{what}: " + " ".join(str(e).split())[:400])

    def done(self):
        assert not self.lines, f"{len(self.lines)} findings:\n" + "\n".join(self.lines[:60])


def _shard_labels(X, Q, metric, shards):
    """the label of every shard of a multi-device index (contiguous blocks of ceil(n / shards) rows, each with scales of its own)"""
    per = -(-len(X) // shards)
    cs = [hc.corpus_scales(X[s * per:(s + 1) * per]) for s in range(shards)]
    return [hc.batch_label(c, Q, metric) for c in cs], cs


def _check_path(p, st, labels, cs, Q, metric, what):
    if all(lb == "exact" for lb in labels):                     # non-finite corpus: no scan copy exists
        assert st["last_path_name"] != "mfma_scan" and st["scan_shape"] == 0 and st["has_i8_copy"] == 0, (what, st)
        return
    if labels[0] == "exact":           # (the statistics name the first shard's path: here the exhaustive one, of a non-finite shard)
        return
    assert st["last_path_name"] == p.name and st["scan_shape"] == p.shape, (what, st)
    if p.name != "mfma_scan" or None in labels:
        return
    must = len(Q) * labels.count("must")
    if "may" not in labels:
        assert st["last_fallback_queries"] == must, (what, st)
        return
    FALLBACKS[what] = int(st["last_fallback_queries"]) - must
    assert st["last_fallback_queries"] >= must, (what, st)
    if cs[0]["byte"] and len(labels) == 1:
        assert st["has_i8_copy"] == 1 and st["scan_dtype"] == int(hc.batch_scales(cs[0], Q, metric)["i8"]), (what, st)


def _flat_index(vdb, p, X, metric, devices=None, id_base=0):
    idx = vdb.FlatIndex(X.shape[1], metric, list(p.devices) if isinstance(p.devices, tuple) else p.devices)
    try:
        for name, value in p.opts:
            if name not in _POST:
                idx.set_option(name, value)
        idx.add(X, id_base=id_base)
        for name, value in p.opts:
            if name in _POST:
                idx.set_option(name, value)
    except Exception:
        idx.close()
        raise
    return idx


@pytest.mark.parametrize("p,family", _flat_params())
def test_flat_search_equals_the_oracle(p, family, vdb, oracle):
    shards = len(p.devices) if isinstance(p.devices, tuple) else 1
    f = _Findings()
    for g in hc.groups(family, p.n, p.d):
        for metric in g.metrics:
            idx = _flat_index(vdb, p, g.corpus.X, metric)
            try:
                for b in g.batches:
                    Q = _queries(b.Q, p.nq)
                    labels, scs = _shard_labels(g.corpus.X, Q, metric, shards)
                    for k in g.ks:
                        what = f"{p.id}/{g.corpus.name}/{b.name}/{metric}/k{k}"
                        got = idx.search(Q, k)
                        st = idx.stats()
                        f.check(what, _equal, got, _want(oracle, g.corpus, p.n, b, Q, metric, k), what)
                        f.check(what, _check_path, p, st, labels, scs, Q, metric, what)
            finally:
                idx.close()
    f.done()


# ---- small corpora: k inside, at and past the finite rows, k = n and k > n ---------------------------------------------------------
SMALL_N = 40


@pytest.mark.parametrize("family", ["inf-rows", "nan-rows", "subnormal"])
@pytest.mark.parametrize("how", ["search", "forced-exhaustive", "two-shards", "rerank", "lsh", "knng"])
def test_small_corpus_every_k(how, family, vdb, oracle):
    """inf-keyed rows come back after every finite key, by id, with D = +-inf and real ids, ahead of the -1 / +-FLT_MAX padding
    (k = n: no padding at all) -- from the exhaustive kernels, the merge of a two-shard index, vdb_rerank over all ids,
    vdb_lsh_search with every row a candidate and vdb_knng_search over an injected complete graph with ef > n, whose float64
    scoring kernels are separate code."""
    n, d = SMALL_N, hc.D
    for g in hc.groups(family, n, d):
        X = g.corpus.X
        for metric in g.metrics:
            if how == "knng":
                idx = vdb.KnnGraphIndex(d, metric, 0)
            else:
                idx = vdb.FlatIndex(d, metric, [0, 0] if how == "two-shards" else 0)
            try:
                if how == "two-shards":
                    idx.set_option("multi_stage_all", 1)
                if how == "lsh":
                    idx.lsh_set_projection(vdb.make_projection(d, 64, 0))
                idx.add(X)
                if how == "forced-exhaustive":
                    idx.set_option("force_path", 3)
                if how == "knng":
                    nb = np.array([[j for j in range(n) if j != i] for i in range(n)], np.int32)
                    idx.knng_set(nb)
                (b,) = g.batches
                for k in g.ks:
                    what = f"{how}/{g.corpus.name}/{metric}/k{k}"
                    want = _want(oracle, g.corpus, n, b, b.Q, metric, k)
                    if how == "rerank":
                        cand = np.tile(np.r_[np.arange(n), [-1, -1, -1]].astype(np.int64), (len(b.Q), 1))
                        got = idx.rerank(b.Q, cand, k)
                    elif how == "lsh":
                        got = idx.lsh_search(b.Q, k, n)
                    elif how == "knng":
                        got = idx.knng_search(b.Q, k, 64)
                    else:
                        got = idx.search(b.Q, k)
                        assert idx.stats()["last_path_name"] == "exact_scan", what
                    _equal(got, want, what)
            finally:
                idx.close()


# ---- partial lists of three handles, merged on the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,family", [(n, f) for n in (SMALL_N, 3000) for f in ("inf-rows", "nan-rows", "subnormal", "inf-query", "nan-query")] +
                         [(3000, "ladder")])
def test_partial_lists_of_three_handles_merge_to_the_oracle(n, family, vdb, oracle):
    """search_partial_device on three handles (rows split 3 ways, global ids) + merge_packed_partials_device: float64 keys travel
    between the two, so an inf key meets the +inf padding key of a short shard in the merge"""
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    bounds = [0, n // 3, (2 * n) // 3 + 1, n]
    for g in hc.groups(family, n, hc.D):
        if family == "ladder" and g.corpus.expect["step"] not in (-44, -30, 0, 20, 38):
            continue
        for metric in g.metrics:
            shards = [vdb.FlatIndex(hc.D, metric, 0) for _ in range(3)]
            try:
                for s, lo, hi in zip(shards, bounds[:-1], bounds[1:]):
                    s.add(g.corpus.X[lo:hi], id_base=lo)
                for b in g.batches:
                    nq = len(b.Q)
                    q_t = torch.from_numpy(b.Q.copy()).cuda()
                    for k in g.ks:
                        packed = torch.empty((3, 2, nq, k), dtype=torch.int64, device="cuda")
                        for p, s in enumerate(shards):
                            s.search_partial_device(q_t.data_ptr(), nq, k, packed[p, 0].data_ptr(), packed[p, 1].data_ptr(), stream)
                        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                        vdb.merge_packed_partials_device(metric, 0, packed.data_ptr(), 3, nq, k, D.data_ptr(), I.data_ptr(), stream)
                        torch.cuda.synchronize()
                        _equal((D.cpu().numpy(), I.cpu().numpy()), _want(oracle, g.corpus, n, b, b.Q, metric, k),
                               f"partial/{g.corpus.name}/{b.name}/{metric}/k{k}")
            finally:
                for s in shards:
                    s.close()


# ---- IVF-Flat -------------------------------------------------------------------------------------------------------------------------------
IVF_N, NLIST = 6000, 16


@dataclass(frozen=True)
class IvfPath:
    id: str
    d: int
    opts: Tuple[Tuple[str, float], ...] = ()
    families: Tuple[str, ...] = tuple(_FLAT_FAMILIES)
    mfma: bool = True          # the list-major MFMA scan serves nprobe = 16 of a finite corpus


IVF_PATHS = [
    IvfPath("list-mfma", 16),
    IvfPath("list-kloop", 136),
    IvfPath("list-exact", 16, (("force_path", 1),), mfma=False),
    IvfPath("list-int8", 16, families=("bytes",)),
]


def _check_ivf_path(p, st, label, nprobe, what, cs, Q, metric):
    assert st["last_path_name"] == "ivf", (what, st)
    if label == "exact":
        assert st["last_rows_scanned"] == 0 and st["last_fallback_queries"] == 0, (what, st)
    if not (p.mfma and nprobe == 16):
        return
    if label == "must":
        assert st["last_fallback_queries"] == len(Q), (what, st)
    if label == "may":
        FALLBACKS[what] = int(st["last_fallback_queries"])
        assert st["last_rows_scanned"] > 0, (what, st)          # the list-major MFMA scan ran
        if cs["byte"]:
            assert st["scan_dtype"] == int(hc.batch_scales(cs, Q, metric)["i8"]), (what, st)


@pytest.mark.parametrize("p,family", [pytest.param(p, f, id=f"{p.id}-{f}") for p in IVF_PATHS for f in p.families])
def test_ivf_flat_search_equals_the_oracle(p, family, vdb, oracle):
    """Centroids = the first 16 rows, so the coarse quantizer sees the same hostile magnitudes (inf-rows: once with an inf in a
    centroid).  The assignment must be the oracle's nearest centroid; a search must equal brute force over the probed lists."""
    gs = hc.groups(family, IVF_N, p.d)
    if family == "inf-rows":
        gs = gs + hc.groups(family, IVF_N, p.d, 6)[:1]
    if family == "ladder" and p.id != "list-mfma":           # thinned interior, every labelled edge kept
        gs = tuple(g for g in gs if g.corpus.expect["step"] in (-44, -36, -30, 0, 10, 20, 38))
    f = _Findings()
    for g in gs:
        X = g.corpus.X
        C = np.ascontiguousarray(X[:NLIST])
        cs = hc.corpus_scales(X)
        for metric in g.metrics:
            idx = vdb.IVFFlatIndex(p.d, NLIST, metric, 0)
            try:
                idx.set_centroids(C)
                idx.add(X)
                for name, value in p.opts:
                    idx.set_option(name, value)
                lor = idx.assignment()
                tag = (g.corpus.name, IVF_N, p.d, metric)
                if ("assign",) + tag not in _ORACLE:
                    _ORACLE[("assign",) + tag] = oracle.ivf_assign(C, X, metric)
                f.check(f"assignment of {tag}", np.testing.assert_array_equal, lor, _ORACLE[("assign",) + tag])
                for nprobe in (1, 4, 16):
                    idx.set_nprobe(nprobe)
                    for b in g.batches:
                        what = f"ivf-{p.id}/{g.corpus.name}/{b.name}/{metric}/nprobe{nprobe}"
                        got = idx.search(b.Q, hc.K)
                        st = idx.stats()
                        want = _want(oracle, g.corpus, IVF_N, b, b.Q, metric, hc.K,
                                     (f"ivf{nprobe}", lambda: oracle.ivf_search(X, C, lor, b.Q, hc.K, nprobe, metric)))
                        f.check(what, _equal, got, want, what)
                        f.check(what, _check_ivf_path, p, st, hc.batch_label(cs, b.Q, metric), nprobe, what, cs, b.Q, metric)
            finally:
                idx.close()
    f.done()


@pytest.mark.parametrize("step", [0, -20])
def test_row_norms_are_float64_sums_rounded_once(step, vdb):
    """corpus_stats_kernel: ||x||^2 is a float64 sum rounded ONCE to float32.  No search can tell a float32 accumulation from it
    ("Hostile values"), so the norm is read back through the scan's own scores: against an all-zero query (sq = 1, no
    dot product) the raw score of row i is bias[i] * cs with cs = sx, a power of two, so the product is exact.  At step -20 the
    squares are float32 subnormals, where an accumulation in float32 is off by up to 1e-5 of the norm."""
    X = hc.ladder_corpus(step, 3000, hc.D).X
    x64 = X.astype(np.float64)
    norm = np.zeros(len(X))
    for c in range(hc.D):                                   # the kernel's chain: fma over the dimensions in order
        norm = x64[:, c] * x64[:, c] + norm                 # (every product is exact in float64; one rounding per step, as fma's)
    want = norm.astype(np.float32)
    acc32 = np.zeros(len(X), np.float32)
    with np.errstate(under="ignore"):
        for c in range(hc.D):
            acc32 = (acc32 + X[:, c] * X[:, c]).astype(np.float32)
    assert (acc32 != want).mean() > 0.2, "the corpus does not tell the two roundings apart"
    idx = vdb.FlatIndex(hc.D, "l2", 0)
    try:
        idx.add(X)
        scores, _, cs = idx.debug_scan_scores(np.zeros((1, hc.D), np.float32), 0, len(X))
    finally:
        idx.close()
    assert cs == float(hc.corpus_scales(X)["sx"]) and np.frexp(cs)[0] == 0.5
    np.testing.assert_array_equal(scores[0], want * np.float32(cs))


def test_zz_report_recorded_fallbacks():
    """not a check: the fallback counts of the "may" searches, for the record (pytest -s shows them)"""
    own = {k: v for k, v in FALLBACKS.items() if v}
    print(f"\n{len(FALLBACKS)} 'may' searches, {len(own)} of them with queries that fell back on their own:")
    for k, v in sorted(own.items()):
        print(f"  {v:3d}  {k}")


# ---- the coded kinds: PQ, IVF-SQ8, IVF-PQ --------------------------------------------------------------------------------------------
# Injected codebooks / centroids / ranges (finite: the library refuses others), unit scale and scaled by 10^+-15; the hostile
# QUERY batches of the ladder, the inf query and the NaN query against them.  The reference is oracle.knn / oracle.ivf_search over
# the reconstructed rows x^ of tests/pq_restatement.py, tests/ivfpq_restatement.py and tests.helpers.np_decode.
import pq_restatement as pq_ref  # noqa: E402
import ivfpq_restatement as ivfpq_ref  # noqa: E402

from tests.helpers import np_decode  # noqa: E402

CODED_M = 4
CODED_SCALES = [("1", 1.0), ("1e15", 1.0e15), ("1e-15", 1.0e-15)]


def _coded_batches():
    return (hc.unit_batch(hc.D),) + hc.ladder_batches(hc.D) + hc.bad_query_batches(hc.D, np.inf, "inf") + \
        hc.bad_query_batches(hc.D, np.nan, "nan")


def _codebooks(scale, tag):
    rng = np.random.default_rng([hc.SEED, 77, len(tag)])
    return np.ascontiguousarray((rng.standard_normal((CODED_M, 256, hc.D // CODED_M)) * scale).astype(np.float32))


def _search_all(f, idx, what, rows_of, oracle_fn, paths):
    """every batch under both... one metric per index: search, compare with the oracle over the reconstructed rows, record the path"""
    for b in _coded_batches():
        got = idx.search(b.Q, hc.K)
        st = idx.stats()
        paths.add(st["last_path_name"])
        f.check(f"{what}/{b.name}", _equal, got, oracle_fn(b.Q), f"{what}/{b.name}")
        if b.expect.get("bad_queries") and st["last_path_name"] in ("mfma_scan", "pq_adc", "ivfpq_adc"):
            # (the IVF-PQ lookup-table scan takes its scale from the usable queries and flags the others one by one, a query far
            #  longer than every row among them: ivfpq_adc_prep_kernel)
            adc = st["last_path_name"] == "ivfpq_adc"
            f.check(f"{what}/{b.name}", _fell_back, st, range(1, len(b.Q) + 1) if adc else [len(b.Q)])


def _fell_back(st, counts):
    assert st["last_fallback_queries"] in counts, st


@pytest.mark.parametrize("scale", CODED_SCALES, ids=[s[0] for s in CODED_SCALES])
@pytest.mark.parametrize("how", ["codes-exact", "decoded-scan", "adc"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_pq_search_equals_the_oracle_over_the_reconstructed_rows(metric, how, scale, vdb, oracle):
    n = 15872
    cb = _codebooks(scale[1], "pq")
    codes = np.random.default_rng([hc.SEED, 78]).integers(0, 256, size=(n, CODED_M)).astype(np.uint8)
    rows = pq_ref.reconstruct(codes, cb)
    idx = vdb.PQIndex(hc.D, CODED_M, metric, 0, adc_max_batch=512 if how == "adc" else 0)
    f, paths = _Findings(), set()
    try:
        idx.set_codebooks(cb)
        idx.add_codes(codes)
        if how != "codes-exact":
            idx.set_option("force_path", 2)
        _search_all(f, idx, f"pq-{how}-{scale[0]}/{metric}", rows, lambda Q: oracle.knn(rows, Q, hc.K, metric), paths)
    finally:
        idx.close()
    want = {"codes-exact": "exact_scan", "decoded-scan": "mfma_scan", "adc": "pq_adc"}[how]
    f.check("paths", lambda: _assert(want in paths or scale[0] != "1", paths))
    f.done()


def _assert(cond, msg):
    assert cond, msg


@pytest.mark.parametrize("scale", CODED_SCALES, ids=[s[0] for s in CODED_SCALES])
@pytest.mark.parametrize("kind", ["sq8", "ivfpq", "ivfpq-adc"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivf_coded_search_equals_the_oracle_over_the_reconstructed_rows(metric, kind, scale, vdb, oracle):
    n, s = IVF_N, scale[1]
    rng = np.random.default_rng([hc.SEED, 79])
    X = np.ascontiguousarray((rng.standard_normal((n, hc.D)) * s).astype(np.float32))
    C = np.ascontiguousarray(X[:NLIST])
    f, paths = _Findings(), set()
    if kind == "sq8":
        idx = vdb.IVFSQ8Index(hc.D, NLIST, metric, 0)
    else:
        idx = vdb.IVFPQIndex(hc.D, NLIST, CODED_M, metric, 0, adc_max_batch=512 if kind == "ivfpq-adc" else 0)
    try:
        idx.set_centroids(C)
        if kind == "sq8":
            idx.set_ranges(np.full(hc.D, -4.0 * s, np.float32), np.full(hc.D, 8.0 * s, np.float32))
            idx.add(X)
            lor = idx.assignment()
            vmin, vdiff = idx.ranges()
            rows = np_decode(idx.codes(), C, lor, vmin, vdiff)
        else:
            cb = _codebooks(0.5 * s, "ivfpq")
            codes = rng.integers(0, 256, size=(n, CODED_M)).astype(np.uint8)
            lor = rng.integers(0, NLIST, size=n).astype(np.int32)
            idx.set_codebooks(cb)
            idx.add_codes(codes, lor)
            rows = ivfpq_ref.decode(codes, C, lor, cb)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        for nprobe in (4, NLIST):
            idx.set_nprobe(nprobe)
            _search_all(f, idx, f"{kind}-{scale[0]}/{metric}/nprobe{nprobe}", rows,
                        lambda Q: oracle.ivf_search(rows, C, lor, Q, hc.K, nprobe, metric), paths)
    finally:
        idx.close()
    f.check("paths", lambda: _assert(("ivfpq_adc" if kind == "ivfpq-adc" else "ivf") in paths or scale[0] != "1", paths))
    f.done()


@pytest.mark.parametrize("kind", ["pq", "sq8", "ivfpq"])
def test_training_on_non_finite_rows_is_refused_and_the_handle_stays_usable(kind, vdb, oracle):
    rng = np.random.default_rng([hc.SEED, 80])
    X = rng.standard_normal((3000, hc.D)).astype(np.float32)
    for bad in (np.inf, np.nan):
        Xb = X.copy()
        Xb[1234, 7] = bad
        if kind == "pq":
            idx = vdb.PQIndex(hc.D, CODED_M, "l2", 0)
            train = idx.train
        elif kind == "sq8":
            idx = vdb.IVFSQ8Index(hc.D, NLIST, "l2", 0)
            idx.set_centroids(X[:NLIST])
            train = idx.train_ranges
        else:
            idx = vdb.IVFPQIndex(hc.D, NLIST, CODED_M, "l2", 0)
            idx.set_centroids(X[:NLIST])
            train = idx.train_codebooks
        try:
            with pytest.raises(ValueError):          # VDB_ERR_INVALID at build time
                train(Xb)
            train(X)                                  # still usable: train on finite rows, add, search
            idx.add(X)
            if kind == "pq":
                rows = pq_ref.reconstruct(idx.codes(), idx.codebooks())
                want = oracle.knn(rows, X[:8], hc.K, "l2")
            else:
                idx.set_nprobe(NLIST)
                lor = idx.assignment()
                if kind == "sq8":
                    vmin, vdiff = idx.ranges()
                    rows = np_decode(idx.codes(), X[:NLIST], lor, vmin, vdiff)
                else:
                    rows = ivfpq_ref.decode(idx.codes(), X[:NLIST], lor, idx.codebooks())
                rows = np.ascontiguousarray(rows, dtype=np.float32)
                want = oracle.ivf_search(rows, X[:NLIST], lor, X[:8], hc.K, NLIST, "l2")
            _equal(idx.search(X[:8], hc.K), want, f"{kind} after a refused training")
        finally:
            idx.close()

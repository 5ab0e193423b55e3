"""The branches of the IVF host code that no other test reaches, pinned bit for bit: both plan paths (`nlist` below and above the
LDS histogram's 8192 lists, the full pairs-per-block variant), every row of the list scans' launch tables (forced `ivf_nw`,
`ivf_bt`, `i8_ring`, `ivf_i8_group`), and the adds of the Flat and the SQ8 codec side by side.  Every search is compared with
`oracle.ivf_search` over injected centroids (the first `nlist` corpus rows) and the index's own `assignment()`; a search that
is meant to take the list-major scan says so through `last_candidates > 0`."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
F32 = np.float32


@pytest.fixture(scope="module")
def vdb():
    import vdbhip

    return vdbhip


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(F32)


def _bytes(rng, n, d):          # (as test_int8_list_scan_bit_exact)
    return np.clip(np.rint(rng.gamma(0.6, 40.0, size=(n, d))), 0, 255).astype(F32)


def _equal(got, want, msg=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)


# ---- plan paths ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[2100, 8200])
def plan_corpus(request):
    nlist = request.param
    rng = np.random.default_rng(nlist)
    return nlist, _gauss(rng, 5 * nlist, 64), _gauss(rng, 300, 64)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_plan_paths_by_nlist(vdb, oracle, plan_corpus, metric):
    """Lists of ~5 rows (one 256-row span each), 300 queries x 16 probes = 4800 pairs, k = 10: 64-row bins, 64 entries per
    query -- inside [4k, 0.7 x 4096], so the list-major scan serves the batch.  2100 lists: LDS histogram, plan and scatter in
    one dispatch, the full pairs-per-block variant (nlist > 2048).  8200 lists: no LDS histogram (> 8192), ivf_plan_kernel
    and ivf_scatter_kernel on their own; the CSR of the add is built on the host."""
    nlist, X, Q = plan_corpus
    C = X[:nlist].copy()
    idx = vdb.IVFFlatIndex(64, nlist, metric, 0)
    idx.set_centroids(C)
    idx.add(X, id_base=3)
    lor = idx.assignment()
    idx.set_nprobe(16)
    got = idx.search(Q, K)
    st = idx.stats()
    _equal(got, oracle.ivf_search(X, C, lor, Q, K, 16, metric, id_base=3))
    assert st["last_path_name"] == "ivf" and st["last_candidates"] > 0, st
    idx.close()


# ---- launch tables -------------------------------------------------------------------------------------------------------------
NPROBES = (8, 16)


SHAPES = [(64, "gauss"), (128, "gauss"), (64, "bytes"), (128, "bytes")]


def _build_tables(vdb, oracle, d, kind):
    rng = np.random.default_rng(1000 + d)
    make = _bytes if kind == "bytes" else _gauss
    X, Q = make(rng, 20_000, d), make(rng, 300, d)
    C = X[:64].copy()
    idx = vdb.IVFFlatIndex(d, 64, "l2", 0)
    idx.set_centroids(C)
    idx.add(X)
    lor = idx.assignment()
    queries = {"float": Q + 3 * _gauss(rng, 300, d)} if kind == "bytes" else {"float": Q}
    if kind == "bytes":
        queries["int"] = Q
        assert idx.stats()["has_i8_copy"] == 1
    want, default = {}, {}
    for name, q in queries.items():
        for nprobe in NPROBES:
            idx.set_nprobe(nprobe)
            want[name, nprobe] = oracle.ivf_search(X, C, lor, q, K, nprobe, "l2")
            default[name, nprobe] = idx.search(q, K)
            _equal(default[name, nprobe], want[name, nprobe], f"default {name} nprobe={nprobe}")
    return idx, queries, want, default


@pytest.fixture(scope="module")
def tables(vdb, oracle):
    """Per (d, kind), built once: 20 000 rows in 64 lists (about 1.9 spans per list), 300 queries: the index, its query sets
    ("int" only on byte-valued rows), and per (query set, nprobe) the oracle's result and the result of the default setting."""
    built = {}

    def get(d, kind):
        if (d, kind) not in built:
            built[d, kind] = _build_tables(vdb, oracle, d, kind)
        return built[d, kind]

    yield get
    for t in built.values():
        t[0].close()


def _sweep(tables, lists_serve, tag):
    idx, queries, want, default = tables
    for name, q in queries.items():
        for nprobe in NPROBES:
            idx.set_nprobe(nprobe)
            got = idx.search(q, K)
            st = idx.stats()
            msg = f"{tag} {name} nprobe={nprobe}"
            _equal(got, default[name, nprobe], msg)
            _equal(got, want[name, nprobe], msg)
            if lists_serve(nprobe):
                assert st["last_candidates"] > 0, (msg, st)
                if "int" in queries:
                    assert st["scan_dtype"] == (1 if name == "int" else 0), (msg, st)
            else:
                assert st["last_candidates"] == 0, (msg, st)


@pytest.mark.parametrize("bt", [4, 16])
@pytest.mark.parametrize("nw", [2, 4, 8])
@pytest.mark.parametrize("d,kind", SHAPES)
def test_forced_waves_and_bins(tables, d, kind, nw, bt):
    """k-steps 4 / 8 x 2 / 4 / 8 waves x 64- / 128-row bins, fp16 and (byte-valued rows, integer queries) int8 scan.
    The geometry wants 4k = 40 bins per query: 8 probes x 1.9 spans give 60 bins of 64 rows but only 30 of 128 rows, so
    `ivf_bt = 16` at nprobe 8 declines and the exact list scan answers (same bits, no candidates); 16 probes give 60 bins of
    128 rows and reach that half of both tables."""
    t = tables(d, kind)
    idx = t[0]
    idx.set_option("ivf_nw", nw)
    idx.set_option("ivf_bt", bt)
    try:
        _sweep(t, lambda nprobe: bt == 4 or nprobe == 16, f"ivf_nw={nw} ivf_bt={bt}")
    finally:
        idx.set_option("ivf_nw", 0)
        idx.set_option("ivf_bt", 0)


@pytest.mark.parametrize("ring,group", [(2, 4), (4, 4), (8, 4), (0, 8)])
@pytest.mark.parametrize("d", [64, 128])
def test_int8_staging_ring_and_octs(tables, d, ring, group):
    """`i8_ring` on a byte-valued IVF index (2 = the double buffer, 4, 8 stages) and candidate groups of 8 rows (`ivf_i8_group`),
    two and four int8 k-steps."""
    t = tables(d, "bytes")
    idx = t[0]
    idx.set_option("i8_ring", ring)
    idx.set_option("ivf_i8_group", group)
    try:
        _sweep(t, lambda nprobe: True, f"i8_ring={ring} ivf_i8_group={group}")
    finally:
        idx.set_option("i8_ring", 0)
        idx.set_option("ivf_i8_group", 4)


# ---- adds, Flat and SQ8 side by side -------------------------------------------------------------------------------------------
def _decoded(idx, C):
    """float32 restatement of the SQ8 decoder over the index's codes, lists and ranges (tests/test_gpu_ivf_sq8.py)."""
    vmin, vdiff = idx.ranges()
    return C[idx.assignment()] + (vmin + ((idx.codes().astype(F32) + F32(0.5)) / F32(255)) * vdiff)


@pytest.fixture(scope="module", params=[("flat", 50), ("flat", 64), ("sq8", 50), ("sq8", 64)], ids=lambda p: f"{p[0]}-{p[1]}")
def adds(request, vdb, oracle):
    """6001 clustered rows in 24 lists; `new()` makes an empty index of the codec with centroids (and ranges); `whole` holds
    one add of X, `ref` its results at nprobe 4 -- equal to the oracle over the rows the codec keeps."""
    codec, d = request.param
    rng = np.random.default_rng(d)
    centers = 3 * _gauss(rng, 24, d)
    X = centers[rng.integers(0, 24, 6001)] + _gauss(rng, 6001, d)
    Q = centers[rng.integers(0, 24, 100)] + _gauss(rng, 100, d)
    C = X[:24].copy()

    def new():
        idx = (vdb.IVFSQ8Index if codec == "sq8" else vdb.IVFFlatIndex)(d, 24, "l2", 0)
        idx.set_centroids(C)
        if codec == "sq8":
            idx.train_ranges(X)
        idx.set_nprobe(4)
        return idx

    whole = new()
    whole.add(X, id_base=40)
    ref = whole.search(Q, K)
    rows = _decoded(whole, C) if codec == "sq8" else X
    _equal(ref, oracle.ivf_search(rows, C, whole.assignment(), Q, K, 4, "l2", id_base=40))
    yield codec, X, Q, new, whole, ref
    whole.close()


def _same_index(idx, whole, codec, Q, ref):
    np.testing.assert_array_equal(idx.assignment(), whole.assignment())
    if codec == "sq8":
        np.testing.assert_array_equal(idx.codes(), whole.codes())
    _equal(idx.search(Q, K), ref)


def test_split_and_assigned_adds_equal_one_add(adds):
    """X[:a] then X[a:] (and an empty third add), and `add_assigned` with the stored lists in two parts: the index of one add."""
    codec, X, Q, new, whole, ref = adds
    split = new()
    split.add(X[:2501], id_base=40)
    split.add(X[2501:], id_base=40)
    split.add(X[:0], id_base=40)
    assert split.ntotal == len(X)
    _same_index(split, whole, codec, Q, ref)
    lor = whole.assignment()
    given = new()
    given.add(X[:2501], id_base=40, list_of_row=lor[:2501])
    given.add(X[2501:], id_base=40, list_of_row=lor[2501:])
    _same_index(given, whole, codec, Q, ref)
    split.close()
    given.close()


def test_refused_appends(adds):
    """An append that is refused leaves the index as it was, both codecs.  Another id base, and a list id out of range in
    `add_assigned` (checked before the add touches the handle): still built, same lists, same results."""
    codec, X, Q, new, whole, ref = adds
    idx = new()
    idx.add(X, id_base=40)
    with pytest.raises(ValueError, match="id.base"):
        idx.add(X[:10], id_base=41)
    _same_index(idx, whole, codec, Q, ref)
    for where, value in ((7, 24), (0, -1), (9, 2**31 - 1)):
        bad = np.zeros(10, np.int32)
        bad[where] = value
        with pytest.raises(ValueError, match="row could not be assigned to a list"):
            idx.add(X[:10], id_base=40, list_of_row=bad)
        assert idx.stats()["ntotal"] == len(X)
        _same_index(idx, whole, codec, Q, ref)
    idx.add(X[:0], id_base=40, list_of_row=np.zeros(0, np.int32))      # (nothing to check, nothing to add)
    _same_index(idx, whole, codec, Q, ref)
    idx.close()
    fresh = new()                       # the first add of an index: refused as well, and the next add builds it
    with pytest.raises(ValueError, match="row could not be assigned to a list"):
        fresh.add(X[:10], id_base=40, list_of_row=np.full(10, 24, np.int32))
    assert fresh.stats()["ntotal"] == 0
    fresh.add(X, id_base=40)
    _same_index(fresh, whole, codec, Q, ref)
    fresh.close()

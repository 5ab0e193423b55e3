"""CPU checks of tests/hostile_cases.py: the cases are hostile in the way they claim, no compared key is NaN, the oracle's
behaviour on infinite and subnormal keys is pinned, and the path labels that tests/test_gpu_hostile.py asserts follow from the
thresholds in csrc/prep.hpp with a factor-4 margin."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from tests import hostile_cases as hc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "vectordb-retrieval_amd" / "csrc"
N = 600                    # rows of the host-side corpora (the GPU file builds the same families at each path's size)
FLT_MAX = np.float32(hc.FLT_MAX)


def _all_keys(oracle, X, Q, metric):
    ids = np.tile(np.arange(len(X), dtype=np.int64), (len(Q), 1))
    return oracle.pair_keys(X, Q, ids, metric)


# ---- the thresholds the labels are derived from ---------------------------------------------------------------------------------
def test_the_restated_thresholds_are_the_ones_in_the_source():
    prep = (CSRC / "prep.hpp").read_text()
    m = re.search(r"force_fallback = \(nonfinite \|\| !\(top < ([0-9.e+-]+)f\) \|\| !\(sq \* f\.sx > ([0-9.e+-]+)f\) \|\| !q_fits \|\| !norms_fit\)", prep)
    assert m, "query_finalize_values no longer has the form that hostile_cases.batch_scales restates"
    assert float(m.group(1)) == hc.TOP_MAX and float(m.group(2)) == hc.SCALE_MIN
    m = re.search(r"const bool q_fits = fm \* amax \* sq <= ([0-9.e+-]+)f;", prep)
    assert m and float(m.group(1)) == hc.Q_FP16_MAX == float(np.finfo(np.float16).max)
    m = re.search(r"if \(!int_ok && amax > 0\.f && amax <= ([0-9.e+-]+)f\)", prep)
    assert m and float(m.group(1)) == hc.AMAX_GATE
    m = re.search(r"const bool norms_fit = f\.maxnorm2 < ([0-9.e+-]+)f;", prep)
    assert m and float(m.group(1)) == hc.NORM_MAX
    assert "sq = ldexpf(1.f, 14 - e);" in prep and "const float top = sq * f.sx * f.maxnorm2;" in prep
    lib = (CSRC / "vdbhip.hip").read_text()
    assert "h->sx = ldexpf(1.f, 14 - e);" in lib and "h->absmax <= 2048.f" in lib
    assert hc.LABEL_MARGIN >= 4.0


def test_labels_keep_a_factor_four_from_every_threshold():
    """a labelled cell's restated top and scale are at least a factor 4 from 1e30 / 1e-30, so a last-bit difference between NumPy
    and the device cannot flip the flag; "must" cells are flagged and "may" cells are not by the restated rule itself"""
    counts = {"must": 0, "may": 0, None: 0}
    for fam in ("ladder", "outlier", "tiny", "subnormal", "bytes", "inf-query", "nan-query"):
        for name, X, Q, metric, k, exp in hc.cases(fam, N):
            b, label = exp["batch"], exp["label"]
            counts[label] += 1
            with np.errstate(all="ignore"):
                if label == "must":
                    assert b["fallback"], name
                    if not b["nonfinite"]:
                        assert not (b["top"] < np.float32(4e30)) or not (b["scale"] > np.float32(0.25e-30)) or \
                            not (b["qtop"] <= np.float32(4 * 65504.0)), name
                elif label == "may":
                    assert not b["fallback"], name
                    assert b["top"] < np.float32(0.25e30) and b["scale"] > np.float32(4e-30) and b["qtop"] <= np.float32(16376.0), name
                else:
                    assert label is None and (fam in ("ladder", "bytes") or "norm-2e38" in name), name
    assert counts["must"] > 100 and counts["may"] > 50 and counts[None] < 20, counts


# ---- every case is hostile in the way it claims -------------------------------------------------------------------------------------
def test_the_ladder_covers_every_cell_and_its_marked_steps_overflow():
    cells = {(exp["step"], ) for *_, exp in hc.cases("ladder", N)}
    got = {(n.split("/")[0], n.split("/")[1]) for n, *_ in hc.cases("ladder", N)}
    assert got == {(f"ladder-x{a:+d}", f"q{b:+d}") for a in hc.LADDER for b in hc.LADDER} and cells
    for g in hc.groups("ladder", N):
        a, X = g.corpus.expect["step"], g.corpus.X
        cs = hc.corpus_scales(X)
        assert np.isfinite(X).all() and not cs["nonfinite"]
        # sum x^2 leaves float32 range although every value is finite (a >= 19), in float64 it does not
        assert cs["norm_overflow"] == (a >= 19), a
        assert np.isinf(cs["maxnorm2"]) == (a >= 19) and np.isfinite(cs["norm64_max"])
        # ldexpf(1, 14 - e) leaves float32 range exactly when absmax < 2^-113
        assert cs["sx_overflow"] == bool(cs["absmax"] < np.float32(2.0 ** -113)) == (a <= -36), a
        with np.errstate(over="ignore"):
            assert np.isinf(np.ldexp(np.float32(1), 14 - int(np.frexp(cs["absmax"])[1]))) == (a <= -36)
        if a in (-44, -40):           # float32 subnormals on purpose
            assert (np.abs(X[X != 0]) < np.float32(2.0 ** -126)).all() and (X != 0).any()
        if a == 38:
            assert (np.abs(X) == FLT_MAX).any()
    for b in hc.ladder_batches(hc.D):
        assert np.isfinite(b.Q).all()
        if b.expect["step"] in (-44, -40):
            assert (np.abs(b.Q[b.Q != 0]) < np.float32(2.0 ** -126)).all() and (b.Q != 0).any()


def test_outlier_rows_leave_every_other_row_zero_in_fp16():
    for g in hc.groups("outlier", N):
        cs = hc.corpus_scales(g.corpus.X)
        rows = g.corpus.expect.get("outliers")
        if g.corpus.name == "scaled-to-norm-2e38":
            n2 = (g.corpus.X.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
            assert np.isfinite(n2).all() and n2.max() > np.float32(1.9e38) and (n2 >= np.float32(0.9e38)).mean() > 0.02
            assert (n2[list(g.corpus.expect["longest"])] >= np.float32(0.9e38)).all()
            continue
        if rows is None:              # the transpose: one scaled query
            for b in g.batches:
                q = b.expect["scaled_query"]
                others = np.delete(np.arange(hc.NQ), q)
                assert np.abs(b.Q[q]).max() > 1e17 and np.abs(b.Q[others]).max() < 10
                bscale = np.float32(2) * hc.batch_scales(cs, b.Q, "l2")["sq"]
                assert ((b.Q[others] * bscale).astype(np.float16) == 0).all()
            continue
        mask = np.ones(N, bool)
        mask[list(rows)] = False
        assert not cs["sx_overflow"] and np.isfinite(cs["sx"])
        with np.errstate(under="ignore"):
            assert ((g.corpus.X[mask] * cs["sx"]).astype(np.float16) == 0).all()         # under the restated sx
            assert ((g.corpus.X[~mask] * cs["sx"]).astype(np.float16) != 0).any()
        assert cs["norm_overflow"] == (g.corpus.expect["scale"] == 30)
        if g.corpus.name == "outlier-norm-2e38":
            assert np.float32(0.9e38) < cs["maxnorm2"] < FLT_MAX and np.isfinite(cs["norm32_max"])


def test_tiny_subnormal_and_byte_corpora_are_what_they_say():
    (g,) = hc.groups("tiny", N)
    assert (g.corpus.X[:, 0] == np.float32(1e15)).all() and np.abs(g.corpus.X[:, 1:]).max() < 10
    (g,) = hc.groups("subnormal", N)
    X, Q = g.corpus.X, g.batches[0].Q
    assert (np.abs(X) < np.float32(2.0 ** -126)).all() and (np.abs(Q) < np.float32(2.0 ** -126)).all()
    assert (np.count_nonzero(X, axis=1) == 1).all() and (Q != 0).all()
    assert (np.signbit(X) & (X == 0)).any(), "-0.0 is among the values"
    (g,) = hc.groups("bytes", N)
    cs = hc.corpus_scales(g.corpus.X)
    assert cs["byte"] and cs["int_unscaled"] and cs["sx"] == 1
    i8 = {b.name: hc.batch_scales(cs, b.Q, "l2")["i8"] for b in g.batches}
    assert i8["q-bytes"] and not i8["q-bytes-255.5"] and not i8["q-bytes-1e6"] and not i8["q-inf-of-8"]


@pytest.mark.parametrize("family", [f for f in hc.FAMILIES if f != "nan-rows"])
def test_rows_within_a_case_are_distinct(family):
    for g in hc.groups(family, N):
        assert len(np.unique(g.corpus.X, axis=0)) == len(g.corpus.X), g.corpus.name


# ---- no key under bit-for-bit comparison is NaN ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", hc.FAMILIES)
def test_no_compared_key_is_nan(family, oracle):
    """The sign of a NaN made by inf - inf or 0 * inf is hardware-defined, and the oracle's bit order puts the two signs at
    opposite ends.  The only NaN keys are those propagated from a NaN in the input: the nan-query's own row of results and the
    nan-rows ("Hostile values", says how each is compared)."""
    for g in hc.groups(family, N) + (hc.groups("inf-rows", 40) if family == "inf-rows" else ()):
        for b in g.batches:
            for metric in g.metrics:
                keys = _all_keys(oracle, g.corpus.X, b.Q, metric)
                ok = np.ones(keys.shape, bool)
                if family == "nan-query" or (family == "bytes" and "nan" in b.name):
                    ok[list(b.expect["bad_queries"])] = False
                    assert np.isnan(keys[~ok]).all()
                if family == "nan-rows":
                    ok[:, list(g.corpus.expect["nan_rows"])] = False
                    assert np.isnan(keys[~ok]).all()
                    # propagated from np.nan: positive under L2, negated (negative) under IP, on every such pair
                    assert (np.signbit(keys[~ok]) == (metric == "ip")).all()
                assert not np.isnan(keys[ok]).any(), (g.corpus.name, b.name, metric)
                if family == "inf-rows":
                    inf_keys = keys[:, list(g.corpus.expect["inf_rows"])]
                    assert np.isinf(inf_keys).all() and ((inf_keys > 0).all() if metric == "l2" else True)
                if family == "inf-query" or (family == "bytes" and "inf" in b.name):
                    assert np.isinf(keys[list(b.expect["bad_queries"])]).all()


# ---- the oracle on these inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_oracle_puts_infinite_keys_after_finite_ones_and_before_the_padding(metric, oracle):
    n = 40
    for g in hc.groups("inf-rows", n):
        X, Q = g.corpus.X, g.batches[0].Q
        inf_rows = np.array(g.corpus.expect["inf_rows"])
        r = len(inf_rows)
        assert {n - r, n, n + 5} <= set(g.ks) and min(g.ks) < n - r
        D, I, keys = oracle.knn(X, Q, n + 5, metric, return_keys=True)
        allk = _all_keys(oracle, X, Q, metric)
        for q in range(len(Q)):
            first = np.sort(inf_rows[allk[q, inf_rows] < 0])            # IP: score +inf, key -inf: ahead of every finite key, by id
            last = np.sort(inf_rows[allk[q, inf_rows] > 0])
            assert metric == "ip" or len(first) == 0
            np.testing.assert_array_equal(I[q, :len(first)], first)
            np.testing.assert_array_equal(I[q, n - len(last):n], last)       # after every finite key, by id, before the padding
            np.testing.assert_array_equal(I[q, n:], -1)
            mid = I[q, len(first):n - len(last)]
            assert np.isfinite(keys[q, len(first):n - len(last)]).all() and not np.isin(mid, inf_rows).any()
            want_first, want_last = (np.inf, -np.inf) if metric == "ip" else (-np.inf, np.inf)
            assert (D[q, :len(first)] == want_first).all() and (D[q, n - len(last):n] == want_last).all()
            assert (D[q, n:] == (FLT_MAX if metric == "l2" else -FLT_MAX)).all()
            assert np.isfinite(D[q, len(first):n - len(last)]).all()


def test_oracle_writes_inf_for_a_finite_key_above_flt_max(oracle):
    g = hc.groups("ladder", N)[-1]                   # 10^38: keys ~1e77, finite in float64
    D, I, keys = oracle.knn(g.corpus.X, hc.ladder_batches(hc.D)[6].Q, 5, "l2", return_keys=True)
    assert np.isfinite(keys).all() and (keys > hc.FLT_MAX).all() and np.isinf(D).all() and (I >= 0).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_oracle_orders_subnormal_keys(metric, oracle):
    (g,) = hc.groups("subnormal", N)
    D, I, keys = oracle.knn(g.corpus.X, g.batches[0].Q, 32, metric, return_keys=True)
    assert (np.diff(keys, axis=1) > 0).all(), "subnormal keys are distinct and ordered"
    assert (np.abs(keys) < 1e-70).all() and (D == 0).all()          # ~2^-298 q^2: far below float32, exact in float64
    allk = _all_keys(oracle, g.corpus.X, g.batches[0].Q, metric)
    np.testing.assert_array_equal(np.sort(allk, axis=1)[:, :32], keys)
    if metric == "ip":
        assert all(len(np.unique(r)) == len(r) for r in allk)

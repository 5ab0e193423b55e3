"""k-means training on the GPU, bit for bit: the centroids of vdb_ivf_train and the codebooks of vdb_pq_train / vdb_ivfpq_train
equal the NumPy restatement (tests/kmeans_restatement.py) with the CPU oracle's assignment injected.  Every comparison is
assert_array_equal on float32; there is no tolerance in this file.  The shapes are the smallest that reach each path of the
sampler, the CSR build (device chunks, more than 1024 lists, the host fallback), the update kernel (padded stride, partial
64-dimension blocks, the spherical norm over several blocks) and the empty-cell split.

What the Gaussian cases cannot see is the ORDER of the rows inside a list: a float64 sum of a few hundred float32 values taken in
another order differs in its last bits, and the rounding to float32 hides them (reversing every list changes no centroid of any
Gaussian case here).  test_summation_order_reaches_the_centroid repeats the device-CSR cases on rows built so that it does.
The order of the additions inside the spherical norm cannot be made visible at all: its terms are squares, nothing cancels,
and (float)(1 / sqrt(n2)) hides a last-bit difference of n2 except about once in 2^29 centroids."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import kmeans_restatement as ref  # noqa: E402
from tests.helpers import np_ranges  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 1234


def _gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F32)


def _ints(n, d, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(F32)


def _duplicates(seed):
    return np.repeat(_gauss(32, 6, seed), 2, axis=0)           # 64 rows, every row twice


def _cancelling(n, nlist, seed):
    """(n, 8) rows whose float32 centroids depend on the ORDER of the float64 additions.  On Gaussian rows they do not: a
    reordered sum differs in the last bits of the float64, which the rounding to float32 hides.  Here the lists are fixed by
    construction -- list k is the rows at grid point k of dimensions 0 and 1 (spacing 2^15), and the rows the sampler draws first
    (the init) are one per grid point -- and in dimensions 2 .. 7 every list holds three rows of +2^12 and three of -2^12 among rows
    of size 2^-20.  The large values cancel exactly, but while a partial sum is large it has no bits left for what a small row adds:
    which small rows are rounded away depends on where they stand between the large ones."""
    rng = np.random.default_rng(seed)
    assert n >= 8 * nlist and n <= 256 * nlist                  # every list has room for the six large rows; the sample is all rows
    pick = ref.sample_rows(n, n, SEED)
    cl = rng.integers(0, nlist, size=n)
    cl[pick[:nlist]] = np.arange(nlist)                         # the init holds one row of every list ...
    cl[rng.permutation(pick[nlist:])[:7 * nlist]] = np.repeat(np.arange(nlist), 7)  # ... and every list at least 8 rows
    side = int(np.ceil(np.sqrt(nlist)))
    X = np.empty((n, 8), F32)
    X[:, 0] = (cl % side) * 2.0 ** 15
    X[:, 1] = (cl // side) * 2.0 ** 15
    X[:, 2:] = rng.standard_normal((n, 6)) * 2.0 ** -20
    for k in range(nlist):
        rows = np.nonzero(cl == k)[0]
        for d in range(2, 8):
            six = rng.choice(rows, size=6, replace=False)
            X[six[:3], d], X[six[3:], d] = 2.0 ** 12, -2.0 ** 12
    return X, cl


def _train_twice(index, X, niter, mpc):
    index.train(X, niter=niter, seed=SEED, max_points_per_centroid=mpc)
    first = index.centroids()
    index.train(X, niter=niter, seed=SEED, max_points_per_centroid=mpc)
    return first, index.centroids()


def _check(vdb, oracle, X, nlist, niter, mpc, metric, need_splits=False):
    want, splits, sizes = ref.kmeans(X, nlist, niter, SEED, mpc, metric, oracle.ivf_assign)
    if need_splits:                                             # a condition on the reference: the case reaches the split rule
        assert splits >= 1, splits
    index = vdb.IVFFlatIndex(X.shape[1], nlist, metric, 0)
    try:
        first, second = _train_twice(index, X, niter, mpc)
    finally:
        index.close()
    assert first.dtype == F32 and first.shape == (nlist, X.shape[1])
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)
    return want, splits


# ---- the sampler and the init alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mpc,ns", [(16, 592), (0, 5000)])
def test_niter_0_returns_the_first_nlist_draws(vdb, oracle, mpc, ns):
    X = _gauss(5000, 8, 1)
    want, _ = _check(vdb, oracle, X, 37, 0, mpc, "l2")
    pick = ref.sample_rows(5000, ns, SEED)
    np.testing.assert_array_equal(want, X[pick[:37]])           # (what the restatement itself must say here)
    assert pick[:37].tolist() != list(range(37))               # ns == n is still a permutation, not the identity


# ---- the update kernel: strides, blocks, the spherical norm ---------------------------------------------------------------------
@pytest.mark.parametrize("n,d,nlist,niter,mpc,metric", [
    (3000, 3, 37, 4, 0, "l2"),            # padded stride D4 = 4 != D; nlist % 4 != 0 (the last block of the update has one wave idle)
    (3000, 70, 37, 3, 0, "ip"),           # a partial second 64-dimension block; the norm runs over two blocks
    (9000, 130, 50, 3, 100, "ip"),        # three blocks, D4 = 132; a strict sub-sample (5000 of 9000 rows)
], ids=["d3", "d70-ip", "d130-ip-subsample"])
def test_update_kernel_shapes(vdb, oracle, n, d, nlist, niter, mpc, metric):
    _check(vdb, oracle, _gauss(n, d, d), nlist, niter, mpc, metric)


# ---- the CSR build: list order is summation order -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,nlist,niter", [
    (8229, 8, 300, 3),                    # three chunks of 4096 rows, the last with 37 rows (not a multiple of 64); nlist > 256
    (9000, 4, 1030, 2),                   # the offsets scan takes a second round of 1024 lists
    (16400, 2, 8200, 2),                  # nlist > kCsrMaxLists: the host counting sort
], ids=["chunks", "offsets-rounds", "host-csr"])
def test_csr_paths(vdb, oracle, n, d, nlist, niter):
    _check(vdb, oracle, _gauss(n, d, nlist), nlist, niter, 0, "l2")


@pytest.mark.parametrize("n,nlist", [(8229, 300), (9000, 1030)], ids=["chunks", "offsets-rounds"])
def test_summation_order_reaches_the_centroid(vdb, oracle, n, nlist):
    """The CSR cases again on rows where a list summed in another order gives other float32 centroids (the Gaussian rows above pin
    WHICH rows a list holds, not their order).  First the conditions on the reference: the lists are the constructed ones, and
    summing them backwards changes many centroids."""
    X, cl = _cancelling(n, nlist, nlist)
    want, _ = _check(vdb, oracle, X, nlist, 2, 0, "l2")
    S = X[ref.sample_rows(n, n, SEED)]
    lor = oracle.ivf_assign(want, S, "l2")
    np.testing.assert_array_equal(lor, cl[ref.sample_rows(n, n, SEED)])
    backwards = np.stack([ref.list_mean(S[lor == c][::-1]) for c in range(nlist)])
    forwards = np.stack([ref.list_mean(S[lor == c]) for c in range(nlist)])
    np.testing.assert_array_equal(forwards, want)              # (the lists no longer move: the update is at its fixed point)
    assert (backwards != want).any(axis=1).sum() >= nlist // 2


# ---- empty cells ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,nlist,niter,metric", [
    (lambda: _ints(2000, 2, 0, 3, 8), 32, 4, "l2"),             # 16 distinct rows for 32 lists
    (lambda: _ints(1500, 5, -1, 1, 9), 40, 4, "ip"),            # ... and zero rows: centroids of zero norm stay unnormalised
    (lambda: _duplicates(10), 64, 3, "l2"),                     # n == nlist, every row twice: ties go to the smaller list
], ids=["ints-l2", "ints-ip", "duplicates"])
def test_empty_cells_are_split(vdb, oracle, make, nlist, niter, metric):
    _check(vdb, oracle, make(), nlist, niter, 0, metric, need_splits=True)


# ---- codebooks ------------------------------------------------------------------------------------------------------------------
def _pq_train_twice(index, X, niter, mpc):
    index.train(X, niter=niter, seed=SEED, max_points_per_centroid=mpc)
    first = index.codebooks()
    index.train(X, niter=niter, seed=SEED, max_points_per_centroid=mpc)
    return first, index.codebooks()


def test_pq_codebooks(vdb, oracle):
    X = _gauss(600, 8, 21)                                      # mpc = 2: a sample of 512 of the 600 rows, permuted again per sub-space
    want, _ = ref.pq_codebooks(X, 4, 3, SEED, 2, oracle.ivf_assign)
    index = vdb.PQIndex(8, 4, "l2", 0)
    try:
        first, second = _pq_train_twice(index, X, 3, 2)
    finally:
        index.close()
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)


def test_pq_codebooks_of_one_dimension_with_empty_cells(vdb, oracle):
    X = _ints(3000, 4, 0, 255, 22)                              # dsub = 1: 256 draws of byte values repeat, so lists start empty
    want, splits = ref.pq_codebooks(X, 4, 3, SEED, 0, oracle.ivf_assign)
    assert all(s >= 1 for s in splits), splits
    index = vdb.PQIndex(4, 4, "ip", 0)                          # (the metric does not enter the codebooks)
    try:
        first, second = _pq_train_twice(index, X, 3, 0)
    finally:
        index.close()
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivfpq_codebooks(vdb, oracle, metric):
    X = _gauss(2000, 8, 23)
    C = _gauss(16, 8, 24)
    want, _ = ref.ivfpq_codebooks(X, C, 2, 3, SEED, 4, metric, oracle.ivf_assign)      # mpc = 4: 1024 of the 2000 rows
    index = vdb.IVFPQIndex(8, 16, 2, metric, 0)
    try:
        index.set_centroids(C)
        index.train_codebooks(X, niter=3, seed=SEED, max_points_per_centroid=4)
        first = index.codebooks()
        index.train_codebooks(X, niter=3, seed=SEED, max_points_per_centroid=4)
        second = index.codebooks()
        np.testing.assert_array_equal(index.centroids(), C)     # training the codebooks leaves the centroids alone
    finally:
        index.close()
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)


# ---- the other handles that train ----------------------------------------------------------------------------------------------
def test_sq8_handle_trains_the_same_centroids_then_its_ranges(vdb, oracle):
    X = _gauss(2000, 10, 31)
    want, _, _ = ref.kmeans(X, 24, 3, SEED, 40, "l2", oracle.ivf_assign)               # 960 of the 2000 rows
    index = vdb.IVFSQ8Index(10, 24, "l2", 0)
    try:
        first, second = _train_twice(index, X, 3, 40)
        vmin, vdiff = index.ranges()
    finally:
        index.close()
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)
    wmin, wdiff = np_ranges(X, want, oracle.ivf_assign(want, X, "l2"))                 # the ranges read ALL rows, not the sample
    np.testing.assert_array_equal(vmin, wmin)
    np.testing.assert_array_equal(vdiff, wdiff)


def test_multi_device_handle_trains_the_same_centroids(vdb, oracle):
    X = _gauss(2000, 10, 32)
    want, _, _ = ref.kmeans(X, 24, 3, SEED, 40, "ip", oracle.ivf_assign)
    index = vdb.IVFFlatIndex(10, 24, "ip", [0, 0])
    try:
        first, second = _train_twice(index, X, 3, 40)
    finally:
        index.close()
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)

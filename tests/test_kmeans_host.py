"""k-means training, host side (no GPU): the pieces of the NumPy restatement (tests/kmeans_restatement.py) against plainer
statements of themselves -- the generator against the C++ standard's values, the sampler, the sequential float64 update, the
butterfly sum, the empty-cell rule -- and the whole against the CPU oracle's assignment."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import kmeans_restatement as ref  # noqa: E402

F32 = np.float32


def test_generator_is_std_mt19937_64():
    rng = ref.MT19937_64(1234)                            # a compiled std::mt19937_64(1234)
    assert [rng() for _ in range(3)] == [17473339210090333472, 963351229459618018, 17972999874122035550]
    rng = ref.MT19937_64()                                # [rand.predef]: the 10000th invocation of a default-constructed one
    for _ in range(9999):
        rng()
    assert rng() == 9981545732273789042
    assert ref.MT19937_64((1 << 64) + 1234)() == 17473339210090333472      # the seed is a uint64_t


def test_sample_rows_is_a_seeded_permutation_prefix():
    pick = ref.sample_rows(1000, 40, 7)
    assert pick.dtype == np.int64 and pick[:8].tolist() == [15, 493, 548, 495, 113, 683, 13, 167]
    assert sorted(pick.tolist()) == list(range(1000))
    assert np.array_equal(pick, ref.sample_rows(1000, 40, 7)) and not np.array_equal(pick, ref.sample_rows(1000, 40, 8))
    # a longer sample extends a shorter one: the draws do not depend on ns
    assert np.array_equal(ref.sample_rows(1000, 90, 7)[:40], pick[:40])
    # rows the draws never touched stay where they were
    touched = set(pick[:40].tolist()) | set(range(40))
    assert all(pick[r] == r for r in range(1000) if r not in touched)
    # ns == n: n - 1 draws, a permutation and not the identity; the last draw (i == n - 1) would be rng() % 1 == 0 anyway
    full = ref.sample_rows(50, 50, 3)
    assert sorted(full.tolist()) == list(range(50)) and full.tolist() != list(range(50))
    rng = ref.MT19937_64(3)
    want = list(range(50))
    for i in range(49):
        j = i + rng() % (50 - i)
        want[i], want[j] = want[j], want[i]
    assert full.tolist() == want
    # n == 1: no draw at all
    assert ref.sample_rows(1, 1, 99).tolist() == [0]
    assert ref.sample_rows(2, 1, 5).tolist() in ([0, 1], [1, 0]) and ref.sample_rows(5, 0, 5).tolist() == [0, 1, 2, 3, 4]


def test_update_is_a_strictly_sequential_float64_sum():
    rng = np.random.default_rng(0)
    # magnitudes spread over 2^40: the float64 sum depends on the order, so a pairwise or blocked sum would differ
    rows = (rng.standard_normal((301, 5)) * np.exp2(rng.integers(-20, 20, size=(301, 5)))).astype(F32)
    want = np.empty(5, F32)
    for d in range(5):
        acc = 0.0
        for r in range(rows.shape[0]):
            acc += float(rows[r, d])
        want[d] = F32(acc / float(rows.shape[0]))
    got = ref.list_mean(rows)
    assert got.dtype == F32 and np.array_equal(got, want)
    assert np.array_equal(ref.list_mean(rows[:1]), rows[0])
    # the order matters to the float64 sum somewhere on this data: the case can tell sequential from pairwise
    seq = np.cumsum(rows.astype(np.float64), axis=0)[-1]
    assert not np.array_equal(seq, np.cumsum(rows[::-1].astype(np.float64), axis=0)[-1])


def _xor_butterfly(v):
    """64 lanes, every lane adds the lane `o` away for o = 32 .. 1 (what __shfl_xor does); returns all 64 lanes."""
    lanes = [float(x) for x in v]
    o = 32
    while o:
        lanes = [lanes[i] + lanes[i ^ o] for i in range(64)]
        o >>= 1
    return lanes


def test_butterfly_equals_the_xor_shuffle_on_every_lane():
    rng = np.random.default_rng(1)
    for _ in range(20):
        v = rng.standard_normal(64) * np.exp2(rng.integers(-30, 30, size=64))
        lanes = _xor_butterfly(v)
        assert len(set(lanes)) == 1 and ref.butterfly_sum(v) == lanes[0]
    v = rng.standard_normal(64) * np.exp2(rng.integers(-30, 30, size=64))
    assert ref.butterfly_sum(v) != float(np.cumsum(v)[-1])             # ... and it is not the sequential sum
    # n2: blocks in ascending order, lanes d >= D contribute 0
    m = (rng.standard_normal(130) * np.exp2(rng.integers(-12, 12, size=130))).astype(F32)
    sq = np.zeros(192)
    sq[:130] = m.astype(np.float64) ** 2
    want = 0.0
    for b in range(3):
        want = want + _xor_butterfly(sq[64 * b:64 * b + 64])[0]
    assert ref.squared_norm(m) == want
    assert ref.squared_norm(m[:3]) == _xor_butterfly(sq[:3].tolist() + [0.0] * 61)[0]
    # normalisation: float32 product with (float)(1 / sqrt(n2)); a zero centroid stays as it is
    inv = F32(1.0 / np.sqrt(want))
    assert np.array_equal(ref.normalize(m), m * inv) and ref.normalize(m).dtype == F32
    assert np.array_equal(ref.normalize(np.zeros(7, F32)), np.zeros(7, F32))


def test_split_rule_on_a_hand_made_count():
    # lists 1 and 4 are empty.  First split: the first largest is list 2 (10 rows; list 5 also has 10) -> 1 gets 5, 2 keeps 5.
    # Second split sees the halved count: the largest is now list 5 (10), not list 2 -> 4 gets 5, 5 keeps 5.
    cnt = np.array([3, 0, 10, 7, 0, 10], np.int64)
    cent = (np.arange(18, dtype=F32).reshape(6, 3) + 1) * F32(1.1)
    before = cent.copy()
    assert ref.split_empty(cent, cnt) == 2
    assert cnt.tolist() == [3, 5, 5, 7, 5, 5]
    up = np.array([1 - 1 / 1024, 1 + 1 / 1024, 1 - 1 / 1024], F32)       # even d: -1/1024, odd d: +1/1024 on the new cell
    down = np.array([1 + 1 / 1024, 1 - 1 / 1024, 1 + 1 / 1024], F32)
    assert np.array_equal(cent[1], before[2] * up) and np.array_equal(cent[2], before[2] * down)
    assert np.array_equal(cent[4], before[5] * up) and np.array_equal(cent[5], before[5] * down)
    assert np.array_equal(cent[[0, 3]], before[[0, 3]]) and cent.dtype == F32
    # an odd count: the new cell gets the smaller half; a cell split twice halves again
    cnt = np.array([0, 0, 7], np.int64)
    cent = np.ones((3, 2), F32)
    assert ref.split_empty(cent, cnt) == 2 and cnt.tolist() == [3, 2, 2]
    d2 = F32(1) * (F32(1) + F32(1 / 1024))                                  # list 2, dimension 0, after the first split
    assert cent[0, 0] == F32(1) * (F32(1) - F32(1 / 1024)) and cent[1, 0] == d2 * (F32(1) - F32(1 / 1024))
    assert cent[2, 0] == d2 * (F32(1) + F32(1 / 1024))
    # nothing empty: nothing moves
    cnt = np.array([1, 2], np.int64)
    assert ref.split_empty(cent[:2], cnt) == 0 and cnt.tolist() == [1, 2]


def test_kmeans_on_the_oracle_assignment(oracle):
    """The whole restatement with the CPU oracle's assignment injected: niter = 0 is the init, empty lists keep their centroid
    until the split, duplicates tie to the smaller list, and the IP centroids that were updated have unit norm."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((700, 6)).astype(F32)
    C0, s0, sizes0 = ref.kmeans(X, 20, 0, 11, 10, "l2", oracle.ivf_assign)
    assert np.array_equal(C0, X[ref.sample_rows(700, 200, 11)[:20]]) and s0 == 0 and not sizes0.any()
    C1, s1, sizes1 = ref.kmeans(X, 20, 1, 11, 10, "l2", oracle.ivf_assign)
    S = X[ref.sample_rows(700, 200, 11)[:200]]
    lor = oracle.ivf_assign(C0, S, "l2")
    assert sizes1.sum() == 200 and np.array_equal(sizes1, np.bincount(lor, minlength=20)) and s1 == 0
    for c in range(20):
        assert np.array_equal(C1[c], ref.list_mean(S[lor == c]))
    # mpc <= 0 means 256; the same arguments give the same bits
    a = ref.kmeans(X, 20, 2, 11, 0, "ip", oracle.ivf_assign)
    b = ref.kmeans(X, 20, 2, 11, 256, "ip", oracle.ivf_assign)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 0
    np.testing.assert_allclose(np.linalg.norm(a[0].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # n == nlist with every row twice: the second copy ties with the first and goes to the smaller list, so half the lists are
    # empty after the first assignment and get split
    half = rng.standard_normal((16, 4)).astype(F32)
    dup = np.repeat(half, 2, axis=0)
    C, splits, sizes = ref.kmeans(dup, 32, 1, 2, 0, "l2", oracle.ivf_assign)
    assert splits == 16 and sorted(sizes.tolist()) == [0] * 16 + [2] * 16
    # sub-space codebooks: kmeans per column block, seed + m, on one shared sample
    Y = rng.standard_normal((600, 4)).astype(F32)
    cb, sp = ref.pq_codebooks(Y, 2, 1, 9, 2, oracle.ivf_assign)
    Ys = Y[ref.sample_rows(600, 512, 9)[:512]]
    assert cb.shape == (2, 256, 2) and len(sp) == 2
    assert np.array_equal(cb[1], ref.kmeans(np.ascontiguousarray(Ys[:, 2:]), 256, 1, 10, 2, "l2", oracle.ivf_assign)[0])
    Cc = rng.standard_normal((8, 4)).astype(F32)
    cbr, _ = ref.ivfpq_codebooks(Y, Cc, 2, 1, 9, 2, "ip", oracle.ivf_assign)
    R = Ys - Cc[oracle.ivf_assign(Cc, Ys, "ip")]
    assert np.array_equal(cbr[0], ref.kmeans(np.ascontiguousarray(R[:, :2]), 256, 1, 9, 2, "l2", oracle.ivf_assign)[0])

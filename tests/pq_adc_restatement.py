"""NumPy restatement of the lookup-table (ADC) scan of a flat PQ<M> index (csrc/pq_adc.hpp, DESIGN 4.9 "ADC scan").  Test
infrastructure only: nothing in the product imports it.

  tables   T[q][m][c] = float32(bs * acc),  acc = sum_j fma(float64(q[m dsub + j]), float64(cb[m][c][j]), acc), j ascending from
           0.0, bs = -2 cs (L2) | -cs (IP), cs = sq * sx the power-of-two scale of the batch (guard_cases.scales)
  scores   s_0 = float32(cs * bias[row]) (bias = float32 of the float64 norm chain of x^; 0 for IP),
           s_{m+1} = float32(s_m + T[q][m][code[row][m]]), m ascending
  eps      1.02 cs [(M + 3) 2^-23 mag + 2^-17 mag], mag = Xn^2 + 2 qn Xn (L2) | qn Xn (IP), Xn = float32(sqrt(max ||x^||^2)) * 1.0000002
  packing  the low 6 mantissa bits of a group minimum carry the group's number inside its 256-row bin (octs for D <= 128, quads above)
  admission  which batches of a PQ handle take the ADC scan
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests import census
from tests import guard_cases as gc

F32 = np.float32
LDS_BUDGET = 160 * 1024          # kPqAdcLdsBudget (pq.inc)
AUX_BYTES = 128                  # kPqAdcAuxBytes (pq_adc.hpp)
MAX_PIECES = 8                   # kPqAdcMaxPieces


def _fma_add(a: np.ndarray, b: np.ndarray, acc: np.ndarray) -> np.ndarray:
    """fma(a, b, acc) element-wise in float64, correctly rounded, as pq_restatement._fma_sq_add does for squares: a * b = hi + lo
    exactly (Veltkamp / Dekker split), acc + hi = s + e exactly (two-sum), and s + (e + lo) is the single rounding of acc + a * b
    whenever e + lo is exact; an element where it is not is recomputed in exact rational arithmetic.  (For float32 inputs widened to
    float64 the product has 48 significant bits, so lo is 0 and this is acc + a * b; the split keeps the restatement independent of
    that.)"""
    a, b, acc = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(acc, np.float64))
    ca, cbb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    al = a - ah
    bh = cbb - (cbb - b)
    bl = b - bh
    hi = a * b
    lo = ((ah * bh - hi) + ah * bl + al * bh) + al * bl
    s = acc + hi
    bb = s - acc
    e = (acc - (s - bb)) + (hi - bb)
    tail = e + lo
    r = s + tail
    tb = tail - e
    doubtful = ((e - (tail - tb)) + (lo - tb)) != 0.0
    if np.any(doubtful):
        r = r.copy()
        for i in zip(*np.nonzero(doubtful)):
            r[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(acc[i])))
    return r


def decode(cb, codes):
    """x^ float32 (n, D): codebook[m][code[m]] side by side."""
    cb = np.asarray(cb, F32)
    return np.ascontiguousarray(np.concatenate([cb[m][codes[:, m]] for m in range(cb.shape[0])], axis=1), dtype=F32)


def bias_of(X, metric):
    """float32 (n,): what build_bias_kernel keeps per row -- the float64 fma chain of squares rounded once (L2), 0 (IP)."""
    if metric == "ip":
        return np.zeros(len(X), F32)
    acc = np.zeros(len(X), np.float64)
    X64 = np.asarray(X, F32).astype(np.float64)
    for j in range(X64.shape[1]):
        acc = _fma_add(X64[:, j], X64[:, j], acc)
    return acc.astype(F32)


def cs_of(X, Q, metric):
    sx, sq = gc.scales(X, Q, metric)
    return float(sx * sq)


def tables(cb, Q, metric, cs):
    """float32 (nq, M, 256)"""
    cb64 = np.asarray(cb, F32).astype(np.float64)
    M, _, dsub = cb64.shape
    Q64 = np.asarray(Q, F32).astype(np.float64).reshape(len(Q), M, dsub)
    acc = np.zeros((len(Q), M, 256), np.float64)
    for j in range(dsub):
        acc = _fma_add(Q64[:, :, None, j], cb64[None, :, :, j], acc)
    bs = (-2.0 if metric == "l2" else -1.0) * cs
    with np.errstate(over="ignore", invalid="ignore"):
        return (bs * acc).astype(F32)


def scores(T, codes, bias, cs):
    """float32 (nq, n): the sum in the kernel's one fixed order, one float32 rounding per add."""
    codes = np.asarray(codes)
    n, M = codes.shape
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.broadcast_to((np.asarray(bias, F32) * F32(cs)).astype(F32)[None, :], (T.shape[0], n)).copy()
        for m in range(M):
            s = (s + T[:, m, :][:, codes[:, m]]).astype(F32)
    return s


def xnorm_max(X):
    """Xn as the host hands it to the kernels: sqrtf(maxnorm2) * 1.0000002f, maxnorm2 the largest float32 row norm."""
    n2 = bias_of(X, "l2").max()
    return F32(np.sqrt(F32(n2))) * F32(1.0000002)


def eps(Q, M, metric, Xn, cs):
    """float32 (nq,): the ADC error bound (summation order of ||q||^2 aside: compare to a few ulp)."""
    qn = np.sqrt((np.asarray(Q, F32).astype(np.float64) ** 2).sum(axis=1))
    Xn = float(Xn)
    mag = Xn * Xn + 2.0 * qn * Xn if metric == "l2" else qn * Xn
    e = cs * 1.02 * ((M + 3) * 2.0 ** -23 * mag + 2.0 ** -17 * mag)
    e = np.where(e < 1.0e37, e, 1.0e37)
    return e.astype(F32) + F32(1.0e-30)


def exact_scaled_keys(X, Q, metric, cs):
    """float64 (nq, n): cs (||x^||^2 - 2 q.x^) | -cs q.x^, what a score approximates."""
    X64, Q64 = np.asarray(X, F32).astype(np.float64), np.asarray(Q, F32).astype(np.float64)
    g = Q64 @ X64.T
    if metric == "ip":
        return -cs * g
    return cs * ((X64 * X64).sum(axis=1)[None, :] - 2.0 * g)


def pack(s, low):
    """The low 6 mantissa bits cleared (low = 0), set (63) or replaced by `low` (an array of group ids)."""
    bits = np.asarray(s, F32).view(np.uint32)
    return ((bits & np.uint32(0xFFFFFFC0)) | np.asarray(low, np.uint32)).view(F32)


def group_rows(d):
    return 4 if d > 128 else 8


def packed_group_minima(s, d):
    """(nq, n / group) float32: the minimum of every candidate group, its number inside the 256-row bin in the low 6 bits.  n must be a
    multiple of the group size."""
    g = group_rows(d)
    nq, n = s.shape
    gm = s.reshape(nq, n // g, g).min(axis=2)
    ids = (np.arange(n // g) % (256 // g)).astype(np.uint32)
    return pack(gm, ids[None, :])


def survivors(s, d, k, geom, eps_q=None):
    """(nq, n) bool: the rows the select hands to the exact refine when its threshold is tau + 2 eps_q (None: eps = 0).  s (nq, n) raw
    scores of ALL rows; geom a census.Geometry of the search.  Restates scan + select_kernel: packed group minima, (min, second min)
    per 256-row bin, superbin (chunk, bin % G) minima, tau = the k-th smallest superbin minimum; a bin whose minimum is within the
    threshold gives the group of its minimum, one whose second minimum is within it too is re-scanned whole."""
    nq, n = s.shape
    grp, G, S = group_rows(d), census.bins_per_span(d), census.span_rows(d)
    npad = geom.nspans * S
    sp = np.full((nq, npad), F32(1.0e38), F32)
    sp[:, :n] = s
    pm = packed_group_minima(sp, d).reshape(nq, npad // 256, 256 // grp)
    order = np.sort(pm, axis=2)
    m1, m2 = order[:, :, 0], order[:, :, 1]
    arg = np.argmin(pm, axis=2)
    nbins = npad // 256
    chunk_of_span = np.repeat(np.arange(geom.nchunks), np.diff(geom.starts))
    sb_of_bin = chunk_of_span[np.arange(nbins) // G] * G + np.arange(nbins) % G
    sb = np.full((nq, geom.nchunks * G), np.inf, np.float64)
    np.minimum.at(sb, (np.arange(nq)[:, None], sb_of_bin[None, :]), m1.astype(np.float64))
    tau = np.sort(sb, axis=1)[:, k - 1].astype(F32)
    that = tau if eps_q is None else (tau + F32(2.0) * np.asarray(eps_q, F32)).astype(F32)
    active = m1 <= that[:, None]
    deep = active & (m2 <= that[:, None])
    mask = np.repeat(deep, 256, axis=1)
    qi, bi = np.nonzero(active & ~deep)
    first = bi * 256 + arg[qi, bi] * grp
    for j in range(grp):
        mask[qi, first + j] = True
    return mask[:, :n]


def wrong_mask(keys, surv, k):
    """Per query: the exact k-th and (k + 1)-th float64 keys differ and the k best rows (key, then row) do not all survive."""
    cols, kk = gc._first(keys, k + 1)
    distinct = kk[:, k - 1] != kk[:, k]
    return distinct & ~np.take_along_axis(surv, cols[:, :k], axis=1).all(axis=1)


def admitted(n, d, M, k, nq, adc_max_batch, force_path=0, spans_per_chunk=0):
    """Does a search of nq queries on a flat PQ handle take the ADC scan (search_batch)?"""
    if not (0 < nq <= adc_max_batch) or k > 1024 or force_path in (1, 3):
        return False
    g = census.scan_geometry(n, d, k, nq, spans_per_chunk)
    if not g.ok:
        return False                                                    # (direct bins, or no scan at all)
    npad = g.nspans * census.span_rows(d)
    if not (force_path == 2 or n >= 32768 or (npad > 8192 and nq * n >= 4.0e6)):
        return False
    return M * 1024 + AUX_BYTES <= LDS_BUDGET


def code_pitch(M):
    pitch = (M + 3) & ~3
    return pitch + 4 if (pitch // 4) % 2 == 0 else pitch


def staged(M):
    """Are the code rows of a bin staged in LDS (else read from the index)?"""
    return M % 4 == 0 and 16 * M <= 256 * MAX_PIECES and M * 1024 + AUX_BYTES + 256 * code_pitch(M) <= LDS_BUDGET

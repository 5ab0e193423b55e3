// lsh.hpp -- sign-LSH codes: encode, Hamming scan, top-c select (gfx950 only).  Host side: lsh.inc.
//
// Contract (include/vdbhip.h): bit j of a vector x is  s_j >= 0  with  s_j = sum_d (double)x[d] * (double)R[j][d], accumulated
// from 0.0 with d ascending and one rounding per step; the candidates of a query are the min(ncand, ntotal) rows smallest
// under (Hamming distance, row), in that order.
//
// Codes: `wp` uint32 words per row, wp = nbits / 32 rounded up to a power of two, the words past nbits / 32 zero in rows
// and queries alike (they add nothing to a distance), so the scan is compiled for wp in {1, 2, 4, 8, 16, 32} only.
//
// Select: distances are integers in [0, nbits], so the c-th smallest is found by counting.  Per query
//   1. lsh_sample_kernel   histogram of a row sample (128 runs of 256 rows) -> t_hi, a generous upper bound of the cut distance
//                          (the whole corpus when it is no larger than the sample: the histogram is exact, step 2 is skipped)
//   2. lsh_scan_kernel<0>  every (query, row) pair: xor + popcount; the rare pairs with d <= t_hi count into hist[q][d] and are
//                          appended to the query's list as (d << 32 | row), as far as the list has room
//   3. lsh_threshold_kernel  t = the smallest distance at which the cumulative count reaches c; m = that count.  Three routes:
//                          complete -- every counted pair fitted the list, which therefore holds the m rows up to t;
//                          rescan   -- the list overflowed (or step 2 was skipped) but m fits: the list restarts empty;
//                          flagged  -- t_hi was too small (fewer than c rows counted) or m exceeds the list (ties at t)
//   4. lsh_scan_kernel<1>  the same scan for the `rescan` queries only, appending the m pairs with d <= t (workgroups whose
//                          256 queries are all complete or flagged return at once)
//   5. lsh_select_kernel   sorts the entries with d <= t (bitonic; compacted into LDS up to 4096 of them, else in place) and
//                          emits the first c; a flagged query first takes the exact fallback: full histogram of its distances
//                          -> t, then the rows below t and the lowest-id rows at t (ordered compaction): exactly c entries.
#pragma once
#include "common.hpp"

namespace vdb {

constexpr int kLshMaxBits = 1024;
constexpr int kLshMaxCand = 65536;
constexpr int kLshEncRows = 8;         // rows per wave of the encode kernel
constexpr int kLshQTile = 256;         // queries per workgroup of the scan (their codes sit in LDS)
constexpr int kLshRowTile = 512;       // rows per workgroup of the scan: two per thread, in registers
constexpr int kLshSampleMax = 32768;   // rows of the threshold sample (a multiple of 256)
constexpr int kLshSampleQ = 4;         // queries per workgroup of the sample kernel
constexpr int kLshSortLds = 4096;      // list entries sorted in LDS

// ---- encode ------------------------------------------------------------------------------------------------------------
// One wave = kLshEncRows rows x 64 bits: lane l owns bit 64 * chunk + l and reads its projection row from the transposed
// copy rt[d][nbits] (coalesced); the x values are wave-uniform.  codes rows are zeroed by the caller (padding words).
__global__ __launch_bounds__(256) void lsh_encode_kernel(const float *__restrict__ x, int64_t n, int dim, int64_t pitch,
                                                         const float *__restrict__ rt, int nbits, int wp,
                                                         uint32_t *__restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int chunks = (nbits + 63) >> 6;
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = (item / chunks) * kLshEncRows;
    const int chunk = (int)(item % chunks);
    if (r0 >= n) return;
    const int j = chunk * 64 + lane;
    const bool active = j < nbits;
    const float *xr[kLshEncRows];
#pragma unroll
    for (int i = 0; i < kLshEncRows; ++i) xr[i] = x + (size_t)(r0 + i < n ? r0 + i : n - 1) * pitch;
    double s[kLshEncRows];
#pragma unroll
    for (int i = 0; i < kLshEncRows; ++i) s[i] = 0.0;
    const float *rj = rt + (active ? j : 0);
    for (int d = 0; d < dim; ++d) {
        const double rv = (double)rj[(size_t)d * nbits];
#pragma unroll
        for (int i = 0; i < kLshEncRows; ++i) s[i] = fma((double)xr[i][d], rv, s[i]);
    }
#pragma unroll
    for (int i = 0; i < kLshEncRows; ++i) {
        const unsigned long long mask = __ballot(active && s[i] >= 0.0);
        if (lane == 0 && r0 + i < n) {
            uint32_t *o = codes + (size_t)(r0 + i) * wp + 2 * chunk;
            o[0] = (uint32_t)mask;
            if (2 * chunk + 1 < wp) o[1] = (uint32_t)(mask >> 32);
        }
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------
struct LshArgs {
    const uint32_t *codes;       // [n][wp]
    const uint32_t *qcodes;      // [nq][wp]
    int64_t n, nq;
    int wp, nbits, hb;           // hb = nbits + 1 histogram bins per query
    int c, cap, ncand;           // c = min(ncand, n); cap = list entries per query (a power of two >= c)
    int64_t sample_n, sample_stride;
    int force_fallback;
    int64_t id_base;
    int *hist;                   // [nq][hb]
    int *thi, *tq, *cnt, *flag, *tsel, *msel;  // [nq] each: upper bound, cut for MODE 1 (-1: none), list fill, fallback flag, cut, rows up to it
    int scanned0;                // lsh_scan_kernel<0> ran (the corpus is larger than the sample)
    unsigned long long *list;    // [nq][cap]
    unsigned long long *nflagged;  // flagged queries since the call began
    int32_t *out_ham;            // [nq][ncand]
    int64_t *out_ids;
};

__device__ __forceinline__ int lsh_ham(const uint32_t *__restrict__ a, const uint32_t *b, int wp) {
    int d = 0;
    for (int w = 0; w < wp; ++w) d += __popc(a[w] ^ b[w]);
    return d;
}

// One workgroup per kLshSampleQ queries: every thread keeps a sample row in registers per step and scores it against the
// workgroup's queries (LDS).  The sample is sample_n / 256 runs of 256 consecutive rows, `sample_stride` rows apart (dense
// loads; the same 1 MiB of codes serves every query), or the whole corpus (sample_stride = 256, exact histogram).
template <int WP>
__global__ __launch_bounds__(256) void lsh_sample_kernel(LshArgs a) {
    __shared__ int sh[kLshSampleQ][kLshMaxBits + 1];
    __shared__ uint32_t qc[kLshSampleQ][WP];
    const int64_t q0 = (int64_t)blockIdx.x * kLshSampleQ;
    const int nqt = (int)(a.nq - q0 < kLshSampleQ ? a.nq - q0 : kLshSampleQ);
    const int tid = threadIdx.x;
    for (int i = tid; i < kLshSampleQ * (kLshMaxBits + 1); i += 256) (&sh[0][0])[i] = 0;
    for (int i = tid; i < nqt * WP; i += 256) qc[i / WP][i % WP] = a.qcodes[(size_t)q0 * WP + i];
    __syncthreads();
    for (int64_t base = 0; base < a.sample_n; base += 256) {
        const int64_t r = (base >> 8) * a.sample_stride + tid;
        if (base + tid >= a.sample_n) continue;
        uint32_t x[WP];
#pragma unroll
        for (int w = 0; w < WP; ++w) x[w] = a.codes[(size_t)r * WP + w];
        for (int q = 0; q < nqt; ++q) {
            int d = 0;
#pragma unroll
            for (int w = 0; w < WP; ++w) d += __popc(x[w] ^ qc[q][w]);
            atomicAdd(&sh[q][d], 1);
        }
    }
    __syncthreads();
    const bool exact = a.sample_n == a.n;
    for (int q = 0; q < nqt; ++q) {
        int *hq = a.hist + (size_t)(q0 + q) * a.hb;
        for (int i = tid; i < a.hb; i += 256) hq[i] = exact ? sh[q][i] : 0;
    }
    if (tid < nqt) {
        int t = a.nbits;
        if (!exact) {
            // the expected sample count lambda of the c nearest rows + 5 sqrt(lambda) + 4, never fewer than 16 sample rows: the
            // true cut lies above t only if the sample overstates the tail by five standard deviations of its Poisson count
            // (such a query takes the exact fallback)
            const float lambda = (float)a.c * (float)a.sample_n / (float)a.n;
            const long long want = (long long)ceilf(lambda + 5.f * sqrtf(lambda) + 4.f);
            const long long target = want > 16 ? want : 16;
            long long cum = 0;
            for (int d = 0; d <= a.nbits; ++d) {
                cum += sh[tid][d];
                if (cum >= target) { t = d; break; }
            }
        }
        a.thi[q0 + tid] = t;
        a.cnt[q0 + tid] = 0;
    }
}

// MODE 0: count the pairs with d <= thi[q] into hist AND append them to the query's list (what fits).  MODE 1: append the pairs
// with d <= tq[q]; a workgroup none of whose queries asks for it (tq < 0: their list was complete after MODE 0) returns at once.
template <int MODE, int WP>
__global__ __launch_bounds__(256) void lsh_scan_kernel(LshArgs a) {
    __shared__ __align__(16) uint32_t qc[kLshQTile * WP];
    __shared__ int thr[kLshQTile];
    __shared__ int sel[kLshQTile], nsel;          // MODE 1: the queries of the tile that ask for the rescan
    const int tid = threadIdx.x;
    if (MODE == 1 && tid == 0) nsel = 0;
    const int64_t q0 = (int64_t)blockIdx.y * kLshQTile;
    const int nqt = (int)(a.nq - q0 < kLshQTile ? a.nq - q0 : kLshQTile);
    for (int i = tid; i < nqt * WP; i += 256) qc[i] = a.qcodes[(size_t)q0 * WP + i];
    int mine = -1;
    if (tid < nqt) thr[tid] = mine = (MODE == 0 ? a.thi : a.tq)[q0 + tid];
    if (MODE == 1) {
        if (!__syncthreads_or(mine >= 0)) return;
        if (mine >= 0) sel[atomicAdd(&nsel, 1)] = tid;
    }
    const int64_t ra = (int64_t)blockIdx.x * kLshRowTile + tid, rb = ra + 256;
    const bool va = ra < a.n, vb = rb < a.n;
    uint32_t xa[WP], xb[WP];
#pragma unroll
    for (int w = 0; w < WP; ++w) {
        xa[w] = va ? a.codes[(size_t)ra * WP + w] : 0u;
        xb[w] = vb ? a.codes[(size_t)rb * WP + w] : 0u;
    }
    __syncthreads();
    const int nloop = MODE == 1 ? nsel : nqt;
    for (int qi = 0; qi < nloop; ++qi) {
        const int q = MODE == 1 ? sel[qi] : qi;
        const int t = thr[q];
        if (t < 0) continue;
        int da = 0, db = 0;
#pragma unroll
        for (int w = 0; w < WP; ++w) {
            const uint32_t qw = qc[q * WP + w];
            da += __popc(xa[w] ^ qw);
            db += __popc(xb[w] ^ qw);
        }
        const bool ha = va && da <= t, hb = vb && db <= t;
        if (ha || hb) {
            const int64_t gq = q0 + q;
            if (MODE == 0) {
                if (ha) atomicAdd(&a.hist[(size_t)gq * a.hb + da], 1);
                if (hb) atomicAdd(&a.hist[(size_t)gq * a.hb + db], 1);
            }
            {
                if (ha) {
                    const int idx = atomicAdd(&a.cnt[gq], 1);
                    if (idx < a.cap) a.list[(size_t)gq * a.cap + idx] = ((unsigned long long)da << 32) | (unsigned long long)ra;
                }
                if (hb) {
                    const int idx = atomicAdd(&a.cnt[gq], 1);
                    if (idx < a.cap) a.list[(size_t)gq * a.cap + idx] = ((unsigned long long)db << 32) | (unsigned long long)rb;
                }
            }
        }
    }
}

// one thread per query: the cut t, the rows m up to it, and which route the query takes
__global__ __launch_bounds__(256) void lsh_threshold_kernel(LshArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nq) return;
    const int *hq = a.hist + (size_t)q * a.hb;
    const int thi = a.thi[q];
    long long cum = 0, m = 0;
    int t = -1;
    for (int d = 0; d <= thi; ++d) {
        cum += hq[d];
        if (t < 0 && cum >= a.c) { t = d; m = cum; }
    }
    const bool flagged = a.force_fallback || t < 0 || m > a.cap;
    // MODE 0 appended every pair it counted: if they all fitted, the list already holds the m rows up to t (and a few beyond)
    const bool complete = !flagged && a.scanned0 && cum <= a.cap;
    a.flag[q] = flagged ? 1 : 0;
    a.tq[q] = (flagged || complete) ? -1 : t;
    a.tsel[q] = t;
    a.msel[q] = (int)m;
    if (!complete) a.cnt[q] = 0;
    if (flagged) stat_add(a.nflagged, q, 0, 1ull);
}

// one workgroup per query: (flagged: exact fallback ->) sort the list -> emit
__global__ __launch_bounds__(256) void lsh_select_kernel(LshArgs a) {
    __shared__ unsigned long long sbuf[kLshSortLds];
    __shared__ int sh[kLshMaxBits + 1];
    __shared__ uint32_t qc[32];
    __shared__ int s_t, s_below, s_fill, wtot[4];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *lq = a.list + (size_t)q * a.cap;
    int n = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;      // list entries: the m rows up to the cut, and after MODE 0 a few beyond it
    int t_cut = a.tsel[q], m = a.msel[q];
    if (tid == 0) s_fill = 0;
    if (a.flag[q]) {       // (uniform over the workgroup)
        for (int i = tid; i < a.hb; i += 256) sh[i] = 0;
        if (tid < a.wp) qc[tid] = a.qcodes[(size_t)q * a.wp + tid];
        __syncthreads();
        for (int64_t r = tid; r < a.n; r += 256) atomicAdd(&sh[lsh_ham(a.codes + (size_t)r * a.wp, qc, a.wp)], 1);
        __syncthreads();
        if (tid == 0) {
            long long cum = 0;
            int t = a.nbits;
            for (int d = 0; d <= a.nbits; ++d) {
                if (cum + sh[d] >= a.c) { t = d; break; }
                cum += sh[d];
            }
            s_t = t;
            s_below = (int)cum;
        }
        __syncthreads();
        const int t = s_t, below = s_below, need = a.c - below;
        int taken = 0;          // rows at distance t seen so far (uniform)
        for (int64_t base = 0; base < a.n; base += 256) {
            const int64_t r = base + tid;
            const int d = r < a.n ? lsh_ham(a.codes + (size_t)r * a.wp, qc, a.wp) : 0x7fffffff;
            if (d < t) lq[atomicAdd(&s_fill, 1)] = ((unsigned long long)d << 32) | (unsigned long long)r;
            const bool tie = d == t;
            const unsigned long long mask = __ballot(tie);
            if (lane == 0) wtot[wave] = __popcll(mask);
            __syncthreads();
            int pos = taken + __popcll(mask & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) pos += wtot[w];
            if (tie && pos < need) lq[below + pos] = ((unsigned long long)d << 32) | (unsigned long long)r;
            taken += wtot[0] + wtot[1] + wtot[2] + wtot[3];
            __syncthreads();
        }
        n = m = a.c;
        t_cut = 0x7fffffff;
        __syncthreads();
        if (tid == 0) s_fill = 0;
    }
    __syncthreads();
    // the m entries with d <= t_cut: compacted into LDS when they fit, else sorted in place with the others blanked
    int P = 1;
    unsigned long long *buf = lq;
    if (m <= kLshSortLds) {
        buf = sbuf;
        while (P < m) P <<= 1;
        for (int i = tid; i < n; i += 256) {
            const unsigned long long key = lq[i];
            if ((int)(key >> 32) <= t_cut) buf[atomicAdd(&s_fill, 1)] = key;
        }
        for (int i = m + tid; i < P; i += 256) buf[i] = ~0ull;
    } else {
        while (P < n) P <<= 1;
        for (int i = tid; i < P; i += 256)
            if (i >= n || (int)(lq[i] >> 32) > t_cut) buf[i] = ~0ull;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = buf[i], y = buf[ixj];
                    if ((x > y) == ((i & k) == 0)) {
                        buf[i] = y;
                        buf[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    int32_t *oh = a.out_ham + (size_t)q * a.ncand;
    int64_t *oi = a.out_ids + (size_t)q * a.ncand;
    for (int i = tid; i < a.ncand; i += 256) {
        if (i < a.c) {
            const unsigned long long key = buf[i];
            oh[i] = (int32_t)(key >> 32);
            oi[i] = a.id_base + (int64_t)(key & 0xffffffffull);
        } else {
            oh[i] = 0x7fffffff;
            oi[i] = -1;
        }
    }
}

}  // namespace vdb

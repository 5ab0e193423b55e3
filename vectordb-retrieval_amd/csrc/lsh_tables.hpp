// lsh_tables.hpp -- hash-table LSH: table keys, collision-vote scan, top-c select (gfx950 only).  Host side: lsh_tables.inc.
//
// Contract (include/vdbhip.h): T tables of H projections each; s[t][h](x) is the float64 chain of lsh.hpp.  Mode 0 ("sign")
// packs the bits s >= 0 of a table into ceil(H / 32) words; mode 1 ("E2") keeps one int32 code floor((s + b) / w) per projection.
// A row collides with a query in table t iff all words of that table are equal; votes = number of such tables, first = the
// smallest of them.  The candidates of a query are its colliding rows under (class, row), class = (T - votes) T + first, the
// first min(ncand, their number) of them: Counter.most_common() over buckets that hold ids in insertion order.
//
// Keys: `wp` uint32 words per table and row, wp = the contract's words per table rounded up to one of {1, 2, 3, 4, 6, 8, 12, 16}
// (LSHT_DISPATCH), the words past them zero in rows and queries alike (equal: they decide no collision).  T wp <= 168.
//
// Select: the scheme of lsh.hpp over the class instead of the Hamming distance, hb = T * T classes, with two differences:
// a pair with no vote has no class and is dropped at once, so a query has c = min(ncand, colliding rows) candidates, found per
// query -- when the bound is the largest class every colliding row was counted, and a query with fewer than ncand of them is
// complete with c = that count, its tail padding.
//   1. lsht_sample_kernel     class histogram of the row sample -> t_hi (the whole corpus when it is no larger: exact, no step 2)
//   2. lsht_scan_kernel<0>    every (query, row) pair: votes and first over the tables; pairs with class <= t_hi count into
//                             hist[q][class] and are appended as (class << 32 | row), as far as the list has room
//   3. lsht_threshold_kernel  c, the cut class t, the rows m up to it; complete / rescan / flagged as in lsh.hpp
//   4. lsht_scan_kernel<1>    the rescan queries only, appending the pairs with class <= t
//   5. lsht_select_kernel     (flagged: exact fallback ->) sort the entries up to t by (class, row), emit the first c as
//                             (votes, id); a query with c = 0 enters the list of empty queries (the brute-force fallback of
//                             the search runs from that list and its count, both on the device)
#pragma once
#include "common.hpp"
#include "lsh.hpp"

namespace vdb {

constexpr int kLshtMaxTables = 32;     // T: T * T classes <= kLshMaxBits
constexpr int kLshtMaxWords = 128;     // T * (words per table of the contract)
constexpr int kLshtLdsWords = 8192;    // query keys of one scan tile (32 KiB of LDS): the tile is min(256, 8192 / (T wp)) queries
constexpr int kLshtRowTile = 256;      // rows per workgroup of the scan: one per thread, its T wp key words in registers

// ---- keys --------------------------------------------------------------------------------------------------------------
struct LshtKeyArgs {
    const float *x;        // [n] rows, `pitch` floats apart
    int64_t n, pitch;
    int dim;
    const float *pt;       // projections transposed [dim][T * H]
    const float *off;      // mode 1: offsets [T * H]
    int T, H, mode, wp, kw;   // kw = T * wp words per row
    double w;              // mode 1: bucket width
    uint32_t *keys;        // [n][kw], zeroed by the caller (padding words, unused bits)
};

__device__ __forceinline__ int32_t lsht_e2_code(double s, double b, double w) {
    const double f = floor((s + b) / w);
    if (!(f == f)) return (int32_t)0x80000000;
    if (f >= 2147483647.0) return 0x7fffffff;
    if (f <= -2147483648.0) return (int32_t)0x80000000;
    return (int32_t)f;
}

// One wave = kLshEncRows rows x one chunk of projections, the chains of lsh_encode_kernel.  Mode 0: a chunk is a table, lane l
// owns its bit l and the wave's ballot is the table's key.  Mode 1: a chunk is 64 consecutive projections j = t H + h, each
// lane stores the code of its own.
__global__ __launch_bounds__(256) void lsht_key_kernel(LshtKeyArgs a) {
    const int lane = threadIdx.x & 63;
    const int TH = a.T * a.H;
    const int chunks = a.mode == 0 ? a.T : (TH + 63) >> 6;
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = (item / chunks) * kLshEncRows;
    const int chunk = (int)(item % chunks);
    if (r0 >= a.n) return;
    const int j = a.mode == 0 ? chunk * a.H + lane : chunk * 64 + lane;
    const bool active = a.mode == 0 ? lane < a.H : j < TH;
    const float *xr[kLshEncRows];
#pragma unroll
    for (int i = 0; i < kLshEncRows; ++i) xr[i] = a.x + (size_t)(r0 + i < a.n ? r0 + i : a.n - 1) * a.pitch;
    double s[kLshEncRows];
#pragma unroll
    for (int i = 0; i < kLshEncRows; ++i) s[i] = 0.0;
    const float *pj = a.pt + (active ? j : 0);
    for (int d = 0; d < a.dim; ++d) {
        const double pv = (double)pj[(size_t)d * TH];
#pragma unroll
        for (int i = 0; i < kLshEncRows; ++i) s[i] = fma((double)xr[i][d], pv, s[i]);
    }
    if (a.mode == 0) {
#pragma unroll
        for (int i = 0; i < kLshEncRows; ++i) {
            const unsigned long long mask = __ballot(active && s[i] >= 0.0);
            if (lane == 0 && r0 + i < a.n) {
                uint32_t *o = a.keys + (size_t)(r0 + i) * a.kw + (size_t)chunk * a.wp;
                o[0] = (uint32_t)mask;
                if (a.H > 32) o[1] = (uint32_t)(mask >> 32);
            }
        }
    } else if (active) {
        const int t = j / a.H, hh = j - t * a.H;
        const double b = (double)a.off[j];
#pragma unroll
        for (int i = 0; i < kLshEncRows; ++i)
            if (r0 + i < a.n) a.keys[(size_t)(r0 + i) * a.kw + (size_t)t * a.wp + hh] = (uint32_t)lsht_e2_code(s[i], b, a.w);
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------
struct LshtArgs {
    const uint32_t *keys;        // [n][kw]
    const uint32_t *qkeys;       // [nq][kw]
    int64_t n, nq, q_base;       // q_base: number of the chunk's first query within the call's batch (empty_list holds q_base + q)
    int T, wp, kw, hb;           // hb = T * T classes per query
    int ncand, cap, qtile;       // cap = list entries per query (a power of two); qtile = queries per scan workgroup
    int64_t sample_n, sample_stride;
    int force_fallback;
    int64_t id_base;
    int *hist;                   // [nq][hb]
    int *thi, *tq, *cnt, *flag, *tsel, *msel, *csel;   // [nq] each, as LshArgs; csel = candidates of the query
    int scanned0;
    unsigned long long *list;    // [nq][cap]
    unsigned long long *stat;    // sharded counters: 0 flagged queries, 1 candidates, 2 empty queries listed
    int32_t *empty_list, *empty_count;    // (null: the call lists no empty queries)
    int32_t *out_votes;          // [nq][ncand]
    int64_t *out_ids;
};

// class of a (row, query) pair, -1 without a vote: the row's words in registers, the query's in LDS (wave-uniform reads)
template <int WP, int TMAX>
__device__ __forceinline__ int lsht_class(const uint32_t (&x)[WP * TMAX], const uint32_t *q, int T) {
    int votes = 0, first = 0;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        if (t < T) {
            uint32_t diff = 0;
#pragma unroll
            for (int w = 0; w < WP; ++w) diff |= x[t * WP + w] ^ q[t * WP + w];
            if (diff == 0) {
                if (votes == 0) first = t;
                ++votes;
            }
        }
    }
    return votes ? (T - votes) * T + first : -1;
}

// the same from memory (the exact fallback of the select)
__device__ __forceinline__ int lsht_class_mem(const uint32_t *__restrict__ row, const uint32_t *q, int T, int wp) {
    int votes = 0, first = 0;
    for (int t = 0; t < T; ++t) {
        uint32_t diff = 0;
        for (int w = 0; w < wp; ++w) diff |= row[t * wp + w] ^ q[t * wp + w];
        if (diff == 0) {
            if (votes == 0) first = t;
            ++votes;
        }
    }
    return votes ? (T - votes) * T + first : -1;
}

// lsh_sample_kernel over classes.  The bound: the class at which the sample holds lambda + 5 sqrt(lambda) + 4 colliding rows
// (lambda = the sample's share of min(ncand, n) rows), never fewer than 16; a sample with fewer has the largest class as its
// bound, under which the scan counts every colliding row.
template <int WP, int TMAX>
__global__ __launch_bounds__(256) void lsht_sample_kernel(LshtArgs a) {
    __shared__ int sh[kLshSampleQ][kLshMaxBits];
    __shared__ uint32_t qc[kLshSampleQ][WP * TMAX];
    const int64_t q0 = (int64_t)blockIdx.x * kLshSampleQ;
    const int nqt = (int)(a.nq - q0 < kLshSampleQ ? a.nq - q0 : kLshSampleQ);
    const int tid = threadIdx.x;
    for (int i = tid; i < kLshSampleQ * kLshMaxBits; i += 256) (&sh[0][0])[i] = 0;
    for (int i = tid; i < nqt * a.kw; i += 256) qc[i / a.kw][i % a.kw] = a.qkeys[(size_t)q0 * a.kw + i];
    __syncthreads();
    for (int64_t base = 0; base < a.sample_n; base += 256) {
        const int64_t r = (base >> 8) * a.sample_stride + tid;
        if (base + tid >= a.sample_n) continue;
        uint32_t x[WP * TMAX];
#pragma unroll
        for (int i = 0; i < WP * TMAX; ++i) x[i] = i < a.kw ? a.keys[(size_t)r * a.kw + i] : 0u;
        for (int q = 0; q < nqt; ++q) {
            const int cl = lsht_class<WP, TMAX>(x, qc[q], a.T);
            if (cl >= 0) atomicAdd(&sh[q][cl], 1);
        }
    }
    __syncthreads();
    const bool exact = a.sample_n == a.n;
    for (int q = 0; q < nqt; ++q) {
        int *hq = a.hist + (size_t)(q0 + q) * a.hb;
        for (int i = tid; i < a.hb; i += 256) hq[i] = exact ? sh[q][i] : 0;
    }
    if (tid < nqt) {
        int t = a.hb - 1;
        if (!exact) {
            const float c = (float)(a.ncand < a.n ? (int64_t)a.ncand : a.n);
            const float lambda = c * (float)a.sample_n / (float)a.n;
            const long long want = (long long)ceilf(lambda + 5.f * sqrtf(lambda) + 4.f);
            const long long target = want > 16 ? want : 16;
            long long cum = 0;
            for (int d = 0; d < a.hb; ++d) {
                cum += sh[tid][d];
                if (cum >= target) { t = d; break; }
            }
        }
        a.thi[q0 + tid] = t;
        a.cnt[q0 + tid] = 0;
    }
}

// MODE 0 / MODE 1 as lsh_scan_kernel: one row per thread, a tile of a.qtile queries per workgroup
template <int MODE, int WP, int TMAX>
__global__ __launch_bounds__(256) void lsht_scan_kernel(LshtArgs a) {
    __shared__ __align__(16) uint32_t qc[kLshtLdsWords];
    __shared__ int thr[256];
    __shared__ int sel[256], nsel;
    const int tid = threadIdx.x;
    if (MODE == 1 && tid == 0) nsel = 0;
    const int64_t q0 = (int64_t)blockIdx.y * a.qtile;
    const int nqt = (int)(a.nq - q0 < a.qtile ? a.nq - q0 : a.qtile);
    for (int i = tid; i < nqt * a.kw; i += 256) qc[i] = a.qkeys[(size_t)q0 * a.kw + i];
    int mine = -1;
    if (tid < nqt) thr[tid] = mine = (MODE == 0 ? a.thi : a.tq)[q0 + tid];
    if (MODE == 1) {
        if (!__syncthreads_or(mine >= 0)) return;
        if (mine >= 0) sel[atomicAdd(&nsel, 1)] = tid;
    }
    const int64_t r = (int64_t)blockIdx.x * kLshtRowTile + tid;
    const bool valid = r < a.n;
    uint32_t x[WP * TMAX];
#pragma unroll
    for (int i = 0; i < WP * TMAX; ++i) x[i] = (valid && i < a.kw) ? a.keys[(size_t)r * a.kw + i] : 0u;
    __syncthreads();
    const int nloop = MODE == 1 ? nsel : nqt;
    for (int qi = 0; qi < nloop; ++qi) {
        const int q = MODE == 1 ? sel[qi] : qi;
        const int t = thr[q];
        if (t < 0) continue;
        const int cl = lsht_class<WP, TMAX>(x, qc + q * a.kw, a.T);
        if (valid && cl >= 0 && cl <= t) {
            const int64_t gq = q0 + q;
            if (MODE == 0) atomicAdd(&a.hist[(size_t)gq * a.hb + cl], 1);
            const int idx = atomicAdd(&a.cnt[gq], 1);
            if (idx < a.cap) a.list[(size_t)gq * a.cap + idx] = ((unsigned long long)cl << 32) | (unsigned long long)r;
        }
    }
}

// one thread per query: its candidates c, the cut t, the rows m up to it, and which route the query takes
__global__ __launch_bounds__(256) void lsht_threshold_kernel(LshtArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nq) return;
    const int *hq = a.hist + (size_t)q * a.hb;
    const int thi = a.thi[q];
    long long cum = 0, m = 0;
    int t = -1, c = a.ncand;
    for (int d = 0; d <= thi; ++d) {
        cum += hq[d];
        if (t < 0 && cum >= a.ncand) { t = d; m = cum; }
    }
    bool flagged = a.force_fallback != 0;
    if (t < 0) {
        if (thi == a.hb - 1) {         // every colliding row was counted and they are fewer than ncand: all of them
            t = thi;
            m = cum;
            c = (int)cum;
        } else {
            flagged = true;
        }
    }
    if (m > a.cap) flagged = true;
    const bool complete = !flagged && a.scanned0 && cum <= a.cap;
    a.flag[q] = flagged ? 1 : 0;
    a.tq[q] = (flagged || complete) ? -1 : t;
    a.tsel[q] = t;
    a.msel[q] = (int)m;
    a.csel[q] = c;
    if (!complete) a.cnt[q] = 0;
    if (flagged) stat_add(a.stat, q, 0, 1ull);
}

// one workgroup per query: (flagged: exact fallback ->) sort the list -> emit
__global__ __launch_bounds__(256) void lsht_select_kernel(LshtArgs a) {
    __shared__ unsigned long long sbuf[kLshSortLds];
    __shared__ int sh[kLshMaxBits];
    __shared__ uint32_t qc[kLshtMaxWords + 64];
    __shared__ int s_t, s_below, s_c, s_fill, wtot[4];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *lq = a.list + (size_t)q * a.cap;
    int n = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;
    int t_cut = a.tsel[q], m = a.msel[q], c = a.csel[q];
    if (tid == 0) s_fill = 0;
    if (a.flag[q]) {       // (uniform over the workgroup)
        for (int i = tid; i < a.hb; i += 256) sh[i] = 0;
        if (tid < a.kw) qc[tid] = a.qkeys[(size_t)q * a.kw + tid];
        __syncthreads();
        for (int64_t r = tid; r < a.n; r += 256) {
            const int cl = lsht_class_mem(a.keys + (size_t)r * a.kw, qc, a.T, a.wp);
            if (cl >= 0) atomicAdd(&sh[cl], 1);
        }
        __syncthreads();
        if (tid == 0) {
            long long total = 0;
            for (int d = 0; d < a.hb; ++d) total += sh[d];
            const int cc = (int)(total < a.ncand ? total : (long long)a.ncand);
            long long cum = 0;
            int t = a.hb - 1;
            for (int d = 0; d < a.hb; ++d) {
                if (cum + sh[d] >= cc) { t = d; break; }
                cum += sh[d];
            }
            s_t = t;
            s_below = (int)cum;
            s_c = cc;
        }
        __syncthreads();
        c = s_c;
        const int t = s_t, below = s_below, need = c - below;
        int taken = 0;          // rows of class t seen so far (uniform)
        for (int64_t base = 0; base < a.n; base += 256) {
            const int64_t r = base + tid;
            int d = 0x7fffffff;
            if (r < a.n) {
                const int cl = lsht_class_mem(a.keys + (size_t)r * a.kw, qc, a.T, a.wp);
                if (cl >= 0) d = cl;
            }
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
        n = m = c;
        t_cut = 0x7fffffff;
        __syncthreads();
        if (tid == 0) s_fill = 0;
    }
    __syncthreads();
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
    int32_t *ov = a.out_votes + (size_t)q * a.ncand;
    int64_t *oi = a.out_ids + (size_t)q * a.ncand;
    for (int i = tid; i < a.ncand; i += 256) {
        if (i < c) {
            const unsigned long long key = buf[i];
            ov[i] = a.T - (int32_t)(key >> 32) / a.T;
            oi[i] = a.id_base + (int64_t)(key & 0xffffffffull);
        } else {
            ov[i] = 0;
            oi[i] = -1;
        }
    }
    if (tid == 0) {
        stat_add(a.stat, q, 1, (unsigned long long)c);
        if (c == 0 && a.empty_list) {
            a.empty_list[atomicAdd(a.empty_count, 1)] = (int32_t)(a.q_base + q);
            stat_add(a.stat, q, 2, 1ull);
        }
    }
}

}  // namespace vdb

// lsh_tables.hpp -- hash-table LSH: table keys, and the vote sample and scan of the counting select (gfx950 only).  Host side: lsh_tables.inc.
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
// Select: lsh_select.hpp with the class as the score: hb = T * T bins, a pair with no vote has no score, and a query wants
// ncand candidates but has only its colliding rows, emitted as (votes, id); a query with none enters the list of empty
// queries (the brute-force fallback of the search runs from that list and its count, both on the device).  This file has the
// sample and the scan, which keep the T wp key words of one row per thread in registers.
#pragma once
#include "common.hpp"
#include "lsh.hpp"

namespace vdb {

constexpr int kLshtMaxTables = 32;     // T: T * T classes <= kLshMaxBits
constexpr int kLshtRowTile = 256;      // rows per workgroup of the scan: one per thread, its T wp key words in registers
constexpr int kLshtLdsWords = 8192;    // query keys of one scan tile (32 KiB of LDS): the tile is min(256, 8192 / (T wp)) queries

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

// ---- sample and scan of the select (lsh_select.hpp) -------------------------------------------------------------------
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

// lsh_sample_kernel over classes.  The bound: the class at which the sample holds lambda + 5 sqrt(lambda) + 4 colliding rows
// (lambda = the sample's share of min(ncand, n) rows), never fewer than 16; a sample with fewer has the largest class as its
// bound, under which the scan counts every colliding row.
template <int WP, int TMAX>
__global__ __launch_bounds__(256) void lsht_sample_kernel(LshSelArgs a) {
    __shared__ int sh[kLshSampleQ][kLshMaxBits];
    __shared__ uint32_t qc[kLshSampleQ][WP * TMAX];
    const int64_t q0 = (int64_t)blockIdx.x * kLshSampleQ;
    const int nqt = (int)(a.nq - q0 < kLshSampleQ ? a.nq - q0 : kLshSampleQ);
    const int tid = threadIdx.x;
    for (int i = tid; i < kLshSampleQ * kLshMaxBits; i += 256) (&sh[0][0])[i] = 0;
    for (int i = tid; i < nqt * a.kw; i += 256) qc[i / a.kw][i % a.kw] = a.qcodes[(size_t)q0 * a.kw + i];
    __syncthreads();
    for (int64_t base = 0; base < a.sample_n; base += 256) {
        const int64_t r = (base >> 8) * a.sample_stride + tid;
        if (base + tid >= a.sample_n) continue;
        uint32_t x[WP * TMAX];
#pragma unroll
        for (int i = 0; i < WP * TMAX; ++i) x[i] = i < a.kw ? a.codes[(size_t)r * a.kw + i] : 0u;
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
__global__ __launch_bounds__(256) void lsht_scan_kernel(LshSelArgs a) {
    __shared__ __align__(16) uint32_t qc[kLshtLdsWords];
    __shared__ int thr[256];
    __shared__ int sel[256], nsel;
    const int tid = threadIdx.x;
    if (MODE == 1 && tid == 0) nsel = 0;
    const int64_t q0 = (int64_t)blockIdx.y * a.qtile;
    const int nqt = (int)(a.nq - q0 < a.qtile ? a.nq - q0 : a.qtile);
    for (int i = tid; i < nqt * a.kw; i += 256) qc[i] = a.qcodes[(size_t)q0 * a.kw + i];
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
    for (int i = 0; i < WP * TMAX; ++i) x[i] = (valid && i < a.kw) ? a.codes[(size_t)r * a.kw + i] : 0u;
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

}  // namespace vdb

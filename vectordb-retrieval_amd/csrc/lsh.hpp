// lsh.hpp -- sign-LSH codes: encode, and the Hamming sample and scan of the counting select (gfx950 only).  Host side: lsh.inc.
//
// Contract (include/vdbhip.h): bit j of a vector x is  s_j >= 0  with  s_j = sum_d (double)x[d] * (double)R[j][d], accumulated
// from 0.0 with d ascending and one rounding per step; the candidates of a query are the min(ncand, ntotal) rows smallest
// under (Hamming distance, row), in that order.
//
// Codes: `wp` uint32 words per row, wp = nbits / 32 rounded up to a power of two, the words past nbits / 32 zero in rows
// and queries alike (they add nothing to a distance), so the scan is compiled for wp in {1, 2, 4, 8, 16, 32} only.
//
// Select: lsh_select.hpp with the Hamming distance as the score: hb = nbits + 1 bins, every pair has a score, and a query
// wants min(ncand, n) candidates, emitted as (distance, id).  This file has the sample and the scan, which keep the code
// words of two rows per thread in registers.
#pragma once
#include "common.hpp"
#include "lsh_select.hpp"

namespace vdb {

constexpr int kLshEncRows = 8;         // rows per wave of the encode kernel
constexpr int kLshQTile = 256;         // queries per workgroup of the scan (their codes sit in LDS)
constexpr int kLshRowTile = 512;       // rows per workgroup of the scan: two per thread, in registers

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

// ---- sample and scan of the select (lsh_select.hpp) -------------------------------------------------------------------
// Step 1 of lsh_select.hpp.  One workgroup per kLshSampleQ queries: every thread keeps a sample row in registers per step and scores it against the
// workgroup's queries (LDS).  The sample is sample_n / 256 runs of 256 consecutive rows, `sample_stride` rows apart (dense
// loads; the same 1 MiB of codes serves every query), or the whole corpus (sample_stride = 256, exact histogram).
template <int WP>
__global__ __launch_bounds__(256) void lsh_sample_kernel(LshSelArgs a) {
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
        int t = a.hb - 1;
        if (!exact) {
            // the expected sample count lambda of the c nearest rows + 5 sqrt(lambda) + 4, never fewer than 16 sample rows: the
            // true cut lies above t only if the sample overstates the tail by five standard deviations of its Poisson count
            // (such a query takes the exact fallback)
            const float lambda = (float)a.want * (float)a.sample_n / (float)a.n;
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

// MODE 0: count the pairs with d <= thi[q] into hist AND append them to the query's list (what fits).  MODE 1: append the pairs
// with d <= tq[q]; a workgroup none of whose queries asks for it (tq < 0: their list was complete after MODE 0) returns at once.
template <int MODE, int WP>
__global__ __launch_bounds__(256) void lsh_scan_kernel(LshSelArgs a) {
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

}  // namespace vdb

// range.hpp -- kernels of the range search (vdb_range_search; host side: range.inc; sizes: range_plan.hpp).
//
// A range search answers "every row within `radius`" exactly, in ascending id, without a sort:
//   prefilter   an fp16 MFMA scan of the resident panels sets bit (query, row) of a candidate bitmap wherever the scan score is
//               <= thr[q] = cs (radius - ||q||^2) + eps[q] (L2) or cs (-radius) + eps[q] (IP): a superset of the answer, by the
//               bound of the top-k guard (prep.hpp, query_eps_body).  The MFMA sequences, bias initialisation and pad-row handling
//               are those of debug_scores_x16_kernel / debug_scores16_kernel (debug_ivf.inc), i.e. of the scans themselves
//   filter      every set bit is re-scored with row_key (refine.hpp) and cleared unless the float32 comparison of the contract
//               passes; survivors are counted per (query, 2048-row segment)
//   prefix      exclusive sums over segments and queries give lims and every segment's write offset
//   emit        the survivors' keys are computed once more and (D, I) written in bit order = ascending id
// A lane of the C/D layout of v_mfma_f32_16x16x32_f16 holds one query (lane & 15) and, over the tiles of a span, CONSECUTIVE
// corpus rows (128 per 512-row span in layout "x16", 256 per 1024-row span in p16): whole bitmap words, built in registers and
// stored without atomics ("x16": 16 bytes at a time).
#pragma once
#include "common.hpp"
#include "prep.hpp"
#include "range_plan.hpp"
#include "refine.hpp"
#include "scan16.hpp"

namespace vdb {

typedef unsigned range_uint4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned range_mask_dev(int64_t w, int64_t N) {        // range_word_mask (range_plan.hpp) on the device
    const int64_t left = N - w * kRangeWordBits;
    return left >= kRangeWordBits ? 0xffffffffu : left <= 0 ? 0u : ((1u << (int)left) - 1u);
}

// ---- per-query threshold in scan units ---------------------------------------------------------------------------------------
// thr[q] >= cs (radius - ||q||^2) + eps[q] (L2) / cs (-radius) + eps[q] (IP), formed in float64 and rounded UP to float32.  The
// allowance: cs is a power of two times sx and radius a float32, so cs * radius is exact in float64; ||q||^2 is a
// chain of D fma steps over non-negative terms, relative error <= D 2^-53; the subtraction and the two additions add one rounding
// each.  (D + 4) 2^-52 (|radius| + ||q||^2) cs covers all of it with a factor two to spare, and one 2^-52 relative step on the sum
// covers the additions of eps and of the allowance itself.
// flag[q]: 0 scan with thr[q] | 1 every row is a candidate (a threshold that is not finite, a batch whose scales are unusable, a
// bound that hit its cap) | thr = -FLT_MAX with flag 0: no row can pass (L2 radius <= 0, IP radius = +inf)
struct RangeThrArgs {
    const float *Q;          // [nq][D]
    int64_t nq;
    int D;
    int metric;
    float radius;
    const QueryBatchInfo *info;
    const float *eps;        // [nq]
    float *thr;              // [nq]
    int *flag;               // [nq]
    unsigned long long *stat;    // sharded counters: [1] += fallback queries
};

__global__ __launch_bounds__(256) void range_thr_kernel(RangeThrArgs a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nq) return;
    const bool none = a.metric == 0 ? !(a.radius > 0.f) : a.radius == __builtin_inff();
    float thr = -3.402823466e+38f;
    int all = 0;
    if (!none) {
        const double cs = (double)a.info->cs, r = (double)a.radius, e = (double)a.eps[q];
        double t, allow = 0.0;
        if (a.metric == 0) {
            double n2 = 0.0;
            const float *row = a.Q + (size_t)q * a.D;
            for (int d = 0; d < a.D; ++d) n2 = fma((double)row[d], (double)row[d], n2);
            t = cs * (r - n2);
            allow = cs * (double)(a.D + 4) * ldexp(1.0, -52) * (fabs(r) + n2);
        } else {
            t = cs * (-r);
        }
        t = t + e + allow;
        t += fabs(t) * ldexp(1.0, -52);
        float tf = (float)t;
        if ((double)tf < t) tf = nextafterf(tf, __builtin_inff());
        all = a.info->force_fallback || !(fabsf(tf) <= 3.402823466e+38f) || !(e < 1.0e36);
        thr = tf;
    }
    a.thr[q] = thr;
    a.flag[q] = all;
    if (all) stat_add(a.stat, q, 1, 1ull);
}

// ---- prefilter scans ---------------------------------------------------------------------------------------------------------
// Workgroup = 4 waves = kRangeQueryTile queries (each wave two blocks of 16) x ONE span of rows: the four waves read the same A
// fragments, which the vector cache serves after the first.  Every (query < nq, word of the span) is written, so the bitmap needs
// no clearing; spans past the panels (a bitmap row is padded to 1024 rows, "x16" panels to 512) get zeros.  Rows >= N are masked
// by row number, never by the bias: with radius = FLT_MAX the threshold passes kPadBias.
struct RangeScanArgs {
    const half8 *panels;
    const float *bias;
    const half8 *qpanels;    // B fragments of the slab's queries, [q / 16][32-dim k-step][lane]
    const QueryBatchInfo *info;
    const float *thr;        // [nq] of the slab
    const int *flag;
    int64_t nq, N, nspans, W;
    unsigned *bitmap;        // [nq][W]
};

// layout "x16" (D <= 128): accumulator register i of lane l, tile t, row block rb: query 16 qb + (l & 15), corpus row
// 512 s + 128 (l >> 4) + 8 t + 4 rb + i  ->  bit 8 (t & 3) + 4 rb + i of the lane's word t >> 2
template <int KS2>
__global__ __launch_bounds__(256) void range_scan_x16_kernel(RangeScanArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int64_t span = blockIdx.x;
    const int64_t qb0 = ((int64_t)blockIdx.y * 4 + wave) * 2;
    if (qb0 * 16 >= a.nq) return;
    const float cs = a.info->cs;
    half8 bf[2][KS2];
    float th[2];
    int64_t q[2];
    bool all[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        q[c] = (qb0 + c) * 16 + (lane & 15);
        const bool live = q[c] < a.nq;
        th[c] = live ? a.thr[q[c]] : -3.402823466e+38f;
        all[c] = live && a.flag[q[c]] != 0;
#pragma unroll
        for (int ks2 = 0; ks2 < KS2; ++ks2) bf[c][ks2] = a.qpanels[((size_t)(qb0 + c) * KS2 + ks2) * 64 + lane];
    }
    unsigned w[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if (span < a.nspans) {
#pragma unroll
        for (int t = 0; t < kTilesPerSpan; ++t) {
            const int64_t tile = span * kTilesPerSpan + t;
            half8 af[2][KS2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int ks2 = 0; ks2 < KS2; ++ks2) af[rb][ks2] = a.panels[((size_t)tile * 2 * KS2 + 2 * ks2 + rb) * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const int64_t rbase = span * kSpanRows + (int64_t)g * 128 + 8 * t + 4 * rb;
                const float4 bv = *reinterpret_cast<const float4 *>(a.bias + rbase);
                float4v init;
                init[0] = (bv.x >= 0.9e38f) ? kPadBias : bv.x * cs;
                init[1] = (bv.y >= 0.9e38f) ? kPadBias : bv.y * cs;
                init[2] = (bv.z >= 0.9e38f) ? kPadBias : bv.z * cs;
                init[3] = (bv.w >= 0.9e38f) ? kPadBias : bv.w * cs;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    float4v acc = init;
#pragma unroll
                    for (int ks2 = 0; ks2 < KS2; ++ks2) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb][ks2], bf[c][ks2], acc, 0, 0, 0);
                    const unsigned bits = (acc[0] <= th[c] ? 1u : 0u) | (acc[1] <= th[c] ? 2u : 0u) | (acc[2] <= th[c] ? 4u : 0u) |
                                          (acc[3] <= th[c] ? 8u : 0u);
                    w[c][t >> 2] |= bits << (8 * (t & 3) + 4 * rb);
                }
            }
        }
    }
    const int64_t wbase = span * (kSpanRows / kRangeWordBits) + g * 4;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (q[c] >= a.nq) continue;
        range_uint4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (all[c] ? 0xffffffffu : w[c][j]) & range_mask_dev(wbase + j, a.N);
        *reinterpret_cast<range_uint4 *>(a.bitmap + (size_t)q[c] * a.W + wbase) = o;
    }
}

// layout p16 (D > 128, KS 32-dim k-steps): accumulator register i of lane l, tile t: query 16 qb + (l & 15), corpus row
// 1024 s + 256 (l >> 4) + 4 t + i  ->  bit 4 (t & 7) + i of the lane's word t >> 3.  A wave takes 8 tiles (one word) x its two
// query blocks per pass over the k-steps: 10 fragment loads per 16 MFMAs.
__global__ __launch_bounds__(256) void range_scan_p16_kernel(RangeScanArgs a, int KS) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int64_t span = blockIdx.x;
    const int64_t qb0 = ((int64_t)blockIdx.y * 4 + wave) * 2;
    if (qb0 * 16 >= a.nq) return;
    const float cs = a.info->cs;
    float th[2];
    int64_t q[2];
    bool all[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        q[c] = (qb0 + c) * 16 + (lane & 15);
        const bool live = q[c] < a.nq;
        th[c] = live ? a.thr[q[c]] : -3.402823466e+38f;
        all[c] = live && a.flag[q[c]] != 0;
    }
    const half8 *b0p = a.qpanels + (size_t)qb0 * KS * 64 + lane, *b1p = a.qpanels + (size_t)(qb0 + 1) * KS * 64 + lane;
#pragma unroll 1
    for (int r = 0; r < kTilesPerSpan16 / 8; ++r) {        // (not unrolled: the 64 accumulator registers of a pass are the budget)
        unsigned w[2] = {0u, 0u};
        if (span < a.nspans) {
            const int t0 = r * 8;
            float4v acc[2][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t rbase = span * kSpanRows16 + (int64_t)g * kBinRows + 4 * (t0 + j);
                const float4 bv = *reinterpret_cast<const float4 *>(a.bias + rbase);
                float4v init;
                init[0] = (bv.x >= 0.9e38f) ? kPadBias : bv.x * cs;
                init[1] = (bv.y >= 0.9e38f) ? kPadBias : bv.y * cs;
                init[2] = (bv.z >= 0.9e38f) ? kPadBias : bv.z * cs;
                init[3] = (bv.w >= 0.9e38f) ? kPadBias : bv.w * cs;
                acc[0][j] = init;
                acc[1][j] = init;
            }
            const half8 *ap = a.panels + ((size_t)(span * kTilesPerSpan16 + t0) * KS) * 64 + lane;
            for (int ks = 0; ks < KS; ++ks) {
                const half8 b0 = b0p[(size_t)ks * 64], b1 = b1p[(size_t)ks * 64];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const half8 af = ap[((size_t)j * KS + ks) * 64];
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, b0, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, b1, acc[1][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned bits = (acc[c][j][0] <= th[c] ? 1u : 0u) | (acc[c][j][1] <= th[c] ? 2u : 0u) |
                                          (acc[c][j][2] <= th[c] ? 4u : 0u) | (acc[c][j][3] <= th[c] ? 8u : 0u);
                    w[c] |= bits << (4 * j);
                }
        }
        const int64_t word = span * (kSpanRows16 / kRangeWordBits) + g * 8 + r;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (q[c] < a.nq) a.bitmap[(size_t)q[c] * a.W + word] = (all[c] ? 0xffffffffu : w[c]) & range_mask_dev(word, a.N);
    }
}

// handles without a resident fp16 copy in those two layouts: every row is a candidate (exact and slow)
__global__ __launch_bounds__(256) void range_fill_kernel(unsigned *bitmap, int64_t nq, int64_t W, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * W) return;
    bitmap[i] = range_mask_dev(i % W, N);
}

// ---- exact filter, prefix, emit ----------------------------------------------------------------------------------------------
struct RangeTailArgs {
    RefineCommon c;          // c.Q: the slab's queries padded to D4
    int64_t nq, W;
    int S;                   // segments per query row
    float radius;
    unsigned *bitmap;        // [nq][W]
    int *seg;                // [nq][S]: survivors per segment (filter), then their exclusive prefix inside the query (prefix)
    int64_t *qtot;           // [nq] survivors per query
    int64_t *lims;           // lims of the slab's first query onward: [0] is given, [1 .. nq] are written
    unsigned long long *stat;    // sharded counters: [0] += candidates scored
    float *D;                // results of the whole call
    int64_t *I;
};

__device__ __forceinline__ bool range_passes(int metric, double key, float radius, float *d) {
    const float v = (float)(metric == 0 ? key : -key);
    *d = v;
    return metric == 0 ? v < radius : v > radius;      // (a NaN key passes neither)
}

// one wave per (query, segment), one bitmap word per lane: a lane scores the rows of its set bits in turn and keeps the survivors
__global__ __launch_bounds__(256) void range_filter_kernel(RangeTailArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= a.nq * a.S) return;
    const int64_t q = unit / a.S;
    const int64_t widx = (unit - q * a.S) * kRangeSegWords + lane;
    unsigned *wp = a.bitmap + (size_t)q * a.W + widx;
    const unsigned word = widx < a.W ? *wp : 0u;
    if (__ballot(word != 0u) == 0ull) {
        if (lane == 0) a.seg[unit] = 0;
        return;
    }
    const float *qptr = a.c.Q + (size_t)q * a.c.D4;
    unsigned keep = 0u;
    for (unsigned m = word; m; m &= m - 1u) {
        const int b = __ffs((int)m) - 1;
        float d;
        if (range_passes(a.c.metric, unsortable_f64(row_key<4>(a.c, widx * kRangeWordBits + b, qptr)), a.radius, &d)) keep |= 1u << b;
    }
    if (keep != word) *wp = keep;
    int cnt = __popc(keep), cand = __popc(word);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        cand += __shfl_xor(cand, o);
    }
    if (lane == 0) {
        a.seg[unit] = cnt;
        stat_add(a.stat, q, 0, (unsigned long long)cand);
    }
}

// one wave per query: exclusive prefix of its segment counts (in place) and the query's total
__global__ __launch_bounds__(256) void range_seg_prefix_kernel(RangeTailArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    int *seg = a.seg + (size_t)q * a.S;
    int64_t run = 0;
    for (int s0 = 0; s0 < a.S; s0 += 64) {
        const int s = s0 + lane;
        const int v = s < a.S ? seg[s] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (s < a.S) seg[s] = (int)run + inc - v;
        run += __shfl(inc, 63);
    }
    if (lane == 0) a.qtot[q] = run;
}

// one workgroup: lims[q + 1] = lims[0] + sum of qtot[0 .. q]
__global__ __launch_bounds__(256) void range_lims_kernel(RangeTailArgs a) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int64_t per = (a.nq + 255) / 256;
    const int64_t q0 = t * per < a.nq ? t * per : a.nq, q1 = q0 + per < a.nq ? q0 + per : a.nq;
    int64_t s = 0;
    for (int64_t q = q0; q < q1; ++q) s += a.qtot[q];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = a.lims[0];
        for (int i = 0; i < 256; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t q = q0; q < q1; ++q) {
        run += a.qtot[q];
        a.lims[q + 1] = run;
    }
}

// the filter's units once more: the survivors of a word are written behind those of the lanes (words) before it
// (IDMAP: the rows are in list order and the id of row r is c.idmap[r] -- ivf_range_emit_kernel, ivf_range.hpp)
template <bool IDMAP>
__device__ __forceinline__ void range_emit_body(const RangeTailArgs &a) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= a.nq * a.S) return;
    const int64_t q = unit / a.S;
    const int64_t widx = (unit - q * a.S) * kRangeSegWords + lane;
    const unsigned word = widx < a.W ? a.bitmap[(size_t)q * a.W + widx] : 0u;
    if (__ballot(word != 0u) == 0ull) return;
    const int n = __popc(word);
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    int64_t out = a.lims[q] + a.seg[unit] + (inc - n);
    const float *qptr = a.c.Q + (size_t)q * a.c.D4;
    for (unsigned m = word; m; m &= m - 1u) {
        const int64_t row = widx * kRangeWordBits + (__ffs((int)m) - 1);
        float d;
        (void)range_passes(a.c.metric, unsortable_f64(row_key<4>(a.c, row, qptr)), a.radius, &d);
        a.D[out] = d;
        a.I[out] = IDMAP ? a.c.idmap[row] : a.c.id_base + row;
        ++out;
    }
}
__global__ __launch_bounds__(256) void range_emit_kernel(RangeTailArgs a) { range_emit_body<false>(a); }

}  // namespace vdb

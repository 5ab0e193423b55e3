// ivf_i8.hpp -- device kernels of IVF-I8 (vdb_ivf_set_codec 3; host side: ivf_i8.inc, rules: ivf_i8_plan.hpp).
//
// An IVF-I8 index keeps a byte-valued corpus as int8 rows x - cx in list order (rows8, the row-major copy the list refine of an
// IVF-Flat index reads) and the int8 copy of the panel space (panels8, bias8, rowstat8): the int8 list scan and the integer
// refine of scan_i8.hpp / refine.hpp serve integer batches from them unchanged.  The build kernels below derive every one of
// those from the int8 ROWS, where ivf_build_panels_i8_kernel / ivf_build_bias_i8_kernel read the float32 rows; the per-batch
// ivf_panels_from_i8_kernel makes the fp16 panels of the same panel space for the batches the int8 scan cannot serve.
#pragma once
#include "common.hpp"
#include "prep.hpp"
#include "scan_i8.hpp"

namespace vdb {

// ---- ingestion: the low bytes of a block of float32 rows, and the block's smallest / largest value -----------------------
// dst[row][pitch]: byte d = (int)x & 0xff for d < D, 0 beyond (one thread per 4-byte word).  That is x - 0 as int8 when the
// corpus takes the s8 window and (x - 128) ^ 0x80 when it takes the u8 one: the window is fixed only after every block has
// been seen (ivf_i8_flip_kernel).  minmax = {min, max} over the block, values clamped to +-1024 first (a NaN counts as
// -1024): they decide the window only when corpus_stats_kernel has found every value a finite integer.
__global__ __launch_bounds__(256) void ivf_i8_ingest_kernel(const float *__restrict__ X, int64_t n, int D, int D4, int pitch,
                                                            unsigned *__restrict__ dst, int *__restrict__ minmax) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = pitch / 4;
    const int64_t row = gid / wpr;
    int lo = 1024, hi = -1024;
    if (row < n) {
        const int w = (int)(gid - row * wpr);
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int d = 4 * w + b;
            if (d < D) {
                const int v = (int)fminf(fmaxf(X[(size_t)row * D4 + d], -1024.f), 1024.f);
                lo = min(lo, v);
                hi = max(hi, v);
                word |= ((unsigned)v & 0xffu) << (8 * b);
            }
        }
        dst[gid] = word;
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0) {      // (plain read first, as the flags of prep.hpp: the extrema settle after a few waves)
        if (lo < *reinterpret_cast<volatile int *>(&minmax[0])) atomicMin(&minmax[0], lo);
        if (hi > *reinterpret_cast<volatile int *>(&minmax[1])) atomicMax(&minmax[1], hi);
    }
}

// every byte ^ 0x80: low byte of x -> int8 of x - 128 (new rows under the u8 window), and int8 of x - cx -> int8 of x - (cx ^ 128)
// (stored rows whose window an append changed); padding bytes go from 0 to -128 and back with it, i.e. stay x = 0
__global__ __launch_bounds__(256) void ivf_i8_flip_kernel(unsigned *__restrict__ p, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) p[i] ^= 0x80808080u;
}

// ---- build: int8 panels over the list-padded panel space, from the int8 rows ----------------------------------------------
// ivf_build_panels_i8_kernel with (int)X[row][d] - cx replaced by the stored byte: the same value.  A lane's 16 dims are 16
// consecutive bytes of its row (one 16-byte load: pitch and d0 are multiples of 16); rows past a span's valid count and dims
// >= D hold A = 0 (the padding bytes of rows8 hold -cx, so they are masked here).
__global__ __launch_bounds__(256) void ivf_i8_build_panels_kernel(const signed char *__restrict__ rows8, int pitch, int D, int ks32,
                                                                  int64_t ntiles, const int32_t *__restrict__ span_row0,
                                                                  const int32_t *__restrict__ span_valid,
                                                                  int4v *__restrict__ panels) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gid & 63);
    const int64_t tk = gid >> 6;
    const int ks = (int)(tk % ks32);
    const int64_t tile = tk / ks32;
    if (tile >= ntiles) return;
    const int rho = lane & 31, kh = lane >> 5;
    const int r = (rho & 3) | ((rho >> 3) << 2), h = (rho >> 2) & 1;
    const int64_t span = tile / kIvfTilesPerSpan;
    const int t = (int)(tile - span * kIvfTilesPerSpan);
    const int local = h * (kIvfSpanRows / 2) + t * 16 + r;
    const bool valid = local < span_valid[span];
    const int64_t row = (int64_t)span_row0[span] + local;
    const int d0 = ks * 32 + kh * 16;
    int4v out = {0, 0, 0, 0};
    if (valid && d0 < D) {
        out = *reinterpret_cast<const int4v *>(rows8 + (size_t)row * pitch + d0);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int keep = D - (d0 + 4 * w);           // dims of this word below D
            if (keep <= 0) out[w] = 0;
            else if (keep < 4) out[w] &= (int)((1u << (8 * keep)) - 1u);
        }
    }
    panels[gid] = out;
}

// ---- build: the accumulator inits of both scans and the row statistics, from the int8 rows -------------------------------
// One thread per panel row.  x = byte + cx; sum x^2 and sum x are exact integers (<= 128 * 255^2 < 2^24), so
//   bias8 / rowstat   are the integers ivf_build_bias_i8_kernel takes from the float32 rows,
//   bias (fp16 scan)  L2: (float)sum x^2 -- the float32 ||x||^2 of corpus_stats_kernel, which rounds the same integer once and
//                     loses nothing below 2^24; IP: 0; padding rows kPadBias -- what ivf_build_bias_kernel stores,
//   *maxn2            max sum x^2: the integer whose float32 is the corpus' maxnorm2.
__global__ __launch_bounds__(256) void ivf_i8_build_bias_kernel(const signed char *__restrict__ rows8, int pitch, int cx,
                                                                int64_t nspans, int D, int metric,
                                                                const int32_t *__restrict__ span_row0,
                                                                const int32_t *__restrict__ span_valid,
                                                                int32_t *__restrict__ bias8, int *__restrict__ rowstat,
                                                                float *__restrict__ bias, int *__restrict__ maxn2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = nspans * kIvfSpanRows;
    int n2 = 0;
    if (i < total) {
        const int64_t span = i / kIvfSpanRows;
        const int local = (int)(i - span * kIvfSpanRows);
        if (local >= span_valid[span]) {
            bias8[i] = kI8PadBias;
            bias8[total + i] = kI8PadBias;
            bias[i] = kPadBias;
        } else {
            const int64_t row = (int64_t)span_row0[span] + local;
            const int *xw = reinterpret_cast<const int *>(rows8 + (size_t)row * pitch);
            int s1 = 0;
            for (int d = 0; d < D; ++d) {
                const int v = (int)(signed char)((xw[d >> 2] >> (8 * (d & 3))) & 0xff) + cx;
                n2 += v * v;
                s1 += v;
            }
            rowstat[2 * row] = n2;
            rowstat[2 * row + 1] = s1;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const long long cq = w == 0 ? 127 : -1;
                const long long b = metric == 0 ? (((long long)n2 - 2 * cq * s1) >> 1) : -cq * s1;    // (>> on a negative: floor)
                bias8[(size_t)w * total + i] = (int32_t)(b + kI8Offset);
            }
            bias[i] = metric == 0 ? (float)n2 : 0.f;
        }
    }
    for (int o = 32; o > 0; o >>= 1) n2 = max(n2, __shfl_xor(n2, o));
    if ((threadIdx.x & 63) == 0 && n2 > *reinterpret_cast<volatile int *>(maxn2)) atomicMax(maxn2, n2);
}

// ---- per batch: the fp16 panels of the whole panel space, converted from the int8 panels ----------------------------------
// The 32-row form of convert_slab_from_i8_kernel over the IVF panel space: fp16 piece (tile, 16-dim k-step ks, lane = (row rho,
// k half kh)) = dims [16 ks + 8 kh, +8) of MFMA row rho = 8 consecutive bytes of the int8 piece (tile, ks / 2, lane' = rho + 32 *
// (that offset >= 16)), value (half)((float)(byte + cx) * sx) -- what ivf_build_panels_kernel makes of the float32 row.  Rows past a
// span's valid count and dims >= D hold A = 0 in the int8 panels (x = cx there) and must come out as 0: both are re-checked.
// Returns at once when the int8 scan serves the batch (info->i8_mode).
__global__ __launch_bounds__(256) void ivf_panels_from_i8_kernel(const int4v *__restrict__ panels8, int ks32, int ksteps, int cx,
                                                                 float sx, int64_t ntiles, int D,
                                                                 const int32_t *__restrict__ span_valid,
                                                                 const QueryBatchInfo *__restrict__ info,
                                                                 half8 *__restrict__ out) {
    if (info->i8_mode) return;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gid & 63);
    const int64_t tk = gid >> 6;
    const int ks = (int)(tk % ksteps);
    const int64_t tile = tk / ksteps;
    if (tile >= ntiles) return;
    const int rho = lane & 31, kh = lane >> 5;
    const int r = (rho & 3) | ((rho >> 3) << 2), h = (rho >> 2) & 1;
    const int64_t span = tile / kIvfTilesPerSpan;
    const int t = (int)(tile - span * kIvfTilesPerSpan);
    const int local = h * (kIvfSpanRows / 2) + t * 16 + r;
    const bool valid = local < span_valid[span];
    const int d0 = ks * 16 + kh * 8;
    const int o = (ks & 1) * 16 + kh * 8;                   // dim offset inside the 32-dim int8 k-step
    const int4v src = panels8[((size_t)tile * ks32 + (ks >> 1)) * 64 + rho + 32 * (o >> 4)];
    const int w0 = src[(o & 15) >> 2], w1 = src[((o & 15) >> 2) + 1];
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = (j < 4 ? (w0 >> (8 * j)) : (w1 >> (8 * (j - 4)))) & 0xff;
        const int x = (int)(signed char)b + cx;
        v[j] = (_Float16)((valid && d0 + j < D) ? (float)x * sx : 0.f);
    }
    out[gid] = v;
}

// option "ivf_i8_scratch" = 0: there are no fp16 panels, so a batch the int8 scan does not serve is flagged as a whole -- the
// select sends every query to the exact list scan of the tail, the flagged-query pass that also answers unusable scales.
// One wave, behind the batch's prep (which finalises info) and ahead of the select.
__global__ __launch_bounds__(64) void ivf_i8_flag_kernel(QueryBatchInfo *__restrict__ info) {
    if (threadIdx.x == 0 && !info->i8_mode) info->force_fallback = 1;
}

}  // namespace vdb

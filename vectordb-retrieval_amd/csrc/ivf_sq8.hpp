// ivf_sq8.hpp -- IVF<nlist>,SQ8 device kernels: range training, encoding, code gather, decoded rows and per-search fp16 panels.
//
// The codec is FAISS' IndexIVFScalarQuantizer with QT_8bit, RS_minmax and by_residual (index_factory "IVF<n>,SQ8"),
// every step float32 and rounded as written (the library compiles with -ffp-contract=off).  c_l = centroid of the row's list:
//   train   r = x - c_l;  vmin[d] = min r[d];  vdiff[d] = max r[d] - vmin[d]
//   encode  u = vdiff[d] != 0 ? (r[d] - vmin[d]) / vdiff[d] : 0;  u = clamp(u, 0, 1);  code = (uint8) trunc(255 * u)
//   decode  x^[d] = c_l[d] + (vmin[d] + ((code + 0.5f) / 255.0f) * vdiff[d])
// Every search path scores x^ (the row accessor sq8_key in refine.hpp: the exact list scan, the refine, the flagged-query
// fallback), and the MFMA list scan runs on fp16 panels converted from the codes per search that equal, bit for bit, the
// panels IVF-Flat builds from the float32 rows x^ -- so an SQ8 index returns what an IVF-Flat index over x^ (same lists)
// returns, under the same exactness guard (DESIGN 4.4 "IVF-SQ8").
// Device layout: codes [N][D4] bytes in list order (padding bytes 0), the list of every list-order row (int32), the
// centroids [nlist][D4] and {vmin, vdiff} [2][D4] float32, both zero padded -- a padding dimension decodes to exactly 0.
#pragma once
#include "common.hpp"
#include "ivf_mfma.hpp"
#include "refine.hpp"

namespace vdb {

// ---- range training: per-dimension min / max of the residuals r = x - c_l ------------------------------------------
// x [n][D] unpadded, cent [nlist][D4].  Block = 64 dims x 4 row lanes over one chunk of rows; partial minima / maxima
// per chunk ([chunks][D]) are reduced on the host (min / max are exact and order-free: no dependence on the chunking).
constexpr int kSq8RangeChunks = 256;

__global__ __launch_bounds__(256) void sq8_range_kernel(const float *__restrict__ x, int64_t n, int D, int D4,
                                                        const float *__restrict__ cent, const int64_t *__restrict__ assign,
                                                        float *__restrict__ pmin, float *__restrict__ pmax) {
    __shared__ float smin[4][64], smax[4][64];
    const int dl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + dl;
    const int64_t per = (n + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = min(n, r0 + per);
    float lo = INFINITY, hi = -INFINITY;
    if (d < D)
        for (int64_t r = r0 + rl; r < r1; r += 4) {
            const float v = x[(size_t)r * D + d] - cent[(size_t)assign[r] * D4 + d];
            // (fminf / fmaxf drop a NaN: it opens the range to infinity instead, which sq8_train_ranges refuses like an inf)
            lo = fminf(lo, v != v ? -INFINITY : v);
            hi = fmaxf(hi, v != v ? INFINITY : v);
        }
    smin[rl][dl] = lo;
    smax[rl][dl] = hi;
    __syncthreads();
    if (rl == 0 && d < D) {
        for (int j = 1; j < 4; ++j) {
            lo = fminf(lo, smin[j][dl]);
            hi = fmaxf(hi, smax[j][dl]);
        }
        pmin[(size_t)blockIdx.y * D + d] = lo;
        pmax[(size_t)blockIdx.y * D + d] = hi;
    }
}

// ---- encode: rows [n][D4] (zero padded) -> codes [n][D4]; cent / vmin / vdiff zero padded to D4 (padding -> code 0) --
__global__ __launch_bounds__(256) void sq8_encode_kernel(const float *__restrict__ x, int64_t n, int D4,
                                                         const float *__restrict__ cent, const int64_t *__restrict__ assign,
                                                         const float *__restrict__ vmin, const float *__restrict__ vdiff,
                                                         unsigned char *__restrict__ codes) {
    // (grid-stride: a launch covers any n * D4)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * D4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / D4;
        const int d = (int)(i - r * D4);
        const float res = x[i] - cent[(size_t)assign[r] * D4 + d];
        const float vd = vdiff[d];
        float u = vd != 0.f ? (res - vmin[d]) / vd : 0.f;
        u = u > 1.f ? 1.f : (u >= 0.f ? u : 0.f);       // clamp (a NaN residual becomes 0)
        codes[i] = (unsigned char)(int)(255.f * u);
    }
}

// ---- CSR build of the codes: codes[i] = src[perm[i]], ids[i] as gather_rows_kernel sets them -------------------------
__global__ __launch_bounds__(256) void sq8_gather_kernel(const unsigned char *__restrict__ src, const int32_t *__restrict__ perm,
                                                         int64_t n, int D4, int64_t id_base, const int64_t *__restrict__ src_ids,
                                                         unsigned char *__restrict__ codes, int64_t *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = n * (D4 / 4);
    if (i >= total) return;
    const int64_t r = i / (D4 / 4);
    const int c = (int)(i - r * (D4 / 4));
    const int64_t s = perm[r];
    reinterpret_cast<unsigned *>(codes)[i] = reinterpret_cast<const unsigned *>(src)[s * (D4 / 4) + c];
    if (c == 0) ids[r] = src_ids ? src_ids[s] : id_base + s;
}

// ---- decoded rows x^ [n][pitch] (d < D; the caller clears any padding) of list-order rows: the query rows of vdb_reserve,
// and the float32 rows the panel space of an SQ8 index is derived from at build time (the transient x32 of sq8_build_panel_space)
__global__ __launch_bounds__(256) void sq8_decode_rows_kernel(Sq8Rows s, int64_t n, int D, int D4, int pitch, float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * D; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / D;
        const int d = (int)(i - r * D);
        out[(size_t)r * pitch + d] = sq8_decode(s.codes[(size_t)r * D4 + d], s.cent[(size_t)s.list[r] * D4 + d], s.vmin[d], s.vdiff[d]);
    }
}

// ---- per-search fp16 panels of an SQ8 index (D <= 128, 32-row tiles): ivf_build_panels_kernel with X[row][d] replaced by
// the decoded x^[d] -- the same float32 value times the same sx, rounded to fp16 the same way, so the panels are bit for bit
// the ones an IVF-Flat index over the float32 rows x^ holds (no statistics flag: the build took it from the same values)
__global__ __launch_bounds__(256) void ivf_sq8_panels_kernel(Sq8Rows s, int D, int D4, int ksteps, int64_t ntiles, float sx,
                                                             const int32_t *__restrict__ span_row0,
                                                             const int32_t *__restrict__ span_valid, half8 *__restrict__ panels) {
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
    const int64_t row = (int64_t)span_row0[span] + local;
    const int d0 = ks * 16 + kh * 8;
    half8 out;
    const unsigned char *code = valid ? s.codes + (size_t)row * D4 : nullptr;
    const float *cent = valid ? s.cent + (size_t)s.list[row] * D4 : nullptr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = d0 + j;
        float v = 0.f;
        if (valid && d < D) v = sq8_decode(code[d], cent[d], s.vmin[d], s.vdiff[d]) * sx;
        out[j] = (_Float16)v;
    }
    panels[gid] = out;
}

}  // namespace vdb

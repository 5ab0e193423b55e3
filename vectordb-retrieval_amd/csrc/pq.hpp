// pq.hpp -- kernels of the product quantizer: the encoder and the row decoder that the flat PQ<M> index and IVF<nlist>,PQ<M>
// (ivf_pq.hpp: RESIDUAL) share, then the table and panel kernels of the flat index (host side: pq.inc; contract: include/vdbhip.h).
//
// A PQ index keeps M code bytes per row and the codebooks, float32 [M][256][dsub] (dsub = D / M).  The reconstructed row
// x^ is the concatenation of codebook[m][code[m]] -- a lookup, no arithmetic -- and a search is the flat exact search of
// this library over the float32 rows x^.  Nothing but the codes is resident: the exact kernels read x^ through pq_key
// (refine.hpp), and the fp16 MFMA scan reads panels that pq_panels_kernel makes from the codes per search, slab by slab.
#pragma once
#include "common.hpp"
#include "prep.hpp"
#include "refine.hpp"

namespace vdb {

// ---- rows -> codes ----------------------------------------------------------------------------------------------------
// code[i][m] = argmin over c of the canonical float64 L2 key between r[m dsub .. (m + 1) dsub) and codebook[m][c]
// (acc = fma(t, t, acc), t = (double)r[d] - (double)c[d], d ascending), ties to the smaller c, whatever the index metric.
// r = x[i], or (RESIDUAL: IVF-PQ, ivf_pq.inc) x[i] - cent[assign[i]]: one float32 subtraction per dimension, rounded before it
// is widened; cent [nlist][pitch] is zero padded like X and assign[i] was validated on the host.
// grid (row blocks, M): one sub-space per workgroup, its 256 centroids in LDS when they fit `lds_floats` (every lane
// of a wave reads the same centroid element: a broadcast), else read from the codebook -- two loops, so that the address
// space of every load is known at compile time; grid-stride over the rows.
template <bool RESIDUAL>
__global__ __launch_bounds__(256) void pq_encode_kernel(const float *__restrict__ X, int64_t n, int64_t pitch, const float *__restrict__ cent,
                                                        const int64_t *__restrict__ assign, const float *__restrict__ cb, int M, int dsub,
                                                        int lds_floats, unsigned char *__restrict__ codes) {
    extern __shared__ float pq_enc_lds[];
    const int m = blockIdx.y;
    const float *cm = cb + (size_t)m * 256 * dsub;
    const bool in_lds = 256 * dsub <= lds_floats;
    if (in_lds) {
        for (int i = threadIdx.x; i < 256 * dsub; i += 256) pq_enc_lds[i] = cm[i];
        __syncthreads();
    }
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        const float *x = X + (size_t)row * pitch + (size_t)m * dsub;
        const float *cl = RESIDUAL ? cent + (size_t)assign[row] * pitch + (size_t)m * dsub : nullptr;
        double best = __builtin_inf();
        int arg = 0;
        for (int c = 0; c < 256; ++c) {
            double acc = 0.0;
            if (in_lds) {
                const float *cv = pq_enc_lds + c * dsub;
                for (int j = 0; j < dsub; ++j) {
                    const float r = RESIDUAL ? x[j] - cl[j] : x[j];
                    const double t = (double)r - (double)cv[j];
                    acc = fma(t, t, acc);
                }
            } else {
                const float *cv = cm + (size_t)c * dsub;
                for (int j = 0; j < dsub; ++j) {
                    const float r = RESIDUAL ? x[j] - cl[j] : x[j];
                    const double t = (double)r - (double)cv[j];
                    acc = fma(t, t, acc);
                }
            }
            if (acc < best) {       // (strict: the smaller c keeps a tie; a NaN key never wins)
                best = acc;
                arg = c;
            }
        }
        codes[(size_t)row * M + m] = (unsigned char)arg;
    }
}

// ---- codes -> float32 rows x^ -----------------------------------------------------------------------------------------
// out[r][d] = codebook[d / dsub][code[r][d / dsub]][d % dsub] for d < D, plus (RESIDUAL: IVF-PQ, list-order rows) the
// centroid cent[list[r]][d] in ONE float32 add; 0 for D <= d < pitch.  Grid-stride, one element per thread and trip.  Used
// for the transient copy of a build (pitch D4) and for the query rows of vdb_reserve (pitch D).
template <bool RESIDUAL>
__global__ __launch_bounds__(256) void pq_decode_rows_kernel(IvfPqRows p, int64_t n, int D, int D4, int64_t pitch, float *__restrict__ out) {
    const int64_t total = n * pitch;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / pitch;
        const int d = (int)(i - r * pitch);
        float v = 0.f;
        if (d < D) {
            const PqRows &c = p.pq;
            const int m = d / c.dsub;
            v = c.cb[((size_t)m * 256 + c.codes[(size_t)r * c.M + m]) * c.dsub + (d - m * c.dsub)];
            if (RESIDUAL) v = p.cent[(size_t)p.list[r] * D4 + d] + v;
        }
        out[i] = v;
    }
}

// fp16-exactness flag of a float32 corpus under the scale sx (what build_panels*_kernel take while they write panels)
__global__ __launch_bounds__(256) void pq_fp16_flag_kernel(const float *__restrict__ X, int64_t total, float sx, IndexStats *st) {
    int inexact = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float v = X[i] * sx;
        inexact |= ((float)(_Float16)v != v);
    }
    if (__any(inexact) && (threadIdx.x & 63) == 0) atomic_set_flag(&st->not_fp16_exact);
}

// the scaled codebooks, rounded to fp16 once per build: tab[i] = (half)(codebook[i] * sx) -- the rounding X[row][d] * sx gets
// when build_panels*_kernel convert a float32 corpus (decoding is a lookup, so it commutes with the rounding)
__global__ __launch_bounds__(256) void pq_table_kernel(const float *__restrict__ cb, int64_t total, float sx, _Float16 *__restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) tab[i] = (_Float16)(cb[i] * sx);
}

// ---- codes -> fp16 panels of one slab (the per-search hot path) ---------------------------------------------------------
struct PqPanelArgs {
    const unsigned char *codes;   // [N][M]; the buffer holds 16 spare bytes behind the last row
    const _Float16 *tab;          // [M][256][dsub] halves
    half8 *panels;                // the slab: tiles [tile0, tile0 + ntiles) in the layout of the scan, from panels[0]
    int64_t N, tile0, ntiles;
    int D, M, dsub;
    int p16;                      // 0: layout "x16" (D <= 128: 32-row tiles, ks16 16-dim k-steps); 1: p16 (16-row tiles, ks32-dim steps)
    int ksteps;                   // k-steps per tile in that layout
    int slice_ks;                 // k-steps (of 32 dims) per table slice: blockIdx.y owns dims [32 y slice_ks, 32 (y + 1) slice_ks)
    int code_pitch;               // bytes per staged code row in LDS (M rounded up to a dword, an odd number of dwords)
};

// LDS image of the table: every sub-space starts kPqTabSkew halves (16 bytes = 4 banks) later than in the packed table.  A sub-space
// of the packed table is a multiple of 512 bytes, so the four 16-lane groups of a gather -- same rows, dims 8 apart, hence other
// sub-spaces when dsub <= 8 -- would meet on the same banks whenever their codes are equal; with the skew they meet 4 banks apart
// per sub-space of distance.  What remains is the conflict rate of random addresses: the codes are data.
constexpr int kPqTabSkew = 8;

// One wave per tile.  The tile's code rows (four runs of consecutive rows) are staged in LDS with 16-byte loads, then every
// lane builds its half8 of every k-step -- 8 consecutive dims of one row -- by gathering W halves at a time from the table
// (W = the largest power of two <= 8 dividing dsub, so a gather never straddles two sub-spaces) and stores 16 bytes: a
// wave writes 1 KiB contiguous per k-step.  LDS = true: the table slice sits in LDS behind the staging area (false: it did
// not fit and is read through the cache).  The staged code rows have an odd dword pitch (the 16 rows a lane group reads
// fall on different banks).  Staging is private to a wave: the one workgroup barrier stands behind the table copy.
template <int W, bool LDS>
__global__ __launch_bounds__(256) void pq_panels_kernel(PqPanelArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = a.p16 ? 16 : 32, runlen = a.p16 ? 4 : 8;
    const int stage_bytes = (R * a.code_pitch + 15) & ~15;
    unsigned char *stage = pq_lds + wave * stage_bytes;
    const int ks32_lo = blockIdx.y * a.slice_ks;                       // (32-dim steps)
    const int ks32_n = a.p16 ? a.ksteps : a.ksteps / 2;
    const int ks32_hi = min(ks32_n, ks32_lo + a.slice_ks);
    const int m_lo = (ks32_lo * 32) / a.dsub;                          // (slices start on a sub-space boundary)
    _Float16 *lt = reinterpret_cast<_Float16 *>(pq_lds + 4 * stage_bytes);     // (kept an LDS pointer: ds_read gathers, not flat loads)
    if (LDS) {
        const int m_hi = min(a.M, (ks32_hi * 32 + a.dsub - 1) / a.dsub);
        const int per = 32 * a.dsub;                                   // 16-byte pieces per sub-space (256 dsub halves)
        const int n16 = (m_hi - m_lo) * per;
        const uint4 *src = reinterpret_cast<const uint4 *>(a.tab + (size_t)m_lo * 256 * a.dsub);
        // (sub-space s of the slice starts s * 16 bytes later than in the table: kPqTabSkew below)
        for (int i = threadIdx.x; i < n16; i += 256) reinterpret_cast<uint4 *>(lt)[i + i / per] = src[i];
        __syncthreads();          // the only workgroup barrier: the staging below is private to a wave
    }
    const int64_t total_bytes = a.N * a.M;
    const int run_bytes = runlen * a.M;
    const bool vec = (a.M & 3) == 0;                                   // runs start 16-byte aligned and split into whole dwords per row
    const int rho = lane & 15;
    for (int64_t t4 = blockIdx.x; t4 * 4 < a.ntiles; t4 += gridDim.x) {
        const int64_t tl = t4 * 4 + wave;
        const bool live = tl < a.ntiles;
        const int64_t tile = a.tile0 + tl;
        int64_t span, row_t;      // first row of run g: span_row0 + g * run_stride + row_t
        int run_stride;
        if (a.p16) {
            span = tile / kTilesPerSpan16;
            row_t = span * kSpanRows16 + 4 * (tile - span * kTilesPerSpan16);
            run_stride = kBinRows;
        } else {
            span = tile / kTilesPerSpan;
            row_t = span * kSpanRows + 8 * (tile - span * kTilesPerSpan);
            run_stride = 128;
        }
        // (no barrier: a wave stages and reads its own tile only, and its LDS operations execute in program order -- the
        //  wave barriers keep the compiler from moving the gathers of one tile across the staging stores of the next)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (live) {
            for (int g = 0; g < 4; ++g) {
                const int64_t byte0 = (row_t + (int64_t)g * run_stride) * a.M;
                unsigned char *dst = stage + g * runlen * a.code_pitch;
                if (vec) {
                    for (int off = lane * 16; off < run_bytes; off += 1024) {
                        uint4 v = make_uint4(0, 0, 0, 0);
                        if (byte0 + off < total_bytes) v = *reinterpret_cast<const uint4 *>(a.codes + byte0 + off);   // (16 spare bytes behind the codes)
                        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int o = off + 4 * j;
                            if (o < run_bytes) {
                                const int r = o / a.M;
                                *reinterpret_cast<unsigned *>(dst + r * a.code_pitch + (o - r * a.M)) = w[j];
                            }
                        }
                    }
                } else {
                    for (int off = lane; off < run_bytes; off += 64) {
                        const int r = off / a.M;
                        dst[r * a.code_pitch + (off - r * a.M)] = byte0 + off < total_bytes ? a.codes[byte0 + off] : (unsigned char)0;
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (!live) continue;
        half8 *out = a.panels + (size_t)tl * a.ksteps * 64 + lane;
        const int g = rho >> 2, i = rho & 3;
        for (int ks32 = ks32_lo; ks32 < ks32_hi; ++ks32) {
            const int d0 = ks32 * 32 + (lane >> 4) * 8;
            const int nsub = a.p16 ? 1 : 2;                            // x16: two 16-dim k-steps (row blocks rb) share the dims of a 32-dim step
            for (int rb = 0; rb < nsub; ++rb) {
                const int r = a.p16 ? rho : g * 8 + rb * 4 + i;        // staged row of this lane
                const int64_t row = row_t + (int64_t)g * run_stride + (a.p16 ? i : rb * 4 + i);
                const unsigned char *cr = stage + r * a.code_pitch;
                union { half8 v; _Float16 h[8]; unsigned u[4]; } o;
                o.u[0] = o.u[1] = o.u[2] = o.u[3] = 0u;
                if (row < a.N && d0 < a.D) {
                    int m = d0 / a.dsub, j = d0 - m * a.dsub;
#pragma unroll
                    for (int e = 0; e < 8; e += W) {
                        if (d0 + e < a.D) {                            // (D is a multiple of W: whole gathers)
                            const _Float16 *src = LDS ? lt + (m - m_lo) * (256 * a.dsub + kPqTabSkew) + cr[m] * a.dsub + j
                                                      : a.tab + ((size_t)m * 256 + cr[m]) * a.dsub + j;
                            if (W == 8) o.v = *reinterpret_cast<const half8 *>(src);
                            else if (W == 4) { const uint2 t = *reinterpret_cast<const uint2 *>(src); o.u[e / 2] = t.x; o.u[e / 2 + 1] = t.y; }
                            else if (W == 2) o.u[e / 2] = *reinterpret_cast<const unsigned *>(src);
                            else o.h[e] = *src;
                        }
                        j += W;
                        if (j == a.dsub) { j = 0; ++m; }
                    }
                }
                out[(size_t)(a.p16 ? ks32 : 2 * ks32 + rb) * 64] = o.v;
            }
        }
    }
}

}  // namespace vdb

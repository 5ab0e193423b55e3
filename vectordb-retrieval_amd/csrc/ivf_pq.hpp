// ivf_pq.hpp -- IVF<nlist>,PQ<M> device kernels: residual encoding, code gather, decoded rows and per-search fp16 panels.
//
// The codec is the product quantizer of pq.hpp applied to the residuals of the inverted lists (index_factory "IVF<n>,PQ<M>"
// in spirit; the contract is the library's own, include/vdbhip.h).  c_l = centroid of the row's list, dsub = D / M, every
// step float32 and rounded as written (the library compiles with -ffp-contract=off):
//   encode  r = x - c_l;  code[m] = argmin over c of the canonical float64 L2 key between r[m dsub .. (m + 1) dsub) and
//           codebook[m][c], ties to the smaller c
//   decode  x^[d] = c_l[d] + codebook[m][code[m]][j]   (ONE float32 add; a padding dimension decodes to exactly 0)
// Every search path scores x^ (the row accessor ivfpq_key in refine.hpp: the exact list scan, the refine, the flagged-query
// fallback), and the MFMA list scan runs on fp16 panels made from the codes per batch that equal, bit for bit, the panels
// IVF-Flat builds from the float32 rows x^ -- so an IVF-PQ index returns what an IVF-Flat index over x^ (same lists)
// returns, under the same exactness guard (DESIGN 4.4 "IVF-PQ").
// Device layout: codes [N][M] bytes in list order, the list of every list-order row (int32), the centroids [nlist][D4]
// zero padded, the codebooks float32 [M][256][dsub].
#pragma once
#include "common.hpp"
#include "ivf_mfma.hpp"
#include "pq.hpp"

namespace vdb {

// (rows -> codes and codes -> rows: pq_encode_kernel<true> and pq_decode_rows_kernel<true>, pq.hpp)

// ---- CSR build of the codes: codes[i] = src[perm[i]] (rows of M bytes), ids[i] as gather_rows_kernel sets them -----------
__global__ __launch_bounds__(256) void ivfpq_gather_kernel(const unsigned char *__restrict__ src, const int32_t *__restrict__ perm, int64_t n,
                                                           int M, int64_t id_base, const int64_t *__restrict__ src_ids,
                                                           unsigned char *__restrict__ codes, int64_t *__restrict__ ids) {
    const int64_t total = n * M;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / M;
        const int c = (int)(i - r * M);
        const int64_t s = perm[r];
        codes[i] = src[s * M + c];
        if (c == 0) ids[r] = src_ids ? src_ids[s] : id_base + s;
    }
}

// ---- per-search fp16 panels of an IVF-PQ index (D <= 128, 32-row tiles): ivf_build_panels_kernel with X[row][d] replaced
// by the decoded x^[d] = c_l[d] + codebook entry -- the same float32 value times the same sx, rounded to fp16 the same way,
// so the panels are bit for bit the ones an IVF-Flat index over the float32 rows x^ holds.  (The table is NOT pre-scaled or
// pre-rounded as pq_panels_kernel's is: the add comes before the scale and the rounding.)
struct IvfPqPanelArgs {
    IvfPqRows rows;
    const int32_t *span_row0, *span_valid;
    half8 *panels;                // the whole panel space: [tile][ks][lane]
    int64_t ntiles;
    float sx;
    int D, D4, ksteps;
    int slice_ks;                 // 16-dim k-steps per table slice: blockIdx.y owns the k-steps [y slice_ks, (y + 1) slice_ks)
    int code_pitch;               // bytes per staged code row in LDS (M rounded up to a dword, an odd number of dwords)
};

constexpr int kIvfPqCentFloats = 128;      // a wave's staged centroid: the dims of kMaxKSteps k-steps

// One wave per tile, four tiles per workgroup, grid-stride over the tile groups.  A tile lies inside ONE panel span, hence
// one list: the wave stages the tile's code rows (two runs of 16 consecutive list-order rows) and its centroid (read once
// per tile) in LDS, then every lane builds its half8 of every k-step of the slice -- 8 consecutive dims of one row -- and
// stores 16 bytes: a wave writes 1 KiB contiguous per k-step.  LDS = true: the float32 codebooks of the sub-spaces the
// slice's dims touch sit in LDS behind the staging areas (false: no slice fits; they are read through the cache).  A code
// byte indexes 256 entries and a dim below D a sub-space of the slice, so every table read is in bounds by construction;
// the list ids were validated on the host when the rows were added.  Staging is private to a wave: the one workgroup
// barrier stands behind the table copy.
template <bool LDS>
__global__ __launch_bounds__(256) void ivf_pq_panels_kernel(IvfPqPanelArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ivfpq_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = a.rows.pq.M, dsub = a.rows.pq.dsub;
    const int stage_bytes = (32 * a.code_pitch + 15) & ~15;
    const int wave_bytes = stage_bytes + kIvfPqCentFloats * (int)sizeof(float);
    unsigned char *stage = ivfpq_lds + wave * wave_bytes;
    float *cstage = reinterpret_cast<float *>(stage + stage_bytes);
    float *lt = reinterpret_cast<float *>(ivfpq_lds + 4 * wave_bytes);
    const int ks_lo = blockIdx.y * a.slice_ks, ks_hi = min(a.ksteps, ks_lo + a.slice_ks);
    const int d_hi = min(a.D, ks_hi * 16);
    const int m_lo = min(ks_lo * 16, a.D) / dsub;
    if (LDS) {
        const int m_hi = (d_hi + dsub - 1) / dsub;
        const int nf = (m_hi - m_lo) * 256 * dsub;                     // (<= 0: the slice holds padding dims only)
        const float *src = a.rows.pq.cb + (size_t)m_lo * 256 * dsub;
        for (int i = threadIdx.x; i < nf; i += 256) lt[i] = src[i];
        __syncthreads();
    }
    const bool vec = (M & 3) == 0;                                     // code rows are whole, 4-byte aligned dwords
    for (int64_t t4 = blockIdx.x; t4 * 4 < a.ntiles; t4 += gridDim.x) {
        const int64_t tile = t4 * 4 + wave;
        const bool live = tile < a.ntiles;
        // (no workgroup barrier: a wave stages and reads its own tile only, and its LDS operations execute in program order --
        //  the wave barriers keep the compiler from moving the reads of one tile across the staging stores of the next)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int t = 0, nvalid = 0;
        if (live) {
            const int64_t span = tile / kIvfTilesPerSpan;
            t = (int)(tile - span * kIvfTilesPerSpan);
            nvalid = a.span_valid[span];
            const int64_t row0 = a.span_row0[span];
            if (nvalid > 0) {
                const float *cl = a.rows.cent + (size_t)a.rows.list[row0] * a.D4;
                for (int d = lane; d < kIvfPqCentFloats; d += 64) cstage[d] = d < a.D ? cl[d] : 0.f;
            }
            // 4 lanes per code row: lane >> 2 = row of the run, lane & 3 = first dword (byte) of its stride-4 share
            const int r = lane >> 2, c0 = lane & 3;
            for (int h = 0; h < 2; ++h) {
                const int local = h * (kIvfSpanRows / 2) + t * 16 + r;
                if (local < nvalid) {
                    const unsigned char *src = a.rows.pq.codes + (size_t)(row0 + local) * M;
                    unsigned char *dst = stage + (h * 16 + r) * a.code_pitch;
                    if (vec)
                        for (int c = c0; c < M / 4; c += 4) reinterpret_cast<unsigned *>(dst)[c] = reinterpret_cast<const unsigned *>(src)[c];
                    else
                        for (int c = c0; c < M; c += 4) dst[c] = src[c];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (!live) continue;
        const int rho = lane & 31, kh = lane >> 5;
        const int r = (rho & 3) | ((rho >> 3) << 2), h = (rho >> 2) & 1;
        const bool valid = h * (kIvfSpanRows / 2) + t * 16 + r < nvalid;
        const unsigned char *cr = stage + (h * 16 + r) * a.code_pitch;
        half8 *out = a.panels + (size_t)tile * a.ksteps * 64 + lane;
        for (int ks = ks_lo; ks < ks_hi; ++ks) {
            const int d0 = ks * 16 + kh * 8;
            union { half8 v; _Float16 h[8]; unsigned u[4]; } o;
            o.u[0] = o.u[1] = o.u[2] = o.u[3] = 0u;
            if (valid && d0 < a.D) {
                int m = d0 / dsub, j = d0 - m * dsub;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (d0 + e < a.D) {
                        const float tv = LDS ? lt[((m - m_lo) * 256 + cr[m]) * dsub + j] : a.rows.pq.cb[((size_t)m * 256 + cr[m]) * dsub + j];
                        o.h[e] = (_Float16)((cstage[d0 + e] + tv) * a.sx);
                        if (++j == dsub) { j = 0; ++m; }
                    }
                }
            }
            out[(size_t)ks * 64] = o.v;
        }
    }
}

}  // namespace vdb

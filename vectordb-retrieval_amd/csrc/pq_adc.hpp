// pq_adc.hpp -- the lookup-table (ADC: asymmetric distance computation) scan of a flat PQ<M> index for small query batches
// (host side: pq.inc, search_flat.inc; contract and error bound: DESIGN.md 4.9 "ADC scan").
//
// The panel pass (pq.hpp) decodes the whole corpus into fp16 panels before the MFMA scan may run; for a handful of queries that
// decode is nearly the whole search.  Here nothing is decoded: a query gets one table of M x 256 partial scores, a row's score is
// M byte-indexed lookups and M float32 adds, and the scores are reduced to exactly the bin records scan_x16_kernel (D <= 128,
// octs) / scan16_kloop_kernel (D > 128, quads) write -- select_kernel*, refine_tail_kernel and the fallback pass consume them
// unchanged.  In both panel layouts a level-1 bin is 256 CONSECUTIVE rows, bin b = rows [256 b, 256 b + 256) = (span b / G,
// lane group b % G), and a candidate group is 8 (4) consecutive rows whose number inside the bin is the packed id.
//   T[q][m][c] = (float)(bs * acc),  acc = sum_j fma((double)q[m dsub + j], (double)cb[m][c][j], acc), j ascending from 0.0,
//                bs = -2 cs (L2) | -cs (IP): the table is in the scan's scaled units (QueryBatchInfo.cs)
//   score(row) = s_M,  s_0 = cs * bias[row],  s_{m+1} = s_m + T[q][m][code[row][m]]  (float32, m ascending; a padding row keeps kPadBias)
#pragma once
#include "common.hpp"
#include "prep.hpp"
#include "scan.hpp"

namespace vdb {

// ---- tables + error bounds of a batch ---------------------------------------------------------------------------------------
constexpr int kPqAdcQB = 8;       // queries per workgroup of the table kernel: a codebook entry is read once for the eight

struct PqAdcTableArgs {
    const float *Q;               // [nq][D]
    const float *cb;              // the float32 codebooks [M][256][dsub] (NOT the fp16 table of the panel pass)
    const QueryBatchInfo *info;
    float *tables;                // [nq][M][256]
    float *eps;                   // [nq]
    int64_t nq;
    int D, M, dsub, metric;
    float xnorm_max;              // max ||x^||
    const float *cs_dev = nullptr;   // IVF-PQ (ivf_pq_adc.hpp): the batch's scale, chosen by its prep kernel instead of info->cs; eps is then the caller's too
};

// The bound of the ADC scores against the ideal scaled key cs (||x^||^2 - 2 q.x^) (L2) / -cs q.x^ (IP), in scan units.  With
// mag = Xn^2 + 2 qn Xn (L2) | qn Xn (IP), every partial sum is at most cs mag in magnitude, so: the bias (one float32 rounding of
// the float64 norm), the M table entries (one rounding each, sum |T_m| <= f cs qn Xn by Cauchy-Schwarz twice) and the M adds
// contribute at most (M + 2) 2^-24 cs mag; the float64 chain behind an entry adds dsub 2^-53 of it.  (M + 3) 2^-23 is more than
// twice that.  Packing the group id into the low 6 mantissa bits moves a score by less than 2^-17 of its magnitude.  No fp16
// term: neither operand is rounded to fp16.  key64_round_err (prep.hpp) is the rounding of the exact key itself.  The 2 % slack and
// the clamp are those of query_eps_body.
__device__ __forceinline__ float pq_adc_eps(double n2, int metric, int M, int D, double Xn, double cs) {
    const double qn = sqrt(n2);
    const double mag = (metric == 0) ? (Xn * Xn + 2.0 * qn * Xn) : (qn * Xn);
    const double eps_true = (double)(M + 3) * ldexp(1.0, -23) * mag + ldexp(1.0, -17) * mag + key64_round_err(metric, D, qn, Xn);
    double e = cs * eps_true * 1.02;
    if (!(e < 1.0e37)) e = 1.0e37;
    return (float)e + 1.0e-30f;
}

// grid (M, ceil(nq / kPqAdcQB)): thread c of workgroup (m, query group) makes T[q][m][c] of the group's queries; the workgroups
// of sub-space 0 also take the norms and the bounds of their queries (wave w: queries w, w + 4 of the group).
__global__ __launch_bounds__(256) void pq_adc_tables_kernel(PqAdcTableArgs a) {
    const int m = blockIdx.x, c = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * kPqAdcQB;
    const int nqb = (int)(a.nq - q0 < kPqAdcQB ? a.nq - q0 : kPqAdcQB);
    const float cs = a.cs_dev ? *a.cs_dev : a.info->cs;
    const double bs = (double)((a.metric == 0 ? -2.f : -1.f) * cs);
    const float *cv = a.cb + ((size_t)m * 256 + c) * a.dsub;
    const float *qv = a.Q + (size_t)q0 * a.D + (size_t)m * a.dsub;
    double acc[kPqAdcQB];
#pragma unroll
    for (int i = 0; i < kPqAdcQB; ++i) acc[i] = 0.0;
    for (int j = 0; j < a.dsub; ++j) {
        const double x = (double)cv[j];
#pragma unroll
        for (int i = 0; i < kPqAdcQB; ++i)
            if (i < nqb) acc[i] = fma((double)qv[(size_t)i * a.D + j], x, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < kPqAdcQB; ++i)
        if (i < nqb) a.tables[((size_t)(q0 + i) * a.M + m) * 256 + c] = (float)(bs * acc[i]);
    if (m != 0 || a.cs_dev) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < nqb; i += 4) {
        const float *row = a.Q + (size_t)(q0 + i) * a.D;
        double n2 = 0.0;
        for (int d = lane; d < a.D; d += 64) n2 = fma((double)row[d], (double)row[d], n2);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n2 += __shfl_xor(n2, o);
        if (lane == 0) a.eps[q0 + i] = pq_adc_eps(n2, a.metric, a.M, a.D, (double)a.xnorm_max, (double)cs);
    }
}

// ---- one row's score --------------------------------------------------------------------------------------------------------
// T: the query's table [M][256] in LDS; cr: the row's M code bytes (staged in LDS or in the index); s0 = cs * bias[row].  Plain
// float32 adds in one fixed order.  DWORDS: cr is 4-byte aligned and M a multiple of 4 (four codes per load).  Sub-space m of
// the table starts at 256 m floats, a multiple of the bank count -- no skew: the lanes of a gather all read sub-space m, so two
// sub-spaces never meet in one instruction and what remains is the conflict rate of random addresses (the codes are data).
template <bool DWORDS, class CodePtr>
__device__ __forceinline__ float pq_adc_row_score(const float *T, CodePtr cr, int M, float s0) {
    float s = s0;
    if (DWORDS) {
        // sixteen codes at a time: their four dwords were read one block ahead, the sixteen gathers are issued together and only the
        // adds wait for them, in order -- one wave per SIMD (the table of M = 64 leaves one workgroup per CU) then has sixteen LDS
        // reads in flight instead of a dependent chain of code read -> gather -> add per sub-space
        int m = 0;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (M >= 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const unsigned *>(cr + 4 * j);
        }
        for (; m + 16 <= M; m += 16) {
            unsigned wn[4] = {0u, 0u, 0u, 0u};
            if (m + 32 <= M) {
#pragma unroll
                for (int j = 0; j < 4; ++j) wn[j] = *reinterpret_cast<const unsigned *>(cr + m + 16 + 4 * j);
            }
            float t[16];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) t[4 * j + b] = T[(m + 4 * j + b) * 256 + ((w[j] >> (8 * b)) & 255u)];
#pragma unroll
            for (int i = 0; i < 16; ++i) s += t[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = wn[j];
        }
        for (; m < M; m += 4) {
            const unsigned w = *reinterpret_cast<const unsigned *>(cr + m);
            s += T[(m + 0) * 256 + (w & 255u)];
            s += T[(m + 1) * 256 + ((w >> 8) & 255u)];
            s += T[(m + 2) * 256 + ((w >> 16) & 255u)];
            s += T[(m + 3) * 256 + (w >> 24)];
        }
    } else {
        for (int m = 0; m < M; ++m) s += T[m * 256 + cr[m]];
    }
    return s;
}

// ---- the scan ---------------------------------------------------------------------------------------------------------------
struct PqAdcScanArgs {
    const unsigned char *codes;   // [N][M]; the buffer holds 16 spare bytes behind the last row
    const float *bias;            // [Npad]
    const float *tables;          // [nq][M][256]
    const QueryBatchInfo *info;
    float *bin_m1, *bin_m2;       // [nspans * G][Qpad]
    float *sb_m1, *sb_m2;         // [nchunks * G][Qpad]
    int32_t *sb_span;
    int64_t N, nspans, Qpad;
    int M;
    int groups;                   // G: bins per span (2: D <= 128, 4: D > 128)
    int gshift;                   // log2 rows per candidate group: 3 (octs, D <= 128) | 2 (quads, D > 128) -- what scan_select assumes
    int code_pitch;               // STAGED: bytes per staged code row (an odd number of dwords)
    int spans_per_chunk, chunk_rem, nchunks;
};

constexpr int kPqAdcAuxBytes = 128;           // behind the table: the waves' (min, second min) of two bins, the superbin records
constexpr int kPqAdcMaxPieces = 8;            // 16-byte pieces of a bin's codes per thread: 16 M / 256, M <= 128

// One workgroup per (scan chunk, query), 256 threads: thread t owns row t of every 256-row bin of the chunk, so the lanes
// [8 j, 8 j + 8) ([4 j, 4 j + 4)) of the workgroup are oct (quad) j of the bin.  Per bin: the group minimum is a butterfly over
// the group's lanes, the group's first lane packs the id, the bin's (min, second min) of the packed values is a butterfly of pairs
// over the wave and thread 0 merges the four waves through LDS, stores the bin record and folds it into the superbin (chunk,
// bin % G) -- the arithmetic of flush_bin (scan_x16.hpp).
// STAGED (M a multiple of 4, table + staging within the LDS budget): the bin's 256 M code bytes arrive by 16-byte loads, one bin
// ahead in registers, and are stored to LDS rows of an odd dword pitch.  Otherwise (M = 128: the table alone takes 128 KiB; M not
// a multiple of 4) a thread reads its row's codes from the index.
template <bool STAGED>
__global__ __launch_bounds__(256) void pq_adc_scan_kernel(PqAdcScanArgs a) {      // (capped at 128 VGPRs for 4 waves per SIMD it spills 3)
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_adc_lds[];
    float *T = reinterpret_cast<float *>(pq_adc_lds);
    float *red = reinterpret_cast<float *>(pq_adc_lds + (size_t)a.M * 1024);       // [2][4 waves][2]
    float *sbm = red + 16;                                                         // [G] min, [G] second min
    int *sbs = reinterpret_cast<int *>(sbm + 8);                                   // [G] span of the min
    unsigned char *stage = pq_adc_lds + (size_t)a.M * 1024 + kPqAdcAuxBytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x;
    const int64_t q = blockIdx.y;
    const int G = a.groups;
    const int64_t span0 = chunk_span0(chunk, a.spans_per_chunk, a.chunk_rem);
    int64_t span1 = chunk_span0(chunk + 1, a.spans_per_chunk, a.chunk_rem);
    if (span1 > a.nspans) span1 = a.nspans;
    const int64_t bin0 = span0 * G;
    const int nb = (int)(span1 - span0) * G;
    const float INF = __builtin_inff();
    {
        const float4 *src = reinterpret_cast<const float4 *>(a.tables + (size_t)q * a.M * 256);
        for (int i = tid; i < a.M * 64; i += 256) reinterpret_cast<float4 *>(T)[i] = src[i];
    }
    if (tid < 4) {
        sbm[tid] = INF;
        sbm[4 + tid] = INF;
        sbs[tid] = 0;
    }
    const float cs = a.info->cs;
    const int64_t total_bytes = a.N * a.M;
    const int npieces = 16 * a.M;                      // 16-byte pieces of a bin's codes
    uint4 pre[kPqAdcMaxPieces];
    auto fetch = [&](int64_t bin) {
        const int64_t byte0 = bin * 256 * a.M;
#pragma unroll
        for (int i = 0; i < kPqAdcMaxPieces; ++i) {
            const int p = tid + i * 256;
            pre[i] = make_uint4(0, 0, 0, 0);
            if (p < npieces && byte0 + (int64_t)p * 16 < total_bytes)      // (16 spare bytes behind the codes)
                pre[i] = *reinterpret_cast<const uint4 *>(a.codes + byte0 + (int64_t)p * 16);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < kPqAdcMaxPieces; ++i) {
            const int p = tid + i * 256;
            if (p < npieces) {
                const unsigned w[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
                int r = (p * 16) / a.M, o = p * 16 - r * a.M;
#pragma unroll
                for (int j = 0; j < 4; ++j) {       // (M is a multiple of 4: a dword never straddles two rows)
                    *reinterpret_cast<unsigned *>(stage + r * a.code_pitch + o) = w[j];
                    o += 4;
                    if (o >= a.M) {
                        o -= a.M;
                        ++r;
                    }
                }
            }
        }
    };
    const unsigned id = (unsigned)tid >> a.gshift;
    const bool leader = (tid & ((1 << a.gshift) - 1)) == 0;
    const bool dwords = (a.M & 3) == 0;
    if (STAGED) fetch(bin0);
    for (int i = 0; i < nb; ++i) {
        const int64_t bin = bin0 + i;
        if (STAGED) {
            store();
            if (i + 1 < nb) fetch(bin + 1);
        }
        if (STAGED || i == 0) __syncthreads();        // the staged codes (first trip: and the table) are in LDS
        const int64_t row = bin * 256 + tid;
        const float bv = a.bias[row];
        float s = kPadBias;
        if (!(bv >= 0.9e38f)) {
            const float s0 = bv * cs;
            if (STAGED) s = pq_adc_row_score<true>(T, stage + tid * a.code_pitch, a.M, s0);
            else if (dwords) s = pq_adc_row_score<true>(T, a.codes + (size_t)row * a.M, a.M, s0);
            else s = pq_adc_row_score<false>(T, a.codes + (size_t)row * a.M, a.M, s0);
        }
        // group minimum over the lanes of the oct / quad, then the wave's (min, second min) of the packed group minima
        s = __builtin_fminf(s, __shfl_xor(s, 1));
        s = __builtin_fminf(s, __shfl_xor(s, 2));
        if (a.gshift == 3) s = __builtin_fminf(s, __shfl_xor(s, 4));
        float v1 = leader ? pack_score(s, kQuadIdMask, id) : INF, v2 = INF;
        for (int o = 1 << a.gshift; o < 64; o <<= 1) {
            const float b1 = __shfl_xor(v1, o), b2 = __shfl_xor(v2, o);
            const float n2 = __builtin_fminf(__builtin_fmaxf(v1, b1), __builtin_fminf(v2, b2));
            v1 = __builtin_fminf(v1, b1);
            v2 = n2;
        }
        float *rd = red + (i & 1) * 8;
        if (lane == 0) {
            rd[2 * wave] = v1;
            rd[2 * wave + 1] = v2;
        }
        __syncthreads();                               // every thread has left the staged codes; the waves' pairs are in LDS
        if (tid == 0) {
            float b1 = rd[0], b2 = rd[1];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float c1 = rd[2 * w], c2 = rd[2 * w + 1];
                b2 = __builtin_fminf(__builtin_fmaxf(b1, c1), __builtin_fminf(b2, c2));
                b1 = __builtin_fminf(b1, c1);
            }
            a.bin_m1[(size_t)bin * a.Qpad + q] = b1;
            a.bin_m2[(size_t)bin * a.Qpad + q] = b2;
            const int g = (int)(bin & (G - 1));
            const float M1 = sbm[g], M2 = sbm[4 + g];
            sbm[4 + g] = __builtin_fminf(__builtin_amdgcn_fmed3f(M1, M2, b1), b2);
            if (b1 < M1) sbs[g] = (int)(bin / G);
            sbm[g] = __builtin_fminf(M1, b1);
        }
    }
    __syncthreads();                                   // (thread 0 folded the last bin behind the loop's last barrier)
    if (tid < G) {
        const size_t so = (size_t)(chunk * G + tid) * a.Qpad + q;
        a.sb_m1[so] = sbm[tid];
        a.sb_m2[so] = sbm[4 + tid];
        a.sb_span[so] = sbs[tid];
    }
}

// ---- test hook: raw scores ----------------------------------------------------------------------------------------------------
// grid (ceil(nrows / 256), nq): the scan's table in LDS, its per-row scoring function on the codes in the index
__global__ __launch_bounds__(256) void pq_adc_scores_kernel(PqAdcScanArgs a, int64_t row0, int64_t nrows, float *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_adc_lds[];
    float *T = reinterpret_cast<float *>(pq_adc_lds);
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.y;
    const float4 *src = reinterpret_cast<const float4 *>(a.tables + (size_t)q * a.M * 256);
    for (int i = tid; i < a.M * 64; i += 256) reinterpret_cast<float4 *>(T)[i] = src[i];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + tid;
    if (r >= nrows) return;
    const int64_t row = row0 + r;
    const float bv = a.bias[row];
    float s = kPadBias;
    if (!(bv >= 0.9e38f)) {
        const float s0 = bv * a.info->cs;
        if ((a.M & 3) == 0) s = pq_adc_row_score<true>(T, a.codes + (size_t)row * a.M, a.M, s0);
        else s = pq_adc_row_score<false>(T, a.codes + (size_t)row * a.M, a.M, s0);
    }
    out[(size_t)q * nrows + r] = s;
}

}  // namespace vdb

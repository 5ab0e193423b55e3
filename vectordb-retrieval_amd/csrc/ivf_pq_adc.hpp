// ivf_pq_adc.hpp -- the lookup-table (ADC) scan of the probed lists of an IVF<nlist>,PQ<M> index for small query batches
// (host side: ivf_pq.inc; admission: ivf_adc_plan, ivf_plan.hpp; contract, bound and measurements: DESIGN.md 4.4 "IVF-PQ ADC scan").
//
// The list-major path decodes the WHOLE index into fp16 panels per batch (D <= 128) and the exact list scan walks a float64
// chain per row and dimension (D > 128, every batch).  Here nothing is decoded.  x^[d] = fl32(c_l[d] + cb[m][code[m]][j]), so
//   q.x^ = q.c_l + sum_m q_m.cb[m][code_m]     up to the one float32 rounding per dimension inside x^
// and the sub-space terms do not depend on the list: ONE table per query -- the table pq_adc_tables_kernel builds -- serves every
// probed list, the centroid term is one scalar per (query, probe), L2 adds ||x^||^2 per row (n2, resident, 4 N bytes, made by the
// first admitted batch after an add).  Any D.  In scan units, cs a power of two chosen per batch, bs = -2 cs (L2) | -cs (IP):
//   T[q][m][c]  as pq_adc.hpp defines it
//   B[q][p]     = (float)(bs * acc),  acc = sum_d fma((double)q[d], (double)c_l[d], acc), d ascending from 0.0, l = probe p of query q
//   score(row)  = s_{M+1}:  s_0 = fl(cs * n2[row]) (L2: exact, cs is a power of two) | 0 (IP),  s_1 = s_0 + B,
//                 s_{m+2} = s_{m+1} + T[m][code[row][m]], m ascending -- plain float32 adds in that one order
// The scores of a query's probed rows land in one array (probe after probe, list order inside); the tail takes tau = the k-th smallest
// of them, re-scores the rows with s <= tau + 2 eps exactly (row_key: the float64 chain over x^ of every other path) and keeps the
// top k of those -- the argument of DESIGN 4.2.  A query with too many candidates, unusable scales or a non-finite score goes to
// ivf_scan_kernel (only_flagged), so the result is the exact list scan's whatever happens here.
#pragma once
#include "common.hpp"
#include "ivf_plan.hpp"
#include "pq_adc.hpp"
#include "refine.hpp"
#include "topk.hpp"

namespace vdb {

static_assert(kIvfAdcAuxBytes == kPqAdcAuxBytes, "the two ADC scans admit the same M");

// ---- the resident norms: n2[i] = (float) of the float64 chain over x^ of list-order row i, and the bits of their maximum -------------
// x^ by the float32 add of pq_key_body<true>; a padding dimension decodes to 0 and leaves the chain as it is.  The maximum is taken
// on the float32 bits (non-negative values order as unsigned integers; a NaN lands above every number and the host refuses the handle).
__global__ __launch_bounds__(256) void ivfpq_norms_kernel(IvfPqRows p, int64_t n, int D4, float *__restrict__ n2, unsigned *__restrict__ max_bits) {
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        const unsigned char *cr = p.pq.codes + (size_t)row * p.pq.M;
        const float *cl = p.cent + (size_t)p.list[row] * D4;
        double acc = 0.0;
        int d = 0;
        for (int m = 0; m < p.pq.M; ++m) {
            const float *cv = p.pq.cb + ((size_t)m * 256 + cr[m]) * p.pq.dsub;
            for (int j = 0; j < p.pq.dsub; ++j, ++d) {
                const double x = (double)(cl[d] + cv[j]);
                acc = fma(x, x, acc);
            }
        }
        const float v = (float)acc;
        n2[row] = v;
        atomicMax(max_bits, __float_as_uint(v));
    }
}

// ---- per batch: norms of the queries, the scale, the bounds, the flags, B and the score positions ------------------------------------
struct IvfPqAdcPrepArgs {
    const float *Q;               // [nq][D]
    const float *cent;            // [nlist][D4]
    const int64_t *probes;        // [nq][nprobe] list ids of the coarse search (-1 = none)
    const int64_t *offsets;       // [nlist + 1]
    int64_t nq;                   // <= kIvfAdcMaxBatch
    int D, D4, M, metric, nprobe, nlist;
    double Xn2, CR;               // max ||x^||^2 and Cn + Rn of the handle
    float *cs;                    // [1]
    float *eps;                   // [nq]
    int32_t *flag;                // [nq] 1: non-finite query or unusable scale -- the exact list scan serves the query
    float *B;                     // [nq][nprobe]
    int64_t *pos0;                // [nq][nprobe + 1] exclusive prefix of the probed lists' lengths; [nprobe] = the query's probed rows
};

// mag' of the bound: every partial sum of a score is at most cs mag' (1 + u) in magnitude
__device__ __forceinline__ double ivfpq_adc_mag(double qn2, int metric, double Xn2, double CR) {
    const double qn = sqrt(qn2);
    return metric == 0 ? Xn2 + 2.0 * qn * CR : qn * CR;
}
__device__ __forceinline__ bool ivfpq_adc_usable(double qn2, double mag) {
    return qn2 <= 1.0e300 && mag >= 1.0e-35 && mag <= 1.0e35;      // (false for NaN)
}
// eps = 1.02 cs (M + 4) 2^-23 mag' + 1e-30: more than twice the derived (M + 3) 2^-24 cs mag' (1 + O(u)); the 2 % and the clamp are
// query_eps_body's.  Nothing is packed into mantissa bits here, so there is no 2^-n term.
__device__ __forceinline__ float ivfpq_adc_eps(double mag, int M, double cs) {
    double e = 1.02 * cs * (double)(M + 4) * ldexp(1.0, -23) * mag;
    if (!(e < 1.0e37)) e = 1.0e37;
    return (float)e + 1.0e-30f;
}

// grid ceil(nq / 4), 256 threads.  Every workgroup takes the norms of ALL queries (one sequential float64 chain each: at most two
// per thread) and so the same scale, without a second dispatch; then wave w serves query 4 blockIdx.x + w, one lane per probe.
__global__ __launch_bounds__(256) void ivfpq_adc_prep_kernel(IvfPqAdcPrepArgs a) {
    __shared__ double s_n2[kIvfAdcMaxBatch], s_mag[kIvfAdcMaxBatch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = tid; q < a.nq; q += 256) {
        const float *row = a.Q + (size_t)q * a.D;
        double n2 = 0.0;
        for (int d = 0; d < a.D; ++d) n2 = fma((double)row[d], (double)row[d], n2);
        s_n2[q] = n2;
        s_mag[q] = ivfpq_adc_mag(n2, a.metric, a.Xn2, a.CR);
    }
    __syncthreads();
    double top = 0.0;
    for (int q = 0; q < a.nq; ++q)
        if (ivfpq_adc_usable(s_n2[q], s_mag[q])) top = fmax(top, s_mag[q]);
    const float cs = top > 0.0 ? (float)ldexp(1.0, -ilogb(top)) : 1.f;      // cs top in [1, 2)
    if (blockIdx.x == 0 && tid == 0) *a.cs = cs;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= a.nq) return;
    const double mag = s_mag[q];
    // (a query far below the batch's largest: its scores would leave the normal range of float32, where the bound is no longer relative;
    //  L2, a query 10^4 times longer than any row: ||q||^2 is no part of mag', and the float64 rounding of the exact keys, D 2^-53 of
    //  it, would no longer be small against the slack of the doubled bound -- DESIGN 4.4)
    const bool bad = !ivfpq_adc_usable(s_n2[q], mag) || (double)cs * mag < 1.0e-25 || (a.metric == 0 && s_n2[q] > 1.0e8 * a.CR * a.CR);
    if (lane == 0) {
        a.eps[q] = bad ? 0.f : ivfpq_adc_eps(mag, a.M, (double)cs);
        a.flag[q] = bad ? 1 : 0;
    }
    const double bs = (double)((a.metric == 0 ? -2.f : -1.f) * cs);
    const float *qv = a.Q + (size_t)q * a.D;
    int64_t carry = 0;
    for (int p0 = 0; p0 < a.nprobe; p0 += 64) {
        const int p = p0 + lane;
        int64_t l = p < a.nprobe ? a.probes[(size_t)q * a.nprobe + p] : -1;
        if (l >= a.nlist) l = -1;
        float b = 0.f;
        int64_t len = 0;
        if (l >= 0) {
            const float *cl = a.cent + (size_t)l * a.D4;
            double acc = 0.0;
            for (int d = 0; d < a.D; ++d) acc = fma((double)qv[d], (double)cl[d], acc);
            b = (float)(bs * acc);
            len = a.offsets[l + 1] - a.offsets[l];
        }
        int64_t incl = len;                                   // inclusive prefix over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (p < a.nprobe) {
            a.B[(size_t)q * a.nprobe + p] = b;
            a.pos0[(size_t)q * (a.nprobe + 1) + p] = carry + incl - len;
        }
        carry += __shfl(incl, 63);
    }
    if (lane == 0) a.pos0[(size_t)q * (a.nprobe + 1) + a.nprobe] = carry;
}

// ---- the scan ---------------------------------------------------------------------------------------------------------------------
struct IvfPqAdcScanArgs {
    const unsigned char *codes;   // [N][M] in list order, NO spare bytes behind the last row
    const float *n2;              // [N]
    const float *tables;          // [nq][M][256]
    const float *cs;              // [1]
    const float *B;               // [nq][nprobe]
    const int64_t *pos0;          // [nq][nprobe + 1]
    const int64_t *probes;        // [nq][nprobe]
    const int64_t *offsets;       // [nlist + 1]
    float *scores;                // [nq][stride]
    int64_t stride, N;
    int nprobe, nlist, M, metric, part_rows;
};

// grid (row parts of the longest list, nprobe, nq), 256 threads: the query's table in LDS (M KiB of dynamic LDS), thread t scores
// rows t, t + 256, ... of its part of the probed list.  Parts beyond the list's end leave before they touch the table.
// Bounds by construction: a code row is read inside its own M bytes only -- by dwords when M is a multiple of 4 (the row of every
// list is then 4-byte aligned; pq_adc_row_score<true> reads [cr, cr + M)), else byte by byte -- so no load passes N M; every gather
// index is 256 m + byte < 256 M; a list id outside [0, nlist) is no probe; a score position is checked against the query's stride.
__global__ __launch_bounds__(256) void ivfpq_adc_scan_kernel(IvfPqAdcScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_adc_lds[];
    float *T = reinterpret_cast<float *>(pq_adc_lds);
    const int tid = threadIdx.x;
    const int p = blockIdx.y;
    const int64_t q = blockIdx.z;
    const int64_t l = a.probes[(size_t)q * a.nprobe + p];
    if (l < 0 || l >= a.nlist) return;
    const int64_t lo = a.offsets[l];
    int64_t n = a.offsets[l + 1] - lo;
    if (n > a.N - lo) n = a.N - lo;
    const int64_t r0 = (int64_t)blockIdx.x * a.part_rows;
    if (r0 >= n) return;
    const int64_t r1 = r0 + a.part_rows < n ? r0 + a.part_rows : n;
    {
        const float4 *src = reinterpret_cast<const float4 *>(a.tables + (size_t)q * a.M * 256);
        for (int i = tid; i < a.M * 64; i += 256) reinterpret_cast<float4 *>(T)[i] = src[i];
    }
    __syncthreads();
    const float cs = *a.cs;
    const float b = a.B[(size_t)q * a.nprobe + p];
    const int64_t pos0 = a.pos0[(size_t)q * (a.nprobe + 1) + p];
    float *out = a.scores + (size_t)q * a.stride;
    const bool dwords = (a.M & 3) == 0;
    for (int64_t r = r0 + tid; r < r1; r += 256) {
        const int64_t row = lo + r;
        const float s0 = a.metric == 0 ? cs * a.n2[row] : 0.f;
        const float s1 = s0 + b;
        const unsigned char *cr = a.codes + (size_t)row * a.M;
        const float s = dwords ? pq_adc_row_score<true>(T, cr, a.M, s1) : pq_adc_row_score<false>(T, cr, a.M, s1);
        const int64_t pos = pos0 + r;
        if (pos < a.stride) out[pos] = s;
    }
}

// ---- the tail: threshold, candidates, exact keys, top-k ---------------------------------------------------------------------------------
struct IvfPqAdcTailArgs {
    RefineCommon c;               // ivfpq rows; Q = the queries padded to D4; idmap = the ids of the list-order rows
    const float *scores;          // [nq][stride]
    const float *eps;             // [nq]
    const int32_t *flag;          // [nq] of the prep kernel
    const int64_t *pos0, *probes, *offsets;
    int64_t stride;
    int nprobe, nlist, cand_cap;  // cand_cap <= kIvfAdcCandMax
    int32_t *fallback;            // [nq] out: 1 = the exact list scan serves the query (ivf_scan_kernel, only_flagged)
    unsigned long long *stat_counters;   // ws.small: [0] rows re-scored exactly, [2] flagged queries
    float *D; int64_t *I;         // final rows, or (D == nullptr) partial rows
    double *pk; int64_t *pi;
};

// One workgroup per query.  tau = the k-th smallest score of the query's P probed rows, by a radix select over the sortable bits (four
// passes of a 256-bin LDS histogram); +inf when P < k.  Candidates: s <= tau + 2 eps (compared in float64: the sum is exact there).
// The four waves take the exact keys of the candidates into LDS, wave 0 keeps their top k.  The order in which candidates are
// appended varies from run to run; the top k by (key, id) does not.
template <int KPL>
__global__ __launch_bounds__(256) void ivfpq_adc_tail_kernel(IvfPqAdcTailArgs a) {
    __shared__ unsigned s_hist[256];
    __shared__ int32_t s_cand[kIvfAdcCandMax];
    __shared__ uint64_t s_key[kIvfAdcCandMax];
    __shared__ unsigned s_sel, s_rank, s_wsum[4];
    __shared__ int s_ncand, s_bad;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t q = blockIdx.x;
    const int k = a.c.k;
    const int64_t *pos0 = a.pos0 + (size_t)q * (a.nprobe + 1);
    const int64_t P = pos0[a.nprobe];
    if (a.flag[q] || P > a.stride) {                          // (wave-uniform: the whole workgroup leaves)
        if (tid == 0) {
            a.fallback[q] = 1;
            stat_add(a.stat_counters, q, 2, 1ull);
        }
        return;
    }
    const float *sc = a.scores + (size_t)q * a.stride;
    if (tid == 0) {
        s_ncand = 0;
        s_bad = 0;
    }
    double thr = __builtin_inf();
    if (P >= k) {
        unsigned prefix = 0u, mask = 0u, rank = (unsigned)k;      // the rank-th smallest (1-based) among the scores whose masked bits equal prefix
        for (int shift = 24; shift >= 0; shift -= 8) {
            s_hist[tid] = 0u;
            __syncthreads();
            for (int64_t j0 = 0; j0 < P; j0 += 1024) {             // four loads in flight per thread, then their LDS atomics
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t j = j0 + i * 256 + tid;
                    v[i] = j < P ? sc[j] : 0.f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned u = sortable_u32(v[i]);
                    if (j0 + i * 256 + tid < P && (u & mask) == prefix) atomicAdd(&s_hist[(u >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            // the bin that holds the rank-th score: an inclusive prefix sum over the 256 counts (thread = bin), wave by wave
            const unsigned h = s_hist[tid];
            unsigned incl = h;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (lane == 63) s_wsum[tid >> 6] = incl;
            if (tid == 0) {                                        // (no bin can fail to qualify while P >= k; the last bin keeps tau an upper bound)
                s_sel = 255u;
                s_rank = 1u;
            }
            __syncthreads();
            for (int w = 0; w < (tid >> 6); ++w) incl += s_wsum[w];
            if (incl - h < rank && rank <= incl) {
                s_sel = (unsigned)tid;
                s_rank = rank - (incl - h);
            }
            __syncthreads();
            prefix |= s_sel << shift;
            mask |= 255u << shift;
            rank = s_rank;
        }
        thr = (double)unsortable_f32(prefix) + 2.0 * (double)a.eps[q];
    }
    __syncthreads();
    for (int64_t j0 = 0; j0 < P; j0 += 1024) {                     // candidates: their positions in the query's score array
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t j = j0 + i * 256 + tid;
            v[i] = j < P ? sc[j] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t j = j0 + i * 256 + tid;
            if (j >= P) continue;
            if (!(fabsf(v[i]) <= 3.0e38f)) s_bad = 1;              // NaN or infinite: no threshold means anything
            if ((double)v[i] <= thr) {
                const int c = atomicAdd(&s_ncand, 1);
                if (c < a.cand_cap) s_cand[c] = (int32_t)j;
            }
        }
    }
    __syncthreads();
    const int ncand = s_ncand;
    if (s_bad || ncand > a.cand_cap) {
        if (tid == 0) {
            a.fallback[q] = 1;
            stat_add(a.stat_counters, q, 2, 1ull);
        }
        return;
    }
    // position -> row: the probe p with pos0[p] <= j < pos0[p + 1] (the last p with pos0[p] <= j that holds rows), row = offsets[l] + j - pos0[p]
    for (int i = tid; i < ncand; i += 256) {
        const int64_t j = s_cand[i];
        int lo = 0, hi = a.nprobe;                                 // invariant: pos0[lo] <= j < pos0[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pos0[mid] <= j) lo = mid;
            else hi = mid;
        }
        s_cand[i] = (int32_t)(a.offsets[a.probes[(size_t)q * a.nprobe + lo]] + j - pos0[lo]);
    }
    __syncthreads();
    const float *qptr = a.c.Q + (size_t)q * a.c.D4;
    for (int i = tid; i < ncand; i += 256) s_key[i] = row_key<4>(a.c, s_cand[i], qptr);
    __syncthreads();
    if (tid >= 64) return;
    if (tid == 0) {
        a.fallback[q] = 0;
        stat_add(a.stat_counters, q, 0, (unsigned long long)ncand);
    }
    WaveTopK<KPL> tk;
    tk.init(k);
    for (int base = 0; base < ncand; base += 64) {
        const int i = base + lane;
        const bool valid = i < ncand;
        tk.offer(valid ? s_key[i] : ~0ull, valid ? a.c.idmap[s_cand[i]] : -1, valid);
    }
    const size_t o = (size_t)q * k;
    if (a.D) write_topk<KPL>(tk, a.c.metric, a.D + o, a.I + o, nullptr, nullptr);
    else write_topk<KPL>(tk, a.c.metric, nullptr, nullptr, a.pk + o, a.pi + o);
}

}  // namespace vdb

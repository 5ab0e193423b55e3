// ivf_sq8_scan.hpp -- IVF<nlist>,SQ8, option "ivf_sq8_direct": the list-major MFMA scan straight from the 8-bit codes (D <= 128).
//
// The fallback route widens the WHOLE panel space into fp16 panels per batch (ivf_sq8_panels_kernel) and runs scan_kernel on them.
// Here the codes are the A operand.  With g = vdiff / 255 and e = vmin + 128.5 g (a row's value at code 128), in real arithmetic
//     x^[d] = c_l[d] + e[d] + g[d] k[d],   k = code - 128 in [-128, 127]
//     q . x^ = q . c_l + q . e + sum_d (q[d] g[d]) k[d]
// so the score cs (||x^||^2 - 2 q . x^) (L2; IP: -cs q . x^) of scan_kernel splits into
//     accumulator init cs ||x^||^2      the resident bias of the panel space, as on every route
//   + sum_d B[d] k[d]                   the MFMAs: B = fp16(bs q[d] g[d]), bs = -2 cs | -cs; k exact in fp16
//   + T[slot]                           one float32 per (query, list) slot: bs (q . c_l + q . e), float64 rounded once
// under a per-batch power-of-two scale cs of its own (bs max|q| max g in [8192, 16384)).  T is added to a quad's minimum, not to its four
// scores: rounding is monotone, so min_i fl(a_i + T) = fl(min_i a_i + T) -- 8 adds per tile instead of 32.
// The bins leave exactly as scan_kernel's items mode writes them (quad ids, one 16-byte store per four bins and array), so the plan,
// ivf_select_kernel and ivf_tail_kernel run unchanged; eps is this route's own (DESIGN 4.4 "IVF-SQ8 direct scan").
//
// Codes into LDS: a tile's 32 MFMA rows are two runs of 16 consecutive list-order rows; global_load_lds lane (rho, kh) of piece p fetches
// the 16-byte chunk 2p + kh of row(rho) (ivf_sq8d_chunk_base) and lands at byte 16 * lane of the piece.  MFMA lane (rho, kh) then reads
// ITS 16 bytes with one ds_read_b128 at 16 * lane -- lane-linear, conflict free -- and uses bytes 0..7 in k-step 2p, 8..15 in 2p + 1: the
// K order inside a pair of k-steps is permuted, identically in the query operand (its rows are written in chunk order).
// Widening: v_perm_b32 with a 0x64 byte makes the fp16 1024 + code, v_pk_add_f16 takes 1152 off: 8 VALU per k-step pair and wave, in
// registers -- no second LDS pass, no barrier, and a stage is half the bytes of an fp16 one.
#pragma once
#include "common.hpp"
#include "ivf_mfma.hpp"
#include "ivf_sq8d_plan.hpp"
#include "scan.hpp"

namespace vdb {

typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// ---- per batch: scale, error bounds, query operand rows, per-list probe counts (replaces ivf_prep_kernel on this route) -----------
struct Sq8dPrepArgs {
    // workgroups [0, n_eps_blocks): error bounds and q . e; [.., + n_row_blocks): operand rows; the rest: ivf_count_body
    const int64_t *probes;
    int64_t npairs;
    int nlist, ppb;
    int32_t *cnt;
    unsigned n_eps_blocks, n_row_blocks;
    const float *Q;               // [nq][D]
    int64_t nq;
    int D, D4, Dpad, metric;
    const float *vmin, *vdiff;    // [D4], zero padded
    _Float16 *wrows;              // [nq][Dpad]: element 16 c + j = fp16(bs q[d] g[d]), d = ivf_sq8d_chunk_dim(c, j), else 0
    float *eps;                   // [nq]
    double *qterm;                // [nq] q . e
    QueryBatchInfo *info;         // published by workgroup 0: cs, bscale, force_fallback of THIS route
    const QueryBatchInfo *src;    // statistics of the same queries taken by the coarse index, or nullptr (info holds them)
    // of the handle (sq8d_constants, ivf_sq8.inc)
    float gmax, camax;            // max g, max |c_l[d]| + max |e[d]|
    double dec_norm, can;         // || |c|max + 2 |vmin| + 4.2 vdiff ||, max_l ||c_l + e||
    float xnorm_max, maxnorm2;
    int consts_ok;
};

// the scale of the batch and whether the route can serve it, from the batch statistics: the windows of query_finalize_values, applied
// to w = q g and to the slot term.  Deterministic, so every workgroup gets the same answer
__device__ inline void sq8d_finalize(QueryBatchInfo *info, const Sq8dPrepArgs &a) {
    const float amax = __uint_as_float(info->absmax_bits);
    const float fm = a.metric == 0 ? 2.f : 1.f;
    const float wmax = fm * amax * a.gmax;
    bool ok = a.consts_ok && !info->nonfinite && amax <= 3.0e38f;
    float cs = 1.f;
    if (wmax > 0.f && wmax <= 3.0e38f) {
        int e;
        frexpf(wmax, &e);
        cs = ldexpf(1.f, 14 - e);           // wmax cs in [8192, 16384)
    } else if (amax > 0.f && a.gmax > 0.f) {
        ok = false;                         // the product left float32
    }
    ok = ok && cs > 1.0e-30f && cs < 1.0e30f && wmax * cs <= 65504.f;
    ok = ok && cs * a.maxnorm2 < 1.0e30f && a.maxnorm2 < 0.9e38f;
    ok = ok && cs * fm * (float)a.D * amax * (a.camax + 128.f * a.gmax) < 1.0e30f;      // the slot term (a NaN fails the test)
    info->sq = cs;
    info->cs = cs;
    info->bscale = -fm * cs;
    info->i8_mode = 0;
    info->force_fallback = ok ? 0 : 1;
}

// the query operand of one dimension: t = bs q g in float64 (exact up to 2^-52), rounded to float32, then to fp16
__device__ __forceinline__ _Float16 sq8d_operand(float q, float vdiff, double bs, double &t) {
    t = bs * ((double)q * ((double)vdiff / 255.0));
    return (_Float16)(float)t;
}

// KLOOP: the operand rows in the K order of the D > 128 scan (ivf_sq8_kloop.hpp, ivf_sq8k_operand_dim) instead of chunk order
template <bool KLOOP>
__device__ __forceinline__ void sq8d_prep_body(const Sq8dPrepArgs &a) {
    extern __shared__ int ivf_hist[];
    __shared__ QueryBatchInfo s_info;
    if (blockIdx.x >= a.n_eps_blocks + a.n_row_blocks) {
        ivf_count_body((int)(blockIdx.x - a.n_eps_blocks - a.n_row_blocks), a.ppb, a.probes, a.npairs, a.nlist, a.cnt, ivf_hist);
        return;
    }
    if (threadIdx.x == 0) {
        s_info = a.src ? *a.src : *a.info;
        sq8d_finalize(&s_info, a);
        if (blockIdx.x == 0) *a.info = s_info;
    }
    __syncthreads();
    if (s_info.force_fallback) {            // flagged whole: nothing below is read (eps only has to be a number)
        const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (blockIdx.x < a.n_eps_blocks && q < a.nq) {
            a.eps[q] = 1.0e37f;
            a.qterm[q] = 0.0;
        }
        return;
    }
    const double cs = (double)s_info.cs, bs = (double)s_info.bscale;
    if (blockIdx.x >= a.n_eps_blocks) {     // operand rows: 8 consecutive elements (half a chunk) per thread
        const int64_t i8 = ((int64_t)(blockIdx.x - a.n_eps_blocks) * 256 + threadIdx.x) * 8;
        if (i8 >= a.nq * a.Dpad) return;
        const int64_t q = i8 / a.Dpad;
        const int e0 = (int)(i8 - q * a.Dpad), c = e0 >> 4, j0 = e0 & 15;
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = KLOOP ? ivf_sq8k_operand_dim(e0 + j, a.D, a.D4) : ivf_sq8d_chunk_dim(c, j0 + j, a.D, a.D4);
            double t;
            o[j] = d < 0 ? (_Float16)0.f : sq8d_operand(a.Q[(size_t)q * a.D + d], a.vdiff[d], bs, t);
        }
        *reinterpret_cast<half8 *>(a.wrows + i8) = o;
        return;
    }
    // error bounds: 16 lanes per query
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t q = gid >> 4;
    const int part = (int)(gid & 15);
    double n2 = 0.0, w1 = 0.0, rerr = 0.0, qe = 0.0;
    if (q < a.nq)
        for (int d = part; d < a.D; d += 16) {
            const float v = a.Q[(size_t)q * a.D + d];
            const double g = (double)a.vdiff[d] / 255.0;
            double t;
            const _Float16 b = sq8d_operand(v, a.vdiff[d], bs, t);
            n2 = fma((double)v, (double)v, n2);
            w1 += fabs((double)v * g);
            rerr += fabs((double)(float)b - t);          // what the fp16 operand really lost, subnormal steps included
            qe = fma((double)v, (double)a.vmin[d] + 128.5 * g, qe);
        }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        n2 += __shfl_xor(n2, o);
        w1 += __shfl_xor(w1, o);
        rerr += __shfl_xor(rerr, o);
        qe += __shfl_xor(qe, o);
    }
    if (q >= a.nq || part != 0) return;
    // DESIGN 4.4 "IVF-SQ8 direct scan", in key units (times cs at the end)
    const double qn = sqrt(n2), Xn = (double)a.xnorm_max, f = a.metric == 0 ? 2.0 : 1.0;
    const double x2 = a.metric == 0 ? Xn * Xn : 0.0;
    const double mag = x2 + f * (256.0 * w1 + qn * a.can);               // |bias| + |MFMA terms| + |slot term|
    const double dec_err = f * ldexp(1.0, -24) * qn * a.dec_norm;        // x^ against its affine form: the float32 roundings of sq8_decode
    const double w_err = 128.0 * rerr / cs;                              // fp16 operand, times the largest |k|
    const double acc_err = (double)(a.Dpad + 4) * ldexp(1.0, -23) * mag; // fp32 accumulation, the slot add included
    const double slot_err = (ldexp(1.0, -24) + ldexp(1.0, -40)) * mag;   // the slot term rounded once (and its float64 sums)
    const double pack_err = ldexp(1.0, -17) * (x2 + f * qn * Xn);        // 6 mantissa bits carry the quad id
    const double bias_err = ldexp(1.0, -24) * x2;
    const double key_err = key64_round_err(a.metric, a.D, qn, Xn);
    double e = cs * (dec_err + w_err + acc_err + slot_err + pack_err + bias_err + key_err) * 1.02;
    if (!(e < 1.0e37)) e = 1.0e37;
    a.eps[q] = (float)e + 1.0e-30f;
    a.qterm[q] = qe;
}
__global__ __launch_bounds__(256) void ivf_sq8d_prep_kernel(Sq8dPrepArgs a) { sq8d_prep_body<false>(a); }

// ---- per batch, after the plan: the slot terms.  16 lanes per (query, probe) pair ---------------------------------------------------
struct Sq8dSlotArgs {
    const int64_t *probes;        // [nq][nprobe]
    const int32_t *slot_of;       // [nq][nprobe], -1: the pair owns no slot
    int64_t npairs;
    int nprobe, nlist, D4, metric;
    const float *qpad;            // [nq][D4] zero padded
    const float *cent;            // [nlist][D4] zero padded
    const double *qterm;
    const QueryBatchInfo *info;
    float *slot_term;             // [slots]
};
__global__ __launch_bounds__(256) void ivf_sq8d_slot_kernel(Sq8dSlotArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = gid >> 4;
    const int part = (int)(gid & 15);
    if (a.info->force_fallback) return;
    int slot = -1;
    int64_t l = -1;
    if (i < a.npairs) {
        slot = a.slot_of[i];
        l = a.probes[i];
    }
    const bool on = slot >= 0 && l >= 0 && l < a.nlist;
    const int64_t q = on ? i / a.nprobe : 0;
    double dot = 0.0;
    if (on)
        for (int d = part; d < a.D4; d += 16) dot = fma((double)a.qpad[(size_t)q * a.D4 + d], (double)a.cent[(size_t)l * a.D4 + d], dot);
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) dot += __shfl_xor(dot, o);
    if (on && part == 0) a.slot_term[slot] = (float)((double)a.info->bscale * (dot + a.qterm[q]));
}

// ---- the scan -------------------------------------------------------------------------------------------------------------------------
struct Sq8dScanArgs {
    const unsigned char *codes;   // [N][D4], list order
    int D4;
    const int32_t *span_row0, *span_valid;      // [pspans] first list-order row / valid rows of every panel span
    const float *bias;            // [pspans * 256] ||x^||^2 (L2) | 0 (IP) | the pad marker
    const _Float16 *wrows;        // [nq][16 KSTEPS] operand rows
    const float *slot_term;       // [slots]
    const QueryBatchInfo *info;
    float *bin_m1, *bin_m2, *bin_m3;
    const int32_t *item_list, *item_slot0, *item_bin0, *n_items, *list_pspan0, *slot_query;
    int part_spans;
};

// two code dwords (8 bytes) -> 8 fp16 values code - 128
__device__ __forceinline__ half8 sq8d_widen(unsigned lo, unsigned hi) {
    const unsigned k64 = 0x64646464u;
    const half2v off = {(_Float16)1152.f, (_Float16)1152.f};
    const half2v p0 = __builtin_bit_cast(half2v, __builtin_amdgcn_perm(k64, lo, 0x04010400u)) - off;
    const half2v p1 = __builtin_bit_cast(half2v, __builtin_amdgcn_perm(k64, lo, 0x04030402u)) - off;
    const half2v p2 = __builtin_bit_cast(half2v, __builtin_amdgcn_perm(k64, hi, 0x04010400u)) - off;
    const half2v p3 = __builtin_bit_cast(half2v, __builtin_amdgcn_perm(k64, hi, 0x04030402u)) - off;
    half8 r;
    r[0] = p0[0]; r[1] = p0[1]; r[2] = p1[0]; r[3] = p1[1]; r[4] = p2[0]; r[5] = p2[1]; r[6] = p3[0]; r[7] = p3[1];
    return r;
}

// A fragments and accumulator init of one tile: one 16-byte LDS read per pair of k-steps, widened in registers
template <int KSTEPS>
__device__ __forceinline__ void sq8d_read_phase(const unsigned char *__restrict__ A_tile, const float4 *__restrict__ c_tile,
                                                half8 (&fr)[KSTEPS], float16v &cin, int lane) {
#pragma unroll
    for (int p = 0; p < KSTEPS / 2; ++p) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(A_tile + p * 1024 + lane * 16);
        fr[2 * p] = sq8d_widen(raw.x, raw.y);
        fr[2 * p + 1] = sq8d_widen(raw.z, raw.w);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 c = c_tile[g];
        cin[4 * g + 0] = c.x; cin[4 * g + 1] = c.y; cin[4 * g + 2] = c.z; cin[4 * g + 3] = c.w;
    }
}

// select_phase<M3> of scan.hpp with the slot term of the lane's two columns added to every quad minimum
__device__ __forceinline__ void sq8d_select_phase(const float16v &acc0, const float16v &acc1, float (&m1)[2], float (&m2)[2],
                                                  float (&m3)[2], unsigned idmask, float neg_inf, unsigned id0, float t0, float t1) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float q0 = quad_min(acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3], neg_inf) + t0;
        const float v0 = pack_score(q0, idmask, id0 + g);
        m3[0] = __builtin_amdgcn_fmed3f(m2[0], m3[0], v0);
        m2[0] = __builtin_amdgcn_fmed3f(m1[0], m2[0], v0);
        m1[0] = fast_min(m1[0], v0, neg_inf);
        const float q1 = quad_min(acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3], neg_inf) + t1;
        const float v1 = pack_score(q1, idmask, id0 + g);
        m3[1] = __builtin_amdgcn_fmed3f(m2[1], m3[1], v1);
        m2[1] = __builtin_amdgcn_fmed3f(m1[1], m2[1], v1);
        m1[1] = fast_min(m1[1], v1, neg_inf);
    }
}

// One workgroup = (list) x (64 NWAVES query slots) x (row part), as scan_kernel's items mode: same spans, stages of ST = 2 tiles, bins of
// BT tiles per lane half, early / late wave halves (scan.hpp, "Phase stagger"), same bin layout.
template <int KSTEPS, int NWAVES, int BT>
__global__ __launch_bounds__(NWAVES * 64, 2) void ivf_sq8_scan_kernel(Sq8dScanArgs a) {
    constexpr int NT = NWAVES * 64, ST = kSq8dStageTiles, TPS = kIvfTilesPerSpan;
    constexpr int HK = KSTEPS / 2;                          // 1-KiB pieces (pairs of k-steps) per tile
    constexpr int kPieces = ST * HK, kStageBytes = kPieces * 1024;
    constexpr int kBiasLoads = (ST * 32 + NT - 1) / NT;
    constexpr int kSpanR = TPS * 32, kHalfR = TPS * 16, SPS = TPS / ST, BPS = TPS / BT;
    static_assert(KSTEPS % 2 == 0 && TPS % BT == 0 && BT % ST == 0, "bad geometry");
    static_assert(2 * (kStageBytes + ST * 32 * 4) == ivf_sq8d_lds_bytes(KSTEPS), "the plan's LDS bytes");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (kStageBytes + ST * 32 * 4)];
    auto lds_a = [&](int buf) { return smem + buf * kStageBytes; };
    auto lds_b = [&](int buf) { return reinterpret_cast<float *>(smem + 2 * kStageBytes + buf * (ST * 32 * 4)); };
    if (a.info->force_fallback) return;                     // flagged whole: the select reads no bin

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const bool late = wave >= NWAVES / 2;
    const int it = blockIdx.x;
    if (it >= *a.n_items) return;
    const int l = a.item_list[it];
    int64_t span0 = a.list_pspan0[l], span1 = a.list_pspan0[l + 1];
    const int64_t lspan0 = span0, lspans = span1 - span0;
    if (a.part_spans > 0) {
        span0 += (int64_t)blockIdx.y * a.part_spans;
        if (span0 >= span1) return;
        if (span0 + a.part_spans < span1) span1 = span0 + a.part_spans;
    }
    const int64_t q0 = (int64_t)a.item_slot0[it] + wave * 64;
    const int64_t out_pitch = NWAVES * 64, out_col = wave * 64 + (lane & 31);
    const size_t bin_base = (size_t)a.item_bin0[it];
    const float cs = a.info->cs;
    const int qa = a.slot_query[q0 + (lane & 31)] - 1, qb = a.slot_query[q0 + 32 + (lane & 31)] - 1;

    const int nstages = (int)(span1 - span0) * SPS;
    const int nb_half = ((int)lspans * BPS + 3) & ~3, nb_item = 2 * nb_half;
    const float INF = __builtin_inff();
    float NEG_INF = -INF;
    asm volatile("" : "+v"(NEG_INF));
    unsigned idmask = kQuadIdMask;
    asm volatile("" : "+v"(idmask));
    float m1[2] = {INF, INF}, m2[2] = {INF, INF}, m3[2] = {INF, INF};

    // ---- staging: DMA lane (rho, kh) of piece (tile tt, pair p) fetches chunk 2p + kh of the row MFMA row rho of the tile stands for;
    //      a padding row (its bias is the pad marker) reads the span's first row instead -- never past the codes
    const int rho = lane & 31;
    const int loc0 = ((rho >> 2) & 1) * kHalfR + ((rho & 3) | ((rho >> 3) << 2));     // local row of MFMA row rho in tile 0 of a span
    float stage_b[kBiasLoads];
    auto stage_issue = [&](int st, int buf) {
        const int64_t span = span0 + st / SPS;
        const int sq = st % SPS;
        const int row0 = a.span_row0[span], valid = a.span_valid[span];
#pragma unroll
        for (int i = 0; i < (kPieces + NWAVES - 1) / NWAVES; ++i) {
            const int pc = wave + i * NWAVES;
            if (pc < kPieces) {
                const int tt = pc / HK, p = pc % HK;
                const int local = loc0 + (sq * ST + tt) * 16;
                const unsigned char *g = a.codes + (size_t)(row0 + (local < valid ? local : 0)) * a.D4 + ivf_sq8d_chunk_base(2 * p + h, a.D4);
                __builtin_amdgcn_global_load_lds(
                    reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(g)),
                    reinterpret_cast<__attribute__((address_space(3))) void *>(
                        static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_a(buf) + pc * 1024))),
                    16, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < kBiasLoads; ++i) {
            const int e = tid + i * NT;
            if (e < ST * 32) {
                const int t = e >> 5, hh = (e >> 4) & 1, r = e & 15;
                stage_b[i] = a.bias[span * kSpanR + hh * kHalfR + (sq * ST + t) * 16 + r];
            }
        }
    };
    auto stage_bias_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kBiasLoads; ++i)
            if (tid + i * NT < ST * 32) lds_b(buf)[tid + i * NT] = (stage_b[i] >= 0.9e38f) ? kPadBias : stage_b[i] * cs;
    };
    // the bins of a lane: one run per lane half, four bins per 16-byte store (scan.hpp, items_push)
    float4 pend1[2], pend2[2], pend3[2];
    auto items_push = [&](int r) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            pend1[cb] = make_float4(pend1[cb].y, pend1[cb].z, pend1[cb].w, m1[cb]);
            pend2[cb] = make_float4(pend2[cb].y, pend2[cb].z, pend2[cb].w, m2[cb]);
            pend3[cb] = make_float4(pend3[cb].y, pend3[cb].z, pend3[cb].w, m3[cb]);
            m1[cb] = INF;
            m2[cb] = INF;
            m3[cb] = INF;
        }
        if ((r & 3) == 3) {
            const size_t o4 = bin_base * out_pitch + (size_t)out_col * nb_item + (size_t)(h * nb_half + r - 3);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                *reinterpret_cast<float4 *>(a.bin_m1 + o4 + (size_t)cb * 32 * nb_item) = pend1[cb];
                *reinterpret_cast<float4 *>(a.bin_m2 + o4 + (size_t)cb * 32 * nb_item) = pend2[cb];
                *reinterpret_cast<float4 *>(a.bin_m3 + o4 + (size_t)cb * 32 * nb_item) = pend3[cb];
            }
        }
    };
    auto flush_bin = [&](int64_t span, int bt) { items_push((int)(span - lspan0) * BPS + bt); };

    stage_issue(0, 0);
    // the slots' operand rows and slot terms, behind the first stage: lane (col, kh) reads chunk 2p + kh of its slot's row
    half8 b0[KSTEPS], b1[KSTEPS];
    float t0 = 0.f, t1 = 0.f;
    {
        const half8 *ra = reinterpret_cast<const half8 *>(a.wrows + (size_t)(qa < 0 ? 0 : qa) * (16 * KSTEPS)) + 2 * h;
        const half8 *rb = reinterpret_cast<const half8 *>(a.wrows + (size_t)(qb < 0 ? 0 : qb) * (16 * KSTEPS)) + 2 * h;
        half8 zero;
#pragma unroll
        for (int j = 0; j < 8; ++j) zero[j] = (_Float16)0.f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int o = (ks >> 1) * 4 + (ks & 1);         // half8 index of (chunk 2p + kh, half ks & 1), less the 2 kh above
            b0[ks] = qa < 0 ? zero : ra[o];
            b1[ks] = qb < 0 ? zero : rb[o];
        }
        if (qa >= 0) t0 = a.slot_term[q0 + (lane & 31)];
        if (qb >= 0) t1 = a.slot_term[q0 + 32 + (lane & 31)];
    }
    stage_bias_store(0);
    __syncthreads();

    if (__ballot(qa >= 0 || qb >= 0) == 0ull) {             // a wave of padding slots only keeps the staging and the barriers going
        for (int st = 0; st < nstages; ++st) {
            if (st + 1 < nstages) {
                stage_issue(st + 1, (st & 1) ^ 1);
                stage_bias_store((st & 1) ^ 1);
            }
            __syncthreads();
        }
        return;
    }

    half8 fr[KSTEPS];
    float16v cin, acc0, acc1;
    if (!late) {        // early half: MFMA(t), then select(t)
        for (int st = 0; st < nstages; ++st) {
            const int buf = st & 1;
            if (st + 1 < nstages) stage_issue(st + 1, buf ^ 1);
            const unsigned char *A = lds_a(buf);
            const float4 *B4 = reinterpret_cast<const float4 *>(lds_b(buf)) + h * 4;
            const int ts0 = (st % SPS) * ST;
            sq8d_read_phase<KSTEPS>(A, B4, fr, cin, lane);
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                __builtin_amdgcn_sched_barrier(0);
                mfma_phase<KSTEPS>(fr, b0, b1, cin, acc0, acc1);
                __builtin_amdgcn_sched_barrier(0);
                if (t + 1 < ST) sq8d_read_phase<KSTEPS>(A + (t + 1) * HK * 1024, B4 + (t + 1) * 8, fr, cin, lane);
                sq8d_select_phase(acc0, acc1, m1, m2, m3, idmask, NEG_INF, (unsigned)(((ts0 + t) % BT) << 2), t0, t1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (((ts0 + ST) % BT) == 0) flush_bin(span0 + st / SPS, (ts0 + ST) / BT - 1);
            if (st + 1 < nstages) stage_bias_store(buf ^ 1);
            __syncthreads();
        }
    } else {            // late half: select(t - 1), then MFMA(t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = 3.0e38f;     // dummy "previous tile": can never win
        acc1 = acc0;
        for (int st = 0; st < nstages; ++st) {
            const int buf = st & 1;
            if (st + 1 < nstages) stage_issue(st + 1, buf ^ 1);
            const unsigned char *A = lds_a(buf);
            const float4 *B4 = reinterpret_cast<const float4 *>(lds_b(buf)) + h * 4;
            const int ts0 = (st % SPS) * ST;
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                __builtin_amdgcn_sched_barrier(0);
                sq8d_read_phase<KSTEPS>(A + t * HK * 1024, B4 + t * 8, fr, cin, lane);
                const int tp = (ts0 + t + TPS - 1) % TPS;
                sq8d_select_phase(acc0, acc1, m1, m2, m3, idmask, NEG_INF, (unsigned)((tp % BT) << 2), t0, t1);
                if (t == 0 && st > 0 && (ts0 % BT) == 0) flush_bin(span0 + (st * ST - 1) / TPS, tp / BT);
                __builtin_amdgcn_sched_barrier(0);
                mfma_phase<KSTEPS>(fr, b0, b1, cin, acc0, acc1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (st + 1 < nstages) stage_bias_store(buf ^ 1);
            __syncthreads();
        }
        sq8d_select_phase(acc0, acc1, m1, m2, m3, idmask, NEG_INF, (unsigned)((BT - 1) << 2), t0, t1);
        flush_bin(span1 - 1, BPS - 1);
    }
    for (int r = (int)(span1 - lspan0) * BPS; r & 3; ++r) items_push(r);      // fill the last vector of this part's run
}

}  // namespace vdb

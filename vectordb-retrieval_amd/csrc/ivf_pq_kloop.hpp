// ivf_pq_kloop.hpp -- IVF<nlist>,PQ<M>, option "ivf_pq_kloop": the K-loop list scan straight from the product codes for D > 128.
//
// x^[d] = fl32(c_l[d] + cb[m][code[m]][j]).  Every row of a work item lies in ONE list, so the centroid part leaves the MFMA as it does
// on the SQ8 routes (ivf_sq8_scan.hpp): the score cs (||x^||^2 - 2 q . x^) (L2; IP: -cs q . x^) splits into
//     accumulator init cs ||x^||^2      the resident bias of the panel space, as on every route
//   + sum_p B[p] T[p]                   the MFMAs over the residual part: T = fp16(ts cb) from the handle's table, B = fp16(bs q / ts),
//                                       bs = -2 cs | -cs, ts a power of two of the handle (max |T| in [128, 256))
//   + S[slot]                           one float32 per (query, list) slot: bs (q . c_l), float64 rounded once (ivf_sq8d_slot_kernel),
//                                       added to the minimum of a candidate group before it is packed (rounding is monotone)
// under a per-batch power-of-two scale cs of this route (max |B| in [8192, 16384)).  eps is the route's own: DESIGN 4.4 "IVF-PQ K-loop scan".
//
// The operands live in the padded space of ivf_pq_kloop_plan.hpp: sub-space m owns the P = 8 ceil(dsub / 8) operand dimensions
// [m P, (m + 1) P), zero beyond dsub, so every 8-element A fragment is one aligned 16-byte piece of one entry of T[m][256][P] (512 KiB at
// 768 dims / PQ64: it lives in L2).  Work split, bins, 6-bit ids, candidate groups and the [item][slot][bin] output are those of
// ivf_kloop_scan_kernel (ivf_kloop.hpp): work item = one list x 512 query slots, 8 waves x 64 slots, blockIdx.y = row part, one pass =
// 8 tiles x 4 column blocks on v_mfma_f32_16x16x32_f16, B gathered per K-step through a buffer descriptor -- the plan, ivf_select_kernel
// and ivf_tail_kernel run unchanged.  What is new is how A arrives:
//   codes     the codes of a pass are 128 list-order rows x M bytes.  Wave w stages the 16 rows of ITS tile w (the p16 row mapping -- MFMA
//             row 4g + i of tile t <-> local row (4 TPS) g + 4 t + i of the span -- applied here; a padding row reads the span's first
//             row, its accumulator init is kPadBias) into LDS one pass ahead of use: 16 lanes walk the 4 M contiguous bytes of four
//             consecutive rows.  Two passes are resident; a wave reads only what it wrote, so a wave barrier orders it.
//   gather    a tile k-step is 16 rows x 32 operand dims of fp16 = 1 KiB = ONE global_load_lds of 16 bytes per lane with per-lane
//             addresses: lane (row r = lane & 15, quarter kq = lane >> 4) reads the code byte of its row and of the sub-space m of piece
//             pc = 4 (k-step) + kq from LDS, forms T + ((m 256 + code) P + 8 sub) 2 and its piece lands at byte 16 lane of the tile: the
//             gather from the table IS the staging.  A piece at or behind Kp reads piece 0 of the table against a zero operand.  The
//             two code bytes of a lane are read (into one register) one K-step before the load is issued, which is BS K-steps
//             before its use, so no LDS latency sits between the MFMAs and the loads.  Wave w gathers tile w; all 8 waves consume
//             all 8 tiles.  (256 VGPRs and 68 bytes of scratch per lane, none of it inside the K-step loop: DESIGN 4.4.)
//   MFMA      every lane reads its fragment with one ds_read_b128, lane-linear, exactly as ivf_kloop_scan_kernel reads its panels.
// Stage ring and barrier placement are those of ivf_kloop_scan_kernel (2 BS stages of 16 KiB, one barrier per BS K-steps); ring depth,
// code pitch CP and the LDS bytes: ivf_pq_kloop_plan.hpp.
#pragma once
#include "ivf_pq_kloop_plan.hpp"
#include "ivf_sq8_scan.hpp"
#include "scan16.hpp"

namespace vdb {

// ---- per batch: scale, error bounds, query operand rows, per-list probe counts (replaces ivf_prep_kernel on this route) -----------
struct PqkPrepArgs {
    // workgroups [0, n_eps_blocks): error bounds; [.., + n_row_blocks): operand rows; the rest: ivf_count_body
    const int64_t *probes;
    int64_t npairs;
    int nlist, ppb;
    int32_t *cnt;
    unsigned n_eps_blocks, n_row_blocks;
    const float *Q;               // [nq][D]
    int64_t nq;
    int D, Kpad, M, dsub, metric; // Kpad = 64 nk operand positions per row
    const float *dimc;            // [3][D] per dimension: max |T| / ts over the 256 entries | max |T / ts - cb| | max_l |c_l| + max |cb|
    _Float16 *wrows;              // [nq][Kpad]: position p = fp16(bs q[d] / ts), d = ivf_pqk_operand_dim(p), else 0
    float *eps;                   // [nq]
    double *qterm;                // [nq] zero: the slot term of this route is bs (q . c_l) alone (ivf_sq8d_slot_kernel adds qterm)
    QueryBatchInfo *info;         // published by workgroup 0: cs, bscale, force_fallback of THIS route
    const QueryBatchInfo *src;    // statistics of the same queries taken by the coarse index, or nullptr (info holds them)
    // of the handle (ivfpqk_build_space, ivf_pq.inc)
    double ts, can;               // scale of the table (a power of two); max_l ||c_l||
    float camax, rmax;            // max |c_l[d]|, max |cb|
    float xnorm_max, maxnorm2;
    int consts_ok;
};

// the scale of the batch and whether the route can serve it: the windows of sq8d_finalize with 1 / ts in the place of max g
__device__ inline void pqk_finalize(QueryBatchInfo *info, const PqkPrepArgs &a) {
    const float amax = __uint_as_float(info->absmax_bits);
    const float fm = a.metric == 0 ? 2.f : 1.f;
    const float tinv = (float)(1.0 / a.ts);
    const float wmax = fm * amax * tinv;
    bool ok = a.consts_ok && !info->nonfinite && amax <= 3.0e38f;
    float cs = 1.f;
    if (wmax > 0.f && wmax <= 3.0e38f) {
        int e;
        frexpf(wmax, &e);
        cs = ldexpf(1.f, 14 - e);           // wmax cs in [8192, 16384)
    } else if (amax > 0.f) {
        ok = false;                         // the product left float32
    }
    ok = ok && cs > 1.0e-30f && cs < 1.0e30f && wmax * cs <= 65504.f;
    ok = ok && cs * a.maxnorm2 < 1.0e30f && a.maxnorm2 < 0.9e38f;
    ok = ok && cs * fm * (float)a.D * amax * (a.camax + a.rmax) < 1.0e30f;      // the slot term and the MFMA sum (a NaN fails the test)
    info->sq = cs;
    info->cs = cs;
    info->bscale = -fm * cs;
    info->i8_mode = 0;
    info->force_fallback = ok ? 0 : 1;
}

// the query operand of one dimension: t = bs q / ts in float64 (exact: ts is a power of two), rounded to float32, then to fp16
__device__ __forceinline__ _Float16 pqk_operand(float q, double bs_ts, double &t) {
    t = bs_ts * (double)q;
    return (_Float16)(float)t;
}

// DIRECT: the operand rows in plain dimension order, Kpad = 16 KSTEPS (the D <= 128 scan, ivf_pq_scan.hpp) instead of the padded space
template <bool DIRECT>
__device__ __forceinline__ void pqk_prep_body(const PqkPrepArgs &a) {
    extern __shared__ int ivf_hist[];
    __shared__ QueryBatchInfo s_info;
    if (blockIdx.x >= a.n_eps_blocks + a.n_row_blocks) {
        ivf_count_body((int)(blockIdx.x - a.n_eps_blocks - a.n_row_blocks), a.ppb, a.probes, a.npairs, a.nlist, a.cnt, ivf_hist);
        return;
    }
    if (threadIdx.x == 0) {
        s_info = a.src ? *a.src : *a.info;
        pqk_finalize(&s_info, a);
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
    const double cs = (double)s_info.cs, bs_ts = (double)s_info.bscale / a.ts;
    if (blockIdx.x >= a.n_eps_blocks) {     // operand rows: 8 consecutive positions per thread (one piece: inside one sub-space)
        const int64_t i8 = ((int64_t)(blockIdx.x - a.n_eps_blocks) * 256 + threadIdx.x) * 8;
        if (i8 >= a.nq * a.Kpad) return;
        const int64_t q = i8 / a.Kpad;
        const int p0 = (int)(i8 - q * a.Kpad);
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = DIRECT ? (p0 + j < a.D ? p0 + j : -1) : ivf_pqk_operand_dim(p0 + j, a.M, a.dsub);
            double t;
            o[j] = d < 0 ? (_Float16)0.f : pqk_operand(a.Q[(size_t)q * a.D + d], bs_ts, t);
        }
        *reinterpret_cast<half8 *>(a.wrows + i8) = o;
        return;
    }
    // error bounds: 16 lanes per query
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t q = gid >> 4;
    const int part = (int)(gid & 15);
    double n2 = 0.0, w1 = 0.0, rerr = 0.0, terr = 0.0, dsum = 0.0;
    if (q < a.nq)
        for (int d = part; d < a.D; d += 16) {
            const float v = a.Q[(size_t)q * a.D + d];
            const double av = fabs((double)v), tmax = (double)a.dimc[d];
            double t;
            const _Float16 b = pqk_operand(v, bs_ts, t);
            n2 = fma((double)v, (double)v, n2);
            w1 += av * tmax;
            rerr += fabs((double)(float)b - t) * tmax;   // what the fp16 operand really lost (subnormal steps included), times the largest |T| / ts
            terr += av * (double)a.dimc[a.D + d];        // what the fp16 table lost of the codebook
            dsum += av * (double)a.dimc[2 * a.D + d];    // the one float32 add of the decode
        }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        n2 += __shfl_xor(n2, o);
        w1 += __shfl_xor(w1, o);
        rerr += __shfl_xor(rerr, o);
        terr += __shfl_xor(terr, o);
        dsum += __shfl_xor(dsum, o);
    }
    if (q >= a.nq || part != 0) return;
    // DESIGN 4.4 "IVF-PQ K-loop scan", in key units (times cs at the end)
    const double qn = sqrt(n2), Xn = (double)a.xnorm_max, f = a.metric == 0 ? 2.0 : 1.0;
    const double x2 = a.metric == 0 ? Xn * Xn : 0.0;
    const double w_err = a.ts * rerr / cs;                               // sum |B - t| |T| / cs, |T| = ts (|T| / ts)
    const double mag = x2 + f * (1.001 * w1 + qn * a.can) + w_err;       // |bias| + |MFMA terms| + |slot term|
    const double dec_err = f * (ldexp(1.0, -24) + ldexp(1.0, -47)) * dsum;   // x^ against c_l + cb: one float32 rounding per dimension
    const double t_err = f * terr;
    const double acc_err = (double)(a.Kpad + 4) * ldexp(1.0, -23) * mag; // fp32 accumulation, the slot add included
    const double slot_err = (ldexp(1.0, -24) + ldexp(1.0, -40)) * mag;   // the slot term rounded once (and its float64 sums)
    const double pack_err = ldexp(1.0, -17) * (x2 + f * qn * Xn);        // 6 mantissa bits carry the group id
    const double bias_err = ldexp(1.0, -24) * x2;
    const double key_err = key64_round_err(a.metric, a.D, qn, Xn);
    double e = cs * (dec_err + t_err + w_err + acc_err + slot_err + pack_err + bias_err + key_err) * 1.02;
    if (!(e < 1.0e37)) e = 1.0e37;
    a.eps[q] = (float)e + 1.0e-30f;
    a.qterm[q] = 0.0;
}
__global__ __launch_bounds__(256) void ivf_pqk_prep_kernel(PqkPrepArgs a) { pqk_prep_body<false>(a); }

// ---- the scan -------------------------------------------------------------------------------------------------------------------------
struct PqkScanArgs {
    const unsigned char *codes;   // [N][M], list order
    const _Float16 *table;        // [M][256][P] fp16(ts cb), zero in the padding
    int M, P8, npieces;           // P / 8 pieces per table entry; Kp / 8 pieces of a row
    const int32_t *span_row0, *span_valid;      // [pspans] first list-order row / valid rows of every panel span
    const float *bias;            // [pspans * TPS * 16] linear in the local row of the span; kPadBias on padding rows
    const _Float16 *wrows;        // [nq][64 nk] operand rows (ivf_pqk_operand_dim)
    const float *slot_term;       // [slots]
    const QueryBatchInfo *info;
    float *bin_m[kIvfKloopMinima];
    const int32_t *item_list, *item_slot0, *item_bin0, *n_items, *list_pspan0, *slot_query;
    int part_spans;               // spans per row part (blockIdx.y), 0 = whole list
    int nk;                       // 64-position K-steps of the operand space (>= 3: D > 128)
};

// TPS, BS, GROUP: as ivf_kloop_scan_kernel (RH = 1: the square tile is not built for this route); CP: bytes between staged code rows
template <int TPS, int BS, int GROUP, int CP>
__global__ __launch_bounds__(512, 2) void ivf_pq_kloop_scan_kernel(PqkScanArgs a) {
    static_assert(GROUP == 4 || ((GROUP == 2 || GROUP == 1) && TPS == 16), "pairs / rows need the 64-row bins of TPS = 16");
    constexpr int NWAVES = 8, RING = 2 * BS, HT = 8, CB = 4, NM = kIvfKloopMinima;
    constexpr int PPS = TPS / HT, SPANROWS = TPS * 16, BINROWS = TPS * 4;
    constexpr int kStageBytes = (int)ivf_pqk_stage_bytes();
    static_assert(HT == NWAVES && TPS % HT == 0 && TPS <= 64, "one tile per wave and stage; the tile number must fit the 6-bit id");
    static_assert(BS <= 2, "codes are fetched BS + 1 K-steps ahead, inside the pass after the current one (nk >= 3)");
    static_assert((size_t)RING * kStageBytes + (size_t)NWAVES * NM * CB * 64 * 4 + (size_t)2 * 128 * CP == ivf_pqk_lds_bytes(BS, CP) &&
                      ivf_pqk_lds_bytes(BS, CP) <= kPqkLdsBudget,
                  "the plan's LDS bytes");
    __shared__ __attribute__((aligned(16))) unsigned char smem[RING * kStageBytes];
    __shared__ float s_min[NWAVES][NM * CB][64];            // the running minima of the current bins between passes (ivf_kloop.hpp)
    __shared__ __attribute__((aligned(16))) unsigned char s_codes[2][NWAVES][16][CP];   // [pass & 1][tile][MFMA row][m]

    const int it = blockIdx.x;
    if (it >= *a.n_items) return;
    if (a.info->force_fallback) return;                     // flagged whole: the select reads no bin
    const int l = a.item_list[it];
    int64_t span0 = a.list_pspan0[l], span1 = a.list_pspan0[l + 1];
    const int64_t lspan0 = span0;
    const int nb_item = (int)(span1 - span0) * 4;           // bins per query slot in this item
    if (a.part_spans > 0) {
        span0 += (int64_t)blockIdx.y * a.part_spans;
        if (span0 >= span1) return;
        if (span0 + a.part_spans < span1) span1 = span0 + a.part_spans;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int nK = a.nk;
    const int slot0 = a.item_slot0[it] + wave * 64;
    const size_t bin_base = (size_t)a.item_bin0[it];
    const float cs = a.info->cs;
    const int npass = (int)(span1 - span0) * PPS;
    const int nsteps = npass * nK;

    // the queries behind this wave's slots: per column block one byte offset into the operand rows (row pitch 128 nK bytes)
    int qoff[CB];
    bool any_query = false;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int qi = a.slot_query[slot0 + cb * 16 + (lane & 15)] - 1;      // (-1: padding slot)
        any_query |= qi >= 0;
        qoff[cb] = (qi < 0 ? 0 : qi) * (nK * 128) + g * 16;
    }
    const bool live = __builtin_amdgcn_readfirstlane((int)(__ballot(any_query) != 0ull)) != 0;

    // codes of pass `pass` -> s_codes[pass & 1], this wave's tile: lane group g owns the MFMA rows 4 g + i = four consecutive local rows
    const int M = a.M;
    auto codes_stage = [&](int pass) {
        const int64_t span = span0 + pass / PPS;
        const int base = BINROWS * g + 4 * ((pass % PPS) * HT + wave);
        const int row0 = a.span_row0[span], valid = a.span_valid[span];
        unsigned char *dst = &s_codes[pass & 1][wave][4 * g][0];
        if ((M & 3) == 0) {
            const int mdw = M >> 2;
#pragma unroll 1
            for (int j = lane & 15; j < 4 * mdw; j += 16) {
                const int i = j / mdw, c = j - i * mdw;
                const int local = base + i;
                const unsigned char *src = a.codes + (size_t)(row0 + (local < valid ? local : 0)) * M;
                reinterpret_cast<unsigned *>(dst + i * CP)[c] = reinterpret_cast<const unsigned *>(src)[c];
            }
        } else {
#pragma unroll 1
            for (int j = lane & 15; j < 4 * M; j += 16) {
                const int i = j / M, c = j - i * M;
                const int local = base + i;
                dst[i * CP + c] = a.codes[(size_t)(row0 + (local < valid ? local : 0)) * M + c];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // (a wave reads only the rows it staged itself)
        __builtin_amdgcn_wave_barrier();
    };

    // The two pieces of this lane in K-step `step`: lane (r, kq) of k-step ks -> piece pc = 8 kk + 4 ks + kq, of sub-space m = pc / P8.
    // code_fetch reads their code bytes (one register); stage_issue forms the table addresses and gathers this wave's tile of the
    // K-step into LDS slot `buf`: the piece of lane (r, kq) lands at byte 16 lane of (tile, ks)
    const float inv_p8 = 1.0f / (float)a.P8;
    auto piece_m = [&](int pc) { return (int)(((float)pc + 0.5f) * inv_p8); };   // pc / P8: pc < 512, the quotient is 0.5 / P8 away from an integer
    auto code_fetch = [&](int step) {
        const int pass = step / nK, kk = step - pass * nK;
        const unsigned char *cr = &s_codes[pass & 1][wave][lane & 15][0];
        const int pc = 8 * kk + g;
        const unsigned c0 = cr[pc < a.npieces ? piece_m(pc) : 0], c1 = cr[pc + 4 < a.npieces ? piece_m(pc + 4) : 0];
        return c0 | (c1 << 8);
    };
    const unsigned char *tab = reinterpret_cast<const unsigned char *>(a.table);
    auto stage_issue = [&](int step, unsigned cpair, int buf) {
        const int kk = step % nK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pc = 8 * kk + 4 * ks + g, m = piece_m(pc);
            const int code = (int)((cpair >> (8 * ks)) & 255u);
            const int off = pc < a.npieces ? ((m * 256 + code) * a.P8 + (pc - m * a.P8)) * 16 : 0;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(tab + off)),
                reinterpret_cast<__attribute__((address_space(3))) void *>(
                    static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem + buf * kStageBytes + (wave * 2 + ks) * 1024))),
                16, 0, 0);
        }
    };
    auto clamp_step = [&](int s) { return s < nsteps ? s : nsteps - 1; };

    codes_stage(0);
#pragma unroll
    for (int i = 0; i < BS; ++i)
        if (i < nsteps) stage_issue(i, code_fetch(i), i);
    unsigned pre = code_fetch(clamp_step(BS));
    if (!live) {                                            // all 64 slots are padding: codes, gathers and barriers only
        __syncthreads();
        for (int step = 0; step < nsteps; ++step) {
            const int pass = step / nK;
            if (step == pass * nK && pass + 1 < npass) codes_stage(pass + 1);
            stage_issue(clamp_step(step + BS), pre, (step + BS) % RING);
            pre = code_fetch(clamp_step(step + 1 + BS));
            if (BS == 1 || (step % BS) == BS - 1) __syncthreads();
        }
        return;
    }

    const float INF = __builtin_inff();
    float NEG_INF = -INF;
    asm volatile("" : "+v"(NEG_INF));
    unsigned idmask = kQuadIdMask;
    asm volatile("" : "+v"(idmask));
#pragma unroll
    for (int i = 0; i < NM * CB; ++i) s_min[wave][i][lane] = INF;

    float4v acc[HT][CB];
    half8 bq[CB][2];          // B fragments of the current K-step, reloaded in place (ivf_kloop.hpp)
    const __amdgpu_buffer_rsrc_t rsq = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(a.wrows), 0, 0x7fffffff, 0x00020000);
    auto load_b = [&](int kk, int ks) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
            bq[cb][ks] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsq, qoff[cb], (kk * 2 + ks) * 64, 0));
    };
    load_b(0, 0);
    __syncthreads();

    half8 fr[2][4];
    auto read_group = [&](int buf, int grp, half8(&dst)[4]) {   // group grp = (ks = grp >> 1, tiles 4 (grp & 1) .. + 3)
        const half8 *A = reinterpret_cast<const half8 *>(smem + buf * kStageBytes);
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[t] = A[(((grp & 1) * 4 + t) * 2 + (grp >> 1)) * 64 + lane];
    };
    read_group(0, 0, fr[0]);

    int step = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const int64_t span = span0 + pass / PPS;
        const int slice = pass % PPS;
        if (pass + 1 < npass) codes_stage(pass + 1);
        // accumulators start from the bias of their rows: local row = BINROWS * g + 4 * (HT * slice + t) + i
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const float4 c = *reinterpret_cast<const float4 *>(a.bias + span * SPANROWS + g * BINROWS + (slice * HT + t) * 4);
            acc[t][0][0] = (c.x >= 0.9e38f) ? kPadBias : c.x * cs;
            acc[t][0][1] = (c.y >= 0.9e38f) ? kPadBias : c.y * cs;
            acc[t][0][2] = (c.z >= 0.9e38f) ? kPadBias : c.z * cs;
            acc[t][0][3] = (c.w >= 0.9e38f) ? kPadBias : c.w * cs;
#pragma unroll
            for (int cb = 1; cb < CB; ++cb) acc[t][cb] = acc[t][0];
        }
#pragma unroll 1
        for (int kk = 0; kk < nK; ++kk, ++step) {
            const int buf = step % RING;
            load_b(kk, 1);
            stage_issue(clamp_step(step + BS), pre, (step + BS) % RING);
            const int kn = (kk + 1 == nK) ? 0 : kk + 1;      // B repeats every pass
#pragma unroll
            for (int grp = 0; grp < 4; ++grp) {
                __builtin_amdgcn_sched_barrier(0);
                if (grp < 3) {
                    read_group(buf, grp + 1, fr[(grp + 1) & 1]);
                    if (grp == 1) pre = code_fetch(clamp_step(step + 1 + BS));   // (the codes of the gather after next: off the MFMA path)
                } else {
                    if (BS == 1 || (step % BS) == BS - 1) __syncthreads();
                    read_group((step + 1) % RING, 0, fr[0]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
                        acc[(grp & 1) * 4 + t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            fr[grp & 1][t], bq[cb][grp >> 1], acc[(grp & 1) * 4 + t][cb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (grp == 1) load_b(kn, 0);
            }
        }
        float m[NM][CB];           // m[0] <= m[1] <= ... : sorted insertion by one v_min + (NM - 1) v_med3 per group
        float tslot[CB];           // the slot terms of the lane's columns, re-read per pass (not held across the K-loop, where every
                                   // register counts).  A padding slot's is never written: nobody reads its bins
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) tslot[cb] = a.slot_term[slot0 + cb * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < NM; ++i)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) m[i][cb] = s_min[wave][i * CB + cb][lane];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const unsigned id = (unsigned)(slice * HT + t);  // tile number inside the span = quad number inside the bin
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                auto insert = [&](float v) {
#pragma unroll
                    for (int i = NM - 1; i > 0; --i) m[i][cb] = __builtin_amdgcn_fmed3f(m[i - 1][cb], m[i][cb], v);
                    m[0][cb] = fast_min(m[0][cb], v, NEG_INF);
                };
                if (GROUP == 4) {
                    const float qm = quad_min(acc[t][cb][0], acc[t][cb][1], acc[t][cb][2], acc[t][cb][3], NEG_INF) + tslot[cb];
                    insert(pack_score(qm, idmask, id));
                } else if (GROUP == 2) {
                    insert(pack_score(fast_min(acc[t][cb][0], acc[t][cb][1], NEG_INF) + tslot[cb], idmask, 2 * id));
                    insert(pack_score(fast_min(acc[t][cb][2], acc[t][cb][3], NEG_INF) + tslot[cb], idmask, 2 * id + 1));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) insert(pack_score(acc[t][cb][i] + tslot[cb], idmask, 4 * id + i));
                }
            }
        }
        if (slice == PPS - 1) {                              // the four bins (span, g) are complete: [item][slot][bin]
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const size_t o = bin_base * kIvfKloopGroup + (size_t)(wave * 64 + cb * 16 + (lane & 15)) * nb_item +
                                 (size_t)((span - lspan0) * 4 + g);
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    a.bin_m[i][o] = m[i][cb];
                    m[i][cb] = INF;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NM; ++i)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) s_min[wave][i * CB + cb][lane] = m[i][cb];
    }
}

}  // namespace vdb

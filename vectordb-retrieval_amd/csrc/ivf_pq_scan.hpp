// ivf_pq_scan.hpp -- IVF<nlist>,PQ<M>, option "ivf_pq_direct": the list-major MFMA scan straight from the product codes (D <= 128).
//
// The fallback route decodes the WHOLE panel space into fp16 panels per batch (ivf_pq_panels_kernel) and runs scan_kernel on them.  Here
// the score is split as on the K-loop route (ivf_pq_kloop.hpp; x^[d] = fl32(c_l[d] + cb[m][code[m]][j]), every row of a work item in ONE
// list), but in plain dimension order:
//     accumulator init cs ||x^||^2      the resident bias of the panel space, as on every route
//   + sum_d B[d] T[d]                   the MFMAs: T = fp16(ts cb) from the handle's table, B = fp16(bs q[d] / ts), bs = -2 cs | -cs
//   + S[slot]                           one float32 per (query, list) slot: bs (q . c_l) (ivf_sq8d_slot_kernel with q . e = 0), added to a
//                                       quad's minimum, not to its four scores (ivf_sq8_scan.hpp: rounding is monotone)
// The K-loop route gathers 16-byte pieces of a zero-padded table from global memory; at D <= 128 the whole table T[m][256][dsub] is
// 512 D bytes <= 64 KiB, so it is RESIDENT IN LDS and nothing is padded by dsub:
//   table    one linear copy per workgroup (global_load_lds, 1 KiB per wave instruction).
//   codes    the 64 rows x M code bytes of a stage (ST = 2 tiles x two runs of 16 consecutive list-order rows; a padding row reads the
//            span's first row, its accumulator init is kPadBias) are fetched one stage ahead of their decode -- 16 / 8 / 4 lanes walk the
//            dwords of a row, through registers held across the stage's MFMAs -- into rows of CP bytes, CP an odd number of dwords.
//            M % 4 != 0: byte copies at the stage's end (code rows are then no whole dwords).
//   decode   a stage is ST x KSTEPS pieces of 1 KiB = (tile, k-step); the pieces are dealt across the NWAVES waves, each decoded ONCE
//            per workgroup.  Lane (rho, kh) forms the dims 16 ks + 8 kh .. + 7 of MFMA row rho by LDS lookups T[m][code[m]][j] -- one
//            ds_read_b128 when dsub % 8 == 0, four ds_read_b32 when dsub is even, eight ds_read_u16 else (a sub-vector may straddle the
//            group); dims >= D are zero; all code bytes are read before all table entries, without a branch -- and stores them with
//            one ds_write_b128 at 16 lane of the piece: the layout of the fp16 panels.  Stage s + 1 is decoded inside the loop
//            iteration that scans stage s, so ONE barrier per stage orders everything:
//            codes (s + 2) -> registers | MFMA (s), decode (s + 1) behind each tile's MFMAs | codes (s + 2) -> LDS | barrier.
//   MFMA     read_phase / mfma_phase of scan.hpp on the decoded stage, sq8d_select_phase, the bins of items mode: the plan,
//            ivf_select_kernel and ivf_tail_kernel run unchanged; eps is this route's own (DESIGN 4.4 "IVF-PQ direct scan").
// LDS bytes by (D, M, KSTEPS): ivf_pq_direct_plan.hpp -- 105 KiB at D = 128 / PQ64 (one workgroup per CU), 51 KiB at D = 64 / PQ16 (three).
#pragma once
#include <type_traits>

#include "common.hpp"
#include "ivf_mfma.hpp"
#include "ivf_pq_direct_plan.hpp"
#include "ivf_pq_kloop.hpp"
#include "ivf_sq8_scan.hpp"
#include "scan.hpp"

namespace vdb {

// per batch: scale, error bounds, operand rows in dimension order, per-list probe counts (the prep of ivf_pq_kloop.hpp with Kpad = 16 KSTEPS)
__global__ __launch_bounds__(256) void ivf_pqd_prep_kernel(PqkPrepArgs a) { pqk_prep_body<true>(a); }

struct PqdScanArgs {
    const unsigned char *codes;   // [N][M], list order
    const _Float16 *table;        // [M][256][dsub] fp16(ts cb), zero padded to whole KiB (ivf_pqd_table_bytes)
    int D, M, dsub;
    const int32_t *span_row0, *span_valid;      // [pspans] first list-order row / valid rows of every panel span
    const float *bias;            // [pspans * 256] ||x^||^2 (L2) | 0 (IP) | the pad marker
    const _Float16 *wrows;        // [nq][16 KSTEPS] operand rows, dimension order
    const float *slot_term;       // [slots]
    const QueryBatchInfo *info;
    float *bin_m1, *bin_m2, *bin_m3;
    const int32_t *item_list, *item_slot0, *item_bin0, *n_items, *list_pspan0, *slot_query;
    int part_spans;
};

// The 8 dims d0 .. d0 + 7 of the row whose staged codes are `cr`, from the table in LDS.  MODE 2: dsub % 8 == 0, 1: dsub even, 0: any.
// Branch free: every code byte is read first, then every table entry, so a piece costs two LDS round trips whatever dsub is (a branch
// per dimension made each of up to sixteen reads wait for the one before it).  A dim >= D reads dim 0 and is zeroed afterwards.
template <int MODE>
__device__ __forceinline__ uint4 pqd_decode8(const _Float16 *__restrict__ T, const unsigned char *__restrict__ cr, int d0, int D, int dsub,
                                             float inv_dsub) {
    constexpr int STEP = MODE == 2 ? 8 : MODE == 1 ? 2 : 1, NE = 8 / STEP;
    int off[NE];
    unsigned code[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int d = d0 + STEP * e, dd = d < D ? d : 0;
        const int m = (int)(((float)dd + 0.5f) * inv_dsub);    // dd / dsub: dd < 128, the quotient is 0.5 / dsub away from an integer
        code[e] = cr[m];
        off[e] = m * 256 * dsub + (dd - m * dsub);
    }
    if (MODE == 2) {
        const uint4 o = *reinterpret_cast<const uint4 *>(T + (off[0] + (int)code[0] * dsub));
        return d0 < D ? o : make_uint4(0u, 0u, 0u, 0u);
    }
    unsigned v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const _Float16 *src = T + (off[e] + (int)code[e] * dsub);
        v[e] = MODE == 1 ? *reinterpret_cast<const unsigned *>(src) : (unsigned)*reinterpret_cast<const unsigned short *>(src);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if (d0 + STEP * e >= D) v[e] = 0u;
    if (MODE == 1) return make_uint4(v[0], v[1], v[2], v[3]);
    return make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}

// One workgroup = (list) x (64 NWAVES query slots) x (row part), as scan_kernel's items mode: same spans, stages of ST = 2 tiles, bins of
// BT tiles per lane half, early / late wave halves (scan.hpp, "Phase stagger"), same bin layout.
// (KSTEPS 8 holds a table of more than 32 KiB: at 2 and 4 waves a SIMD sees one wave anyway, so the allocator gets its 512 registers)
template <int KSTEPS, int NWAVES, int BT>
__global__ __launch_bounds__(NWAVES * 64, (KSTEPS == 8 && NWAVES <= 4) ? 1 : 2) void ivf_pq_scan_kernel(PqdScanArgs a) {
    constexpr int NT = NWAVES * 64, ST = kPqdStageTiles, TPS = kIvfTilesPerSpan;
    constexpr int kPieces = ST * KSTEPS, kStageBytes = kPieces * 1024, PW = kPieces / NWAVES;     // PW: pieces a wave decodes per stage
    constexpr int kBiasLoads = (ST * 32 + NT - 1) / NT;
    constexpr int kRowLoads = ST * 32 * 16 / NT;            // code dwords of a lane per stage and column pass, 16 lanes per row
    constexpr int kSpanR = TPS * 32, kHalfR = TPS * 16, SPS = TPS / ST, BPS = TPS / BT;
    static_assert(kPieces % NWAVES == 0 && TPS % BT == 0 && BT % ST == 0 && ST == 2, "bad geometry");
    static_assert(kStageBytes == (int)ivf_pqd_stage_bytes(KSTEPS), "the plan's LDS bytes");
    extern __shared__ __attribute__((aligned(16))) unsigned char pqd_lds[];
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
    const int D = a.D, M = a.M, dsub = a.dsub, CP = ivf_pqd_code_pitch(M);
    const _Float16 *T = reinterpret_cast<const _Float16 *>(pqd_lds);
    unsigned char *lds_stage = pqd_lds + ivf_pqd_table_bytes(D);
    unsigned char *lds_codes = lds_stage + 2 * kStageBytes;
    const int codes_bytes = ST * 32 * CP;
    auto lds_a = [&](int buf) { return lds_stage + buf * kStageBytes; };
    auto lds_c = [&](int buf) { return lds_codes + buf * codes_bytes; };
    auto lds_b = [&](int buf) { return reinterpret_cast<float *>(lds_codes + 2 * codes_bytes) + buf * (ST * 32); };

    // ---- the table: one linear copy, 1 KiB per wave instruction ----
    {
        const int npieces = (int)(ivf_pqd_table_bytes(D) >> 10);
        const unsigned char *src = reinterpret_cast<const unsigned char *>(a.table);
        for (int p = wave; p < npieces; p += NWAVES)
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(src + p * 1024 + lane * 16)),
                reinterpret_cast<__attribute__((address_space(3))) void *>(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(pqd_lds + p * 1024))),
                16, 0, 0);
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

    // ---- codes of a stage -> LDS row (tile t, run hh, r) = t 32 + hh 16 + r: local row hh kHalfR + (sq ST + t) 16 + r of the span ----
    const bool vec = (M & 3) == 0;
    const int mdw = M >> 2;
    const int lg = mdw > 8 ? 4 : mdw > 4 ? 3 : 2;           // lanes per code row: 16 / 8 / 4 (each reads dword c, and c + 16 when M > 64)
    auto stage_row = [&](int st, int slot) {               // list-order row behind LDS row `slot` of stage st (never past the codes)
        const int64_t span = span0 + st / SPS;
        const int local = ((slot >> 4) & 1) * kHalfR + ((st % SPS) * ST + (slot >> 5)) * 16 + (slot & 15);
        return (size_t)(a.span_row0[span] + (local < a.span_valid[span] ? local : 0));
    };
    unsigned creg[kRowLoads][2];
    auto codes_issue = [&](int st) {
#pragma unroll
        for (int i = 0; i < kRowLoads; ++i) {
            const int u = tid + i * NT, slot = u >> lg, c = u & ((1 << lg) - 1);
            if (slot < ST * 32) {
                const unsigned *src = reinterpret_cast<const unsigned *>(a.codes + stage_row(st, slot) * M);
                if (c < mdw) creg[i][0] = src[c];
                if (c + 16 < mdw) creg[i][1] = src[c + 16];
            }
        }
    };
    auto codes_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kRowLoads; ++i) {
            const int u = tid + i * NT, slot = u >> lg, c = u & ((1 << lg) - 1);
            if (slot < ST * 32) {
                unsigned *dst = reinterpret_cast<unsigned *>(lds_c(buf) + slot * CP);
                if (c < mdw) dst[c] = creg[i][0];
                if (c + 16 < mdw) dst[c + 16] = creg[i][1];
            }
        }
    };
    const float inv_m = 1.0f / (float)M;
    auto codes_bytes_copy = [&](int st, int buf) {          // M % 4 != 0: i / M by a float product (i < 8192, the quotient is 0.5 / M off)
        for (int i = tid; i < ST * 32 * M; i += NT) {
            const int slot = (int)(((float)i + 0.5f) * inv_m), c = i - slot * M;
            lds_c(buf)[slot * CP + c] = a.codes[stage_row(st, slot) * M + c];
        }
    };
    auto codes_fetch = [&](int st, int buf) {
        if (vec) {
            codes_issue(st);
            codes_store(buf);
        } else {
            codes_bytes_copy(st, buf);
        }
    };

    float stage_b[kBiasLoads];
    auto bias_issue = [&](int st) {
        const int64_t span = span0 + st / SPS;
        const int sq = st % SPS;
#pragma unroll
        for (int i = 0; i < kBiasLoads; ++i) {
            const int e = tid + i * NT;
            if (e < ST * 32) {
                const int t = e >> 5, hh = (e >> 4) & 1, r = e & 15;
                stage_b[i] = a.bias[span * kSpanR + hh * kHalfR + (sq * ST + t) * 16 + r];
            }
        }
    };
    auto bias_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kBiasLoads; ++i)
            if (tid + i * NT < ST * 32) lds_b(buf)[tid + i * NT] = (stage_b[i] >= 0.9e38f) ? kPadBias : stage_b[i] * cs;
    };

    // ---- decode: pieces [i0, i1) of this wave's share of a stage, codes buffer `buf` -> A buffer `buf` ----
    const int rho = lane & 31;
    const int slot_lo = ((rho >> 2) & 1) * 16 + ((rho & 3) | ((rho >> 3) << 2));      // LDS code row of MFMA row rho in tile 0
    const float inv_dsub = 1.0f / (float)dsub;
    const int mode = (dsub & 7) == 0 ? 2 : (dsub & 1) == 0 ? 1 : 0;
    auto decode = [&](int buf, int i0, int i1) {
        auto pieces = [&](auto mode_tag) {
#pragma unroll
            for (int i = i0; i < i1; ++i) {
                const int pc = wave + i * NWAVES, tt = pc / KSTEPS, ks = pc % KSTEPS;
                const uint4 o = pqd_decode8<decltype(mode_tag)::value>(T, lds_c(buf) + (tt * 32 + slot_lo) * CP, ks * 16 + h * 8, D, dsub, inv_dsub);
                *reinterpret_cast<uint4 *>(lds_a(buf) + pc * 1024 + lane * 16) = o;
            }
        };
        if (mode == 2) pieces(std::integral_constant<int, 2>{});
        else if (mode == 1) pieces(std::integral_constant<int, 1>{});
        else pieces(std::integral_constant<int, 0>{});
    };
    // what an iteration does beside its MFMAs: the loads of later stages up front, their LDS stores and the barrier at the end
    auto stage_top = [&](int st) {
        if (vec && st + 2 < nstages) codes_issue(st + 2);
        if (st + 1 < nstages) bias_issue(st + 1);
    };
    auto stage_bottom = [&](int st) {
        if (st + 2 < nstages) {
            if (vec) codes_store(st & 1);
            else codes_bytes_copy(st + 2, st & 1);
        }
        if (st + 1 < nstages) bias_store((st & 1) ^ 1);
        __syncthreads();
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

    // ---- prologue: codes of stages 0 and 1, bias of stage 0, the slots' operand rows and slot terms behind them ----
    codes_fetch(0, 0);
    if (nstages > 1) codes_fetch(1, 1);
    bias_issue(0);
    half8 b0[KSTEPS], b1[KSTEPS];
    float t0 = 0.f, t1 = 0.f;
    {
        const half8 *ra = reinterpret_cast<const half8 *>(a.wrows + (size_t)(qa < 0 ? 0 : qa) * (16 * KSTEPS)) + h;
        const half8 *rb = reinterpret_cast<const half8 *>(a.wrows + (size_t)(qb < 0 ? 0 : qb) * (16 * KSTEPS)) + h;
        half8 zero;
#pragma unroll
        for (int j = 0; j < 8; ++j) zero[j] = (_Float16)0.f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            b0[ks] = qa < 0 ? zero : ra[ks * 2];
            b1[ks] = qb < 0 ? zero : rb[ks * 2];
        }
        if (qa >= 0) t0 = a.slot_term[q0 + (lane & 31)];
        if (qb >= 0) t1 = a.slot_term[q0 + 32 + (lane & 31)];
    }
    bias_store(0);
    __syncthreads();                                        // the table and the codes of stages 0 and 1 are in LDS
    decode(0, 0, PW);
    __syncthreads();

    if (__ballot(qa >= 0 || qb >= 0) == 0ull) {             // a wave of padding slots only keeps staging, decode and barriers going
        for (int st = 0; st < nstages; ++st) {
            stage_top(st);
            if (st + 1 < nstages) decode((st & 1) ^ 1, 0, PW);
            stage_bottom(st);
        }
        return;
    }

    half8 fr[KSTEPS];
    float16v cin, acc0, acc1;
    if (!late) {        // early half: MFMA(t), then select(t)
        for (int st = 0; st < nstages; ++st) {
            const int buf = st & 1;
            const bool more = st + 1 < nstages;
            stage_top(st);
            const half8 *A = reinterpret_cast<const half8 *>(lds_a(buf));
            const float4 *B4 = reinterpret_cast<const float4 *>(lds_b(buf)) + h * 4;
            const int ts0 = (st % SPS) * ST;
            read_phase<KSTEPS>(A, B4, fr, cin, lane);
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                __builtin_amdgcn_sched_barrier(0);
                mfma_phase<KSTEPS>(fr, b0, b1, cin, acc0, acc1);
                __builtin_amdgcn_sched_barrier(0);
                if (t + 1 < ST) read_phase<KSTEPS>(A + (t + 1) * KSTEPS * 64, B4 + (t + 1) * 8, fr, cin, lane);
                if (more) decode(buf ^ 1, t * PW / ST, (t + 1) * PW / ST);   // behind the MFMAs just issued: the matrix pipe is still busy
                sq8d_select_phase(acc0, acc1, m1, m2, m3, idmask, NEG_INF, (unsigned)(((ts0 + t) % BT) << 2), t0, t1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (((ts0 + ST) % BT) == 0) flush_bin(span0 + st / SPS, (ts0 + ST) / BT - 1);
            stage_bottom(st);
        }
    } else {            // late half: select(t - 1), then MFMA(t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = 3.0e38f;     // dummy "previous tile": can never win
        acc1 = acc0;
        for (int st = 0; st < nstages; ++st) {
            const int buf = st & 1;
            const bool more = st + 1 < nstages;
            stage_top(st);
            const half8 *A = reinterpret_cast<const half8 *>(lds_a(buf));
            const float4 *B4 = reinterpret_cast<const float4 *>(lds_b(buf)) + h * 4;
            const int ts0 = (st % SPS) * ST;
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                __builtin_amdgcn_sched_barrier(0);
                read_phase<KSTEPS>(A + t * KSTEPS * 64, B4 + t * 8, fr, cin, lane);
                const int tp = (ts0 + t + TPS - 1) % TPS;
                sq8d_select_phase(acc0, acc1, m1, m2, m3, idmask, NEG_INF, (unsigned)((tp % BT) << 2), t0, t1);
                if (t == 0 && st > 0 && (ts0 % BT) == 0) flush_bin(span0 + (st * ST - 1) / TPS, tp / BT);
                __builtin_amdgcn_sched_barrier(0);
                mfma_phase<KSTEPS>(fr, b0, b1, cin, acc0, acc1);
                __builtin_amdgcn_sched_barrier(0);
                if (more) decode(buf ^ 1, t * PW / ST, (t + 1) * PW / ST);
            }
            __builtin_amdgcn_sched_barrier(0);
            stage_bottom(st);
        }
        sq8d_select_phase(acc0, acc1, m1, m2, m3, idmask, NEG_INF, (unsigned)((BT - 1) << 2), t0, t1);
        flush_bin(span1 - 1, BPS - 1);
    }
    for (int r = (int)(span1 - lspan0) * BPS; r & 3; ++r) items_push(r);      // fill the last vector of this part's run
}

}  // namespace vdb

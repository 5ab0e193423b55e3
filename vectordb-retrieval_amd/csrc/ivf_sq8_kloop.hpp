// ivf_sq8_kloop.hpp -- IVF<nlist>,SQ8, option "ivf_sq8_kloop": the K-loop list scan straight from the 8-bit codes for D > 128.
//
// The K-loop form of ivf_sq8_scan.hpp (whose header derives the split of the score: accumulator init cs ||x^||^2, MFMA sum of
// B[d] k[d] with B = fp16(bs q[d] vdiff[d] / 255) and k = code - 128 exact in fp16, one float32 slot term per (query, list) slot) on
// the work split of ivf_kloop_scan_kernel (ivf_kloop.hpp): work item = one list x 512 query slots, 8 waves x 64 slots, blockIdx.y =
// row part, one pass = 8 tiles x 4 column blocks (128 accumulator registers), B gathered per 64-dim K-step from the fp16 operand rows
// through a buffer descriptor with per-lane row offsets.  An SQ8 index holds no panels, so the A operand is the list-order codes:
//   staging   a tile K-step is 16 rows x 64 code bytes = 1 KiB = ONE global_load_lds per wave: lane (row r = lane & 15, quarter kq =
//             lane >> 4) fetches the 16-byte chunk 4 kk + kq of its row (ivf_sq8d_chunk_base: a chunk that would cross the row's end is
//             the row's last 16 bytes) and lands at byte 16 * lane of the tile.  Wave w stages tile w of the pass: a stage is 8 KiB,
//             half of the fp16 scan's.  The p16 row mapping -- MFMA row 4g + i of tile t <-> local row (4 TPS) g + 4 t + i of the span --
//             is applied in the load addresses, so bins, 6-bit ids and candidate groups are those of ivf_kloop_scan_kernel.  A padding
//             row of the last span (its accumulator init is kPadBias) reads the span's first row: never past the codes.
//   MFMA      lane (r, kq) reads ITS 16 bytes with one ds_read_b128 (lane-linear, conflict free) and widens them in registers
//             (sq8d_widen: v_perm_b32 to 1024 + code, v_pk_add_f16 - 1152): bytes 0..7 feed the first v_mfma_f32_16x16x32_f16 of the
//             K-step, bytes 8..15 the second.  The K order inside a K-step is therefore permuted -- element 32 ks + 8 kq + j of the
//             K-step is dimension 64 kk + 16 kq + 8 ks + j -- and the operand rows are written in the same order (ivf_sq8k_operand_dim).
//   bins      the slot term is added to the minimum of a candidate group before it is packed, not to the group's scores (rounding is
//             monotone: ivf_sq8_scan.hpp); every bin keeps its kIvfKloopMinima smallest group minima with their ids and they leave in
//             [item][slot][bin] order, so the plan, ivf_select_kernel and ivf_tail_kernel run unchanged.
// Stage ring and barrier placement are those of ivf_kloop_scan_kernel (RING = 2 BS slots, one barrier per BS K-steps).
#pragma once
#include "ivf_sq8_scan.hpp"
#include "scan16.hpp"

namespace vdb {

// ---- per batch: ivf_sq8d_prep_kernel with the operand rows in the K order of this scan -------------------------------------------
// Scale, windows, q . e and the error bound are the D <= 128 route's (sq8d_prep_body): the bound is written in Dpad, the terms of the
// float32 accumulator, and holds unchanged up to the K-loop's 4096 dimensions (DESIGN 4.4 "IVF-SQ8 K-loop scan").
__global__ __launch_bounds__(256) void ivf_sq8k_prep_kernel(Sq8dPrepArgs a) { sq8d_prep_body<true>(a); }

// ---- the scan -------------------------------------------------------------------------------------------------------------------------
struct Sq8kScanArgs {
    const unsigned char *codes;   // [N][D4], list order
    int D4;
    const int32_t *span_row0, *span_valid;      // [pspans] first list-order row / valid rows of every panel span
    const float *bias;            // [pspans * TPS * 16] linear in the local row of the span; kPadBias on padding rows
    const _Float16 *wrows;        // [nq][64 nk] operand rows (ivf_sq8k_operand_dim)
    const float *slot_term;       // [slots]
    const QueryBatchInfo *info;
    float *bin_m[kIvfKloopMinima];
    const int32_t *item_list, *item_slot0, *item_bin0, *n_items, *list_pspan0, *slot_query;
    int part_spans;               // spans per row part (blockIdx.y), 0 = whole list
    int nk;                       // 64-dim K-steps of the index
};

// TPS, BS, GROUP: as ivf_kloop_scan_kernel (RH = 1: the square tile is not built for this route)
template <int TPS, int BS, int GROUP>
__global__ __launch_bounds__(512, 2) void ivf_sq8_kloop_scan_kernel(Sq8kScanArgs a) {
    static_assert(GROUP == 4 || ((GROUP == 2 || GROUP == 1) && TPS == 16), "pairs / rows need the 64-row bins of TPS = 16");
    constexpr int NWAVES = 8, RING = 2 * BS, HT = kSq8kStageTiles, CB = 4, NM = kIvfKloopMinima;
    constexpr int PPS = TPS / HT, SPANROWS = TPS * 16, BINROWS = TPS * 4;
    constexpr int kStageBytes = (int)ivf_sq8k_stage_bytes();
    static_assert(HT == NWAVES && TPS % HT == 0 && TPS <= 64, "one tile per wave and stage; the tile number must fit the 6-bit id");
    static_assert((size_t)RING * kStageBytes + (size_t)NWAVES * NM * CB * 64 * 4 == ivf_sq8k_lds_bytes(BS), "the plan's LDS bytes");
    __shared__ __attribute__((aligned(16))) unsigned char smem[RING * kStageBytes];
    __shared__ float s_min[NWAVES][NM * CB][64];            // the running minima of the current bins between passes (ivf_kloop.hpp)

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

    // the queries behind this wave's slots: per column block one byte offset into the operand rows (row pitch 128 nK bytes) and
    // the slot term of the lane's column
    int qoff[CB];
    bool any_query = false;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int qi = a.slot_query[slot0 + cb * 16 + (lane & 15)] - 1;      // (-1: padding slot)
        any_query |= qi >= 0;
        qoff[cb] = (qi < 0 ? 0 : qi) * (nK * 128) + g * 16;
    }
    const bool live = __builtin_amdgcn_readfirstlane((int)(__ballot(any_query) != 0ull)) != 0;

    // staging: this wave's tile of K-step `step` -> LDS slot `buf`.  Lane (r, kq): chunk 4 kk + kq of the row behind MFMA row r
    const int loc0 = BINROWS * ((lane & 15) >> 2) + (lane & 3);      // local row of MFMA row r in tile 0 of a span
    auto stage_issue = [&](int step, int buf) {
        const int pass = step / nK, kk = step - pass * nK;
        const int64_t span = span0 + pass / PPS;
        const int local = loc0 + 4 * ((pass % PPS) * HT + wave);
        const int row0 = a.span_row0[span], valid = a.span_valid[span];
        const unsigned char *src = a.codes + (size_t)(row0 + (local < valid ? local : 0)) * a.D4 + ivf_sq8d_chunk_base(4 * kk + g, a.D4);
        __builtin_amdgcn_global_load_lds(
            reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(src)),
            reinterpret_cast<__attribute__((address_space(3))) void *>(
                static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem + buf * kStageBytes + wave * 1024))),
            16, 0, 0);
    };
#pragma unroll
    for (int i = 0; i < BS; ++i)
        if (i < nsteps) stage_issue(i, i);
    if (!live) {                                            // all 64 slots are padding: staging + barriers only
        __syncthreads();
        for (int step = 0; step < nsteps; ++step) {
            stage_issue(step + BS < nsteps ? step + BS : nsteps - 1, (step + BS) % RING);
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

    // A: raw[t] = the lane's 16 code bytes of tile t (both k-steps of the K-step).  Tiles 0..3 of a K-step are read while the previous
    // one finishes (they are free after its third group), tiles 4..7 during the first group
    uint4 raw[HT];
    auto read_half = [&](int buf, int hf) {
        const unsigned char *A = smem + buf * kStageBytes + lane * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) raw[hf * 4 + t] = *reinterpret_cast<const uint4 *>(A + (hf * 4 + t) * 1024);
    };
    read_half(0, 0);

    int step = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const int64_t span = span0 + pass / PPS;
        const int slice = pass % PPS;
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
            stage_issue(step + BS < nsteps ? step + BS : nsteps - 1, (step + BS) % RING);
            const int kn = (kk + 1 == nK) ? 0 : kk + 1;      // B repeats every pass
#pragma unroll
            for (int grp = 0; grp < 4; ++grp) {             // group = (k-step ks = grp >> 1, tiles 4 (grp & 1) .. + 3)
                __builtin_amdgcn_sched_barrier(0);
                if (grp == 0) read_half(buf, 1);
                if (grp == 3) {                             // (tiles 0..3 are consumed: the next K-step's land in their registers)
                    if (BS == 1 || (step % BS) == BS - 1) __syncthreads();
                    read_half((step + 1) % RING, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 4; ++t) {               // widen one tile's 8 bytes, four MFMAs on them: 4 fragment registers live
                    const uint4 r = raw[(grp & 1) * 4 + t];
                    const half8 fr = (grp >> 1) ? sq8d_widen(r.z, r.w) : sq8d_widen(r.x, r.y);
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
                        acc[(grp & 1) * 4 + t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            fr, bq[cb][grp >> 1], acc[(grp & 1) * 4 + t][cb], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (grp == 1) load_b(kn, 0);
            }
        }
        float m[NM][CB];           // m[0] <= m[1] <= ... : sorted insertion by one v_min + (NM - 1) v_med3 per group
        float tslot[CB];           // the slot terms of the lane's columns, re-read per pass (4 loads per 64 nK MFMAs; not held across the
                                   // K-loop, where every register counts).  A padding slot's is never written: nobody reads its bins
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

// ivf_kloop_i8.hpp -- the int8 K-loop LIST scan: IVF-Flat over a byte-valued corpus of D > 128 on v_mfma_i32_16x16x64_i8
// (option "ivf_i8_kloop").
//
// The items-mode form of scan16_i8_kloop_kernel (scan16_i8.hpp), as ivf_kloop_scan_kernel (ivf_kloop.hpp; read that header first) is
// the items-mode form of scan16_kloop_kernel: work item, grid, row parts, p16 row mapping, the five kept minima per bin and their
// [item][slot][bin] order are the fp16 list scan's, so ivf_select_kernel and the tail run unchanged behind it; arithmetic, stage
// ring and key are the flat int8 K-loop scan's.
//   work split   one work item = one inverted list x 512 query slots on 8 waves x 64 slots; blockIdx.y = row part of the list.
//                Per pass a wave owns 8 tiles x 4 column blocks = 128 int32 accumulators, started from the bias8 row of the batch's
//                query window (padding rows: pad, with zero panels -- they leave as kI8kPadKey << 6 | id)
//   A panels     one 64-dim K-step of a pass = 8 x 1 KiB, ONE buffer-addressed LDS-DMA request per wave into a ring of 2 BS stages
//                (half the fp16 stage for the same dimensions); K-step s + BS is requested during K-step s, the workgroup meets at
//                a barrier every BS K-steps; A fragments are read from LDS one group of four tiles ahead
//   B fragments  GATHERED: lane (c = lane & 15, kq = lane >> 4) reads 16 bytes of its slot's int8 query row cq - q ([nq][Dpad],
//                ivf_prep_kernel) through a buffer descriptor with a per-lane row offset -- ONE request per column block and
//                K-step where the fp16 scan issues two -- one K-step ahead into a second register set.  Padding slots read query 0
//   epilogue     per candidate group (quad, pair or row)  integer min, >> shift, v_lshl_or with the 6-bit id, sorted insertion into
//                the five minima of the bin by one v_min_i32 + four v_med3_i32; the running minima are parked in LDS between passes
// Which of the two K-loop list scans serves a batch is decided on the device (QueryBatchInfo.i8_mode): both are enqueued, the one not
// needed returns at once.  The rules (which handles hold the copy, which batches are offered, the launch): ivf_i8k_plan.hpp.
#pragma once
#include "ivf_i8k_plan.hpp"
#include "ivf_kloop.hpp"
#include "scan16_i8.hpp"

namespace vdb {

struct IvfKloopI8Args {
    const int4v *panels;          // [pspans * TPS tiles][nk][64] int8 A panels, p16 order
    const int32_t *bias8;         // [2][npad] accumulator inits per query window, linear in the local row of the span; pad on padding rows
    const signed char *qrows;     // [nq][64 nk] int8 query rows cq - q
    const QueryBatchInfo *info;
    float *bin_m[kIvfKloopMinima];
    const int32_t *item_list, *item_slot0, *item_bin0, *n_items, *list_pspan0, *slot_query;
    int part_spans;               // spans per row part (blockIdx.y), 0 = whole list
    int nk;                       // 64-dim K-steps of the index
    int shift;                    // key rule of the handle
    int64_t npad;                 // rows of one query window of bias8 = pspans * span rows
};

template <int TPS, int BS, int GROUP = 4>
__global__ __launch_bounds__(512, 2) void ivf_kloop_i8_scan_kernel(IvfKloopI8Args a) {
    static_assert(GROUP == 4 || ((GROUP == 2 || GROUP == 1) && TPS == 16), "pairs / rows need the 64-row bins of TPS = 16");
    constexpr int NWAVES = 8, RING = 2 * BS, HT = 8, CB = 4, NM = kIvfKloopMinima;
    constexpr int kSlots = 64 * NWAVES;                      // query slots per work item
    constexpr int PPS = TPS / HT;                            // passes per span
    constexpr int SPANROWS = TPS * 16, BINROWS = TPS * 4;
    static_assert(TPS % HT == 0 && TPS <= 64, "the tile number must fit the 6-bit id");
    static_assert(HT == NWAVES, "one 1-KiB piece per wave and stage");
    constexpr int kStageVec = HT * 64;                       // 16-byte vectors per K-step stage (8 KiB)
    __shared__ __attribute__((aligned(16))) unsigned char smem[RING * kStageVec * 16];
    __shared__ int s_min[NWAVES][NM * CB][64];               // the running minima of the current bins, between passes (ivf_kloop.hpp)
    auto lds_a = [&](int buf) { return reinterpret_cast<int4v *>(smem + buf * (kStageVec * 16)); };
    const int mode = a.info->i8_mode;
    if (!mode) return;                                       // this batch is served by ivf_kloop_scan_kernel

    const int it = blockIdx.x;
    if (it >= *a.n_items) return;
    const int l = a.item_list[it];
    int64_t span0 = a.list_pspan0[l], span1 = a.list_pspan0[l + 1];
    const int64_t lspan0 = span0;
    const int nb_item = (int)(span1 - span0) * 4;            // bins per query slot in this item
    if (a.part_spans > 0) {
        span0 += (int64_t)blockIdx.y * a.part_spans;
        if (span0 + a.part_spans < span1) span1 = span0 + a.part_spans;
    }
    if (span0 >= span1) return;                              // (a part beyond the list's end, or an empty list)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;                                 // lane group = bin of the span
    const int nK = a.nk, shift = a.shift;
    const int slot0 = a.item_slot0[it] + wave * 64;
    const size_t bin_base = (size_t)a.item_bin0[it];
    const int32_t *bias = a.bias8 + ((mode & 3) == 1 ? 0 : a.npad);
    const int npass = (int)(span1 - span0) * PPS;
    const int nsteps = npass * nK;

    // the queries behind this wave's slots: per column block one byte offset into qrows (row pitch 64 nK bytes)
    int qoff[CB];
    bool any_query = false;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int qi = a.slot_query[slot0 + cb * 16 + (lane & 15)] - 1;      // (-1: padding slot)
        any_query |= qi >= 0;
        qoff[cb] = (qi < 0 ? 0 : qi) * (nK * 64) + g * 16;
    }
    const bool live = __builtin_amdgcn_readfirstlane((int)(__ballot(any_query) != 0ull)) != 0;

    const int lane16 = lane * 16;
    auto stage_issue = [&](int step, int buf) {              // A panels of K-step `step` -> LDS slot: wave w brings tile w of the pass
        const int pass = step / nK, kk = step - pass * nK;
        const int64_t tile0 = (span0 + pass / PPS) * TPS + (pass % PPS) * HT;
        const int4v *base = a.panels + ((size_t)tile0 * nK + kk) * 64;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int4v *>(base), 0, 0x7fffffff, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, reinterpret_cast<__attribute__((address_space(3))) void *>(
                    static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_a(buf) + wave * 64))),
            16, lane16, wave * nK * 1024, 0, 0);
    };
    // the wait that goes with the barrier: this wave's LDS-DMA requests (and B loads) have landed
    auto stage_barrier = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };

#pragma unroll
    for (int i = 0; i < BS; ++i) stage_issue(i < nsteps ? i : nsteps - 1, i);
    // A wave whose 64 slots are all padding keeps its share of the A staging and the barriers going and nothing else: one barrier up
    // front and one after every K-step with step % BS == BS - 1, as the live waves below -- whatever nsteps is a multiple of
    if (!live) {
        stage_barrier();
        for (int step = 0; step < nsteps; ++step) {
            stage_issue(step + BS < nsteps ? step + BS : nsteps - 1, (step + BS) % RING);
            if (BS == 1 || (step % BS) == BS - 1) stage_barrier();
        }
        return;
    }

    const int INF = (int)kI8Inf;
#pragma unroll
    for (int i = 0; i < NM * CB; ++i) s_min[wave][i][lane] = INF;

    int4v bq[CB], bqn[CB];
    const __amdgpu_buffer_rsrc_t rsq = __builtin_amdgcn_make_buffer_rsrc(const_cast<signed char *>(a.qrows), 0, 0x7fffffff, 0x00020000);
    auto load_b = [&](int kk, int4v(&dst)[CB]) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
            dst[cb] = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(rsq, qoff[cb], kk * 64, 0));
    };
    load_b(0, bq);
    stage_barrier();

    int4v fr[2][4];
    auto read_group = [&](int buf, int half, int4v(&dst)[4]) {   // tiles 4 half .. 4 half + 3 of the stage
        const int4v *A = lds_a(buf);
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[t] = A[(half * 4 + t) * 64 + lane];
    };
    read_group(0, 0, fr[0]);

    int4v acc[HT][CB];
    int step = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const int64_t span = span0 + pass / PPS;
        const int slice = pass % PPS;
        // accumulators start from the integer init of their rows: local row = BINROWS g + 4 (HT slice + t) + i
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const int4v c = *reinterpret_cast<const int4v *>(bias + span * SPANROWS + g * BINROWS + (slice * HT + t) * 4);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) acc[t][cb] = c;
        }
#pragma unroll 1
        for (int kk = 0; kk < nK; ++kk, ++step) {
            const int buf = step % RING;
            load_b(kk + 1 == nK ? 0 : kk + 1, bqn);          // (B repeats every pass)
            // (past the end of the part the last stage is requested again into a slot nobody reads)
            stage_issue(step + BS < nsteps ? step + BS : nsteps - 1, (step + BS) % RING);
            __builtin_amdgcn_sched_barrier(0);
            read_group(buf, 1, fr[1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    acc[t][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fr[0][t], bq[cb], acc[t][cb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            // the barrier that publishes the next BS stages and frees the ones just read sits in front of this K-step's last 16
            // MFMAs (scan16_i8_kloop_kernel)
            if (BS == 1 || (step % BS) == BS - 1) stage_barrier();
            read_group((step + 1) % RING, 0, fr[0]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    acc[4 + t][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fr[1][t], bq[cb], acc[4 + t][cb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) bq[cb] = bqn[cb];
        }
        // epilogue of the pass.  m[0] <= m[1] <= ...: sorted insertion by one v_min_i32 + (NM - 1) v_med3_i32 per candidate group
        int m[NM][CB];
#pragma unroll
        for (int i = 0; i < NM; ++i)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) m[i][cb] = s_min[wave][i * CB + cb][lane];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const unsigned id = (unsigned)__builtin_amdgcn_readfirstlane(slice * HT + t);    // tile number inside the span = quad number inside the bin
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                auto insert = [&](int score, unsigned gid) {
                    const int v = (int)(((unsigned)(score >> shift) << 6) | gid);
#pragma unroll
                    for (int i = NM - 1; i > 0; --i) m[i][cb] = imed3(m[i - 1][cb], m[i][cb], v);
                    m[0][cb] = imin(m[0][cb], v);
                };
                if (GROUP == 4) {
                    insert(imin(imin(acc[t][cb][0], acc[t][cb][1]), imin(acc[t][cb][2], acc[t][cb][3])), id);
                } else if (GROUP == 2) {
                    insert(imin(acc[t][cb][0], acc[t][cb][1]), 2 * id);
                    insert(imin(acc[t][cb][2], acc[t][cb][3]), 2 * id + 1);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) insert(acc[t][cb][i], 4 * id + i);
                }
            }
        }
        if (slice == PPS - 1) {                              // the four bins (span, g) are complete: [item][slot][bin]
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const size_t o = bin_base * kSlots + (size_t)(wave * 64 + cb * 16 + (lane & 15)) * nb_item +
                                 (size_t)((span - lspan0) * 4 + g);
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    a.bin_m[i][o] = __int_as_float(m[i][cb]);
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

// ---- build: the int8 copy of the list-padded panel space (span = tps tiles; span_row0 / span_valid as ivf_mfma.hpp) ----------------
// panels8[tile][K-step][lane][16 x int8]: tile t of a span, lane l holds MFMA row l & 15 = 4 g + i <-> local row 4 tps g + 4 t + i (the
// p16 mapping of ivf_build_panels16_kernel), dims 64 ks + 16 (l >> 4) .. +15, value x - cx (0 beyond D or the list's end)
__global__ __launch_bounds__(256) void ivf_build_panels16_i8_kernel(const float *__restrict__ X, int D, int D4, int nk, int tps,
                                                                    int64_t ntiles, int cx, const int32_t *__restrict__ span_row0,
                                                                    const int32_t *__restrict__ span_valid, int4v *__restrict__ panels) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gid & 63);
    const int64_t tk = gid >> 6;
    const int ks = (int)(tk % nk);
    const int64_t tile = tk / nk;
    if (tile >= ntiles) return;
    const int rho = lane & 15, g = rho >> 2, i = rho & 3;
    const int64_t span = tile / tps;
    const int t = (int)(tile - span * tps);
    const int local = 4 * tps * g + 4 * t + i;
    const bool valid = local < span_valid[span];
    const int64_t row = (int64_t)span_row0[span] + local;
    const int d0 = ks * 64 + (lane >> 4) * 16;
    int4v out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int d = d0 + 4 * w + b;
            int v = 0;
            if (valid && d < D) v = (int)X[(size_t)row * D4 + d] - cx;
            word |= ((unsigned)v & 0xffu) << (8 * b);
        }
        out[w] = (int)word;
    }
    panels[gid] = out;
}

// accumulator inits bias8[w][span * span_rows + local row] for both query windows (w = 0: cq = 127, 1: cq = -1) with the handle's key
// rule (build_bias_i8k_kernel: the same values, addressed through the span tables), pad on padding rows; and rowstat[row] =
// {sum x^2, sum x} of the list-order rows for the int8 list refine.  One thread per slot of the panel space.
__global__ __launch_bounds__(256) void ivf_build_bias_i8k_kernel(const float *__restrict__ X, int64_t nspans, int span_rows, int D, int D4,
                                                                 int metric, long long offset, int pad,
                                                                 const int32_t *__restrict__ span_row0, const int32_t *__restrict__ span_valid,
                                                                 int32_t *__restrict__ bias8, int *__restrict__ rowstat) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t npad = nspans * span_rows;
    if (gid >= npad) return;
    const int64_t span = gid / span_rows;
    const int local = (int)(gid - span * span_rows);
    if (local >= span_valid[span]) {
        bias8[gid] = pad;
        bias8[npad + gid] = pad;
        return;
    }
    const int64_t row = (int64_t)span_row0[span] + local;
    long long n2 = 0, s1 = 0;
    for (int d = 0; d < D; ++d) {
        const long long v = (long long)X[(size_t)row * D4 + d];
        n2 += v * v;
        s1 += v;
    }
    rowstat[2 * row] = (int)n2;
    rowstat[2 * row + 1] = (int)s1;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const long long cq = w == 0 ? 127 : -1;
        const long long b = metric == 0 ? ((n2 - 2 * cq * s1) >> 1) : -cq * s1;    // (>> on a negative: floor)
        bias8[(size_t)w * npad + gid] = (int32_t)(b + offset);
    }
}

}  // namespace vdb

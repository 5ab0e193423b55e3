// scan16_i8.hpp -- the int8 K-loop scan: byte-valued corpora of D > 128 on v_mfma_i32_16x16x64_i8 (option "i8_kloop").
//
// The int8 twin of scan16_kloop_kernel (scan16.hpp; read that header first): same p16 row mapping, same bins and superbins,
// same outputs -- bin_m1 / bin_m2 / sb_m1 / sb_m2 / sb_span, a packed minimum's 6-bit id = the tile number inside the span --
// so select and refine run unchanged behind it.  What differs is everything inside:
//   arithmetic   A = x - cx, B = cq - q in int8, exact int32 accumulation from a per-row integer init (bias8 of the batch's
//                query window): no error bound, the select widens by the dropped parity bit only (prep.hpp, query_eps_body)
//   stage        one 64-dim K-step of a pass = 8 tiles x 1 KiB = 8 KiB of A panels (half the fp16 stage for the same
//                dimensions), ONE buffer-addressed LDS-DMA request per wave; the ring holds 2 BS stages and the workgroup
//                meets at a barrier every BS K-steps (BS = 2: 128 dimensions and 64 MFMAs per wave between barriers)
//   MFMAs        32 per K-step and wave (8 tiles x 4 column blocks), A fragments pipelined one group of 4 tiles ahead
//   B fragments  one 16-byte fragment per column block and K-step, streamed from L2 one K-step ahead into a second register
//                set (the fp16 kernel reloads its two k-steps in place; here a K-step IS one k-step)
//   epilogue     per quad  min of the four accumulators, >> shift, v_lshl_or with the id, med3 + min  -- the key format of
//                the handle (i8k_plan.hpp); stores are float bit patterns
// Which of the two K-loop scans serves a batch is decided on the device (QueryBatchInfo.i8_mode): both are enqueued, the one
// not needed returns at once.
#pragma once
#include "i8k_plan.hpp"
#include "scan16.hpp"
#include "scan_i8.hpp"

namespace vdb {

static_assert(kI8kPadKey == kI8PadBias && kI8kInf == kI8Inf, "i8k_plan.hpp restates the constants of common.hpp");

// ---- build: int8 A panels in p16 order ---------------------------------------------------------------------------------------
// panels8[tile][K-step][lane][16 x int8]: lane l holds MFMA row l & 15 -- corpus row 1024 span + 256 (row >> 2) + 4 t + (row & 3),
// the p16 mapping of common.hpp -- dims 64 ks + 16 (l >> 4) .. +15, value x - cx (0 beyond D or N).  One thread per 16 bytes.
__global__ __launch_bounds__(256) void build_panels16_i8_kernel(const float *__restrict__ X, int64_t N, int D, int D4, int nk,
                                                                int64_t ntiles, int cx, int4v *__restrict__ panels) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gid & 63);
    const int64_t tk = gid >> 6;
    const int ks = (int)(tk % nk);
    const int64_t tile = tk / nk;
    if (tile >= ntiles) return;
    const int rho = lane & 15, g = rho >> 2, i = rho & 3;
    const int64_t span = tile / kTilesPerSpan16;
    const int t = (int)(tile - span * kTilesPerSpan16);
    const int64_t row = span * kSpanRows16 + (int64_t)g * kBinRows + 4 * t + i;
    const int d0 = ks * 64 + (lane >> 4) * 16;
    int4v out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int d = d0 + 4 * w + b;
            int v = 0;
            if (row < N && d < D) v = (int)X[(size_t)row * D4 + d] - cx;
            word |= ((unsigned)v & 0xffu) << (8 * b);
        }
        out[w] = (int)word;
    }
    panels[gid] = out;
}

// accumulator init per row for both query windows, bias8[w][row] (w = 0: cq = 127, 1: cq = -1), with the handle's key rule:
//   L2: floor((||x||^2 - 2 cq sum(x)) / 2) + offset     IP: -cq sum(x) + offset     padding rows: pad
// and rowstat[row] = {sum x^2, sum x} for the int8 list refine
__global__ __launch_bounds__(256) void build_bias_i8k_kernel(const float *__restrict__ X, int64_t N, int64_t Npad, int D, int D4,
                                                             int metric, long long offset, int pad, int32_t *__restrict__ bias8,
                                                             int *__restrict__ rowstat) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= Npad) return;
    if (row >= N) {
        bias8[row] = pad;
        bias8[Npad + row] = pad;
        return;
    }
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
        bias8[(size_t)w * Npad + row] = (int32_t)(b + offset);
    }
}

// ---- the scan --------------------------------------------------------------------------------------------------------------------
// ScanArgs as scan16_kloop_kernel takes them, with the int8 operands behind the pointers: panels = the int8 A panels above,
// bias = bias8 (int32 [2][npad]), qpanels = the int8 B fragments [q / 16][K-step][lane] (build_qpanels_i8_kernel, 16-query form).
struct ScanI8KloopExtra {
    int nk;        // 64-dim K-steps (D padded to 64 nk)
    int qgroup;    // query tiles per group of the block order (as ScanKloopExtra)
    int shift;     // key rule of the handle
    int64_t npad;  // rows of one query window of bias8
};

template <int BS>
__global__ __launch_bounds__(512, 2) void scan16_i8_kloop_kernel(ScanArgs a, ScanI8KloopExtra ex) {
    constexpr int NWAVES = 8, RING = 2 * BS, HT = 8, CB = 4;
    constexpr int PPS = kTilesPerSpan16 / HT;               // passes per span (8): a pass = 8 tiles = 32 rows of each of the four bins
    constexpr int kStageVec = HT * 64;                      // 16-byte vectors per K-step stage (8 KiB)
    static_assert(HT == NWAVES, "one 1-KiB piece per wave and stage");
    __shared__ __attribute__((aligned(16))) unsigned char smem[RING * kStageVec * 16];
    auto lds_a = [&](int buf) { return reinterpret_cast<int4v *>(smem + buf * (kStageVec * 16)); };
    const int mode = a.info->i8_mode;
    if (!mode) return;                                      // this batch is served by scan16_kloop_kernel

    const int b = blockIdx.x;
    const int x = b & 7, j = b >> 3;
    const int cpx = (a.nchunks + 7) >> 3;                   // chunks per XCD label
    const int per_group = cpx * ex.qgroup;
    const int qg = j / per_group, rem = j - qg * per_group;
    const int ci = rem / ex.qgroup, qt = qg * ex.qgroup + (rem - ci * ex.qgroup);
    if (x + 8 * ci >= a.nchunks || qt >= a.nqtiles) return;
    const int chunk = x + 8 * ci;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;                                // lane group = bin of the span
    const int nK = ex.nk;
    const int shift = ex.shift;
    const int64_t q0 = (int64_t)qt * (NWAVES * 16 * CB) + wave * (16 * CB);
    const int4v *panels = reinterpret_cast<const int4v *>(a.panels);
    const int32_t *bias = reinterpret_cast<const int32_t *>(a.bias) + ((mode & 3) == 1 ? 0 : ex.npad);

    const int64_t span0 = chunk_span0(chunk, a.spans_per_chunk, a.chunk_rem);
    int64_t span1 = chunk_span0(chunk + 1, a.spans_per_chunk, a.chunk_rem);
    if (span1 > a.nspans) span1 = a.nspans;
    const int npass = (int)(span1 - span0) * PPS;
    const int nsteps = npass * nK;
    if (nsteps <= 0) return;

    const int INF = (int)kI8Inf;
    int m1[CB], m2[CB], M1[CB], M2[CB], Ms[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        m1[cb] = m2[cb] = M1[cb] = M2[cb] = INF;
        Ms[cb] = 0;
    }

    const int lane16 = lane * 16;
    auto stage_issue = [&](int step, int buf) {             // A panels of K-step `step` -> LDS slot: wave w brings tile w of the pass
        const int pass = step / nK, kk = step - pass * nK;
        const int64_t tile0 = (span0 + pass / PPS) * kTilesPerSpan16 + (pass % PPS) * HT;
        const int4v *base = panels + ((size_t)tile0 * nK + kk) * 64;
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
    // A wave whose 64 query columns are all padding keeps its share of the A staging and the barriers going and nothing else
    if (a.nq_valid > 0 && q0 >= a.nq_valid) {
        stage_barrier();
        for (int step = 0; step < nsteps; ++step) {
            stage_issue(step + BS < nsteps ? step + BS : nsteps - 1, (step + BS) % RING);
            if (BS == 1 || (step % BS) == BS - 1) stage_barrier();
        }
        return;
    }

    int4v bq[CB], bqn[CB];
    const __amdgpu_buffer_rsrc_t rsq = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int4v *>(reinterpret_cast<const int4v *>(a.qpanels) + (size_t)(q0 / 16) * nK * 64), 0, 0x7fffffff, 0x00020000);
    auto load_b = [&](int kk, int4v(&dst)[CB]) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
            dst[cb] = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(rsq, lane16, (cb * nK + kk) * 1024, 0));
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
        // accumulators start from the integer init of their rows: row = 1024 span + 256 g + 4 (HT slice + t) + i
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const int4v c = *reinterpret_cast<const int4v *>(bias + span * kSpanRows16 + g * kBinRows + (slice * HT + t) * 4);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) acc[t][cb] = c;
        }
#pragma unroll 1
        for (int kk = 0; kk < nK; ++kk, ++step) {
            const int buf = step % RING;
            load_b(kk + 1 == nK ? 0 : kk + 1, bqn);          // (B repeats every pass)
            // (past the end of the chunk the last stage is requested again into a slot nobody reads)
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
            // MFMAs: a wave leaves it with matrix work in hand while its first fragments of the next K-step are in flight
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
        // epilogue of the pass: one quad per (tile, column block); id = the tile's number inside the span
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const unsigned id = (unsigned)__builtin_amdgcn_readfirstlane(slice * HT + t);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const int qm = imin(imin(acc[t][cb][0], acc[t][cb][1]), imin(acc[t][cb][2], acc[t][cb][3]));
                const int v = (int)(((unsigned)(qm >> shift) << 6) | id);
                m2[cb] = imed3(m1[cb], m2[cb], v);
                m1[cb] = imin(m1[cb], v);
            }
        }
        if (slice == PPS - 1) {      // the four bins (span, g) are complete
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const size_t o = (size_t)(span * 4 + g) * a.Qpad + q0 + cb * 16 + (lane & 15);
                a.bin_m1[o] = __int_as_float(m1[cb]);
                a.bin_m2[o] = __int_as_float(m2[cb]);
                M2[cb] = imin(imed3(M1[cb], M2[cb], m1[cb]), m2[cb]);
                if (m1[cb] < M1[cb]) Ms[cb] = (int)span;
                M1[cb] = imin(M1[cb], m1[cb]);
                m1[cb] = INF;
                m2[cb] = INF;
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const size_t so = (size_t)(chunk * 4 + g) * a.Qpad + q0 + cb * 16 + (lane & 15);
        a.sb_m1[so] = __int_as_float(M1[cb]);
        a.sb_m2[so] = __int_as_float(M2[cb]);
        a.sb_span[so] = Ms[cb];
    }
}

}  // namespace vdb

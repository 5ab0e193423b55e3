// range_i8.hpp -- the range prefilter on the int8 scan copy (option "range_i8"; host side: range.inc; rules: range_plan.hpp;
// DESIGN 4.13 "int8 prefilter").
//
// An integer query batch in the byte window of an index with an int8 copy in layout "x16" needs no error bound: the accumulators
// of v_mfma_i32_16x16x64_i8 are exact, so the candidate bitmap comes from ONE integer comparison per (query, row) against
// thr8[q] = range_i8_thr(...) -- for IP exactly the answer (radii below 2^27, range_plan.hpp), for L2 the answer and the keys in
// [radius, radius + 1) that the parity bit dropped from the accumulator init cannot tell apart.  Operands are those of scan_i8x16_kernel: panels8 ([tile][2 ks2 + rb]
// [lane], x16_row_in_span), bias8[w] with w from the query window, qpanels8 from build_qpanels_i8_kernel(.., x16 = 1).
//
// Work split (the scan's, not the fp16 range scan's): a workgroup is 8 waves, a wave holds CB column blocks of 16 queries (CB = 8:
// 1024 queries per workgroup, CB = 4: 512 for short slabs) with all CB x KS2 B fragments in registers for its whole life, and walks
// a chunk of 512-row spans.  A fragments and accumulator inits of a stage (ST = 8 tiles: 16 or 32 KiB + 1 KiB) arrive by LDS-DMA
// in a ring of two buffers: stage s + 1 is requested before the MFMAs of stage s, one full wait and one barrier per stage.  (The
// three-buffer hand-over of scan_ring.hpp was not tried here: it pays when the step behind the barrier would otherwise start
// with LDS reads in all eight waves at once, and this loop has no select to keep fed across the barrier.  Not measured.)
// The grid is (span chunks, query tiles): the panels are read once per 1024 queries, against once per 128 in range_scan_x16_kernel.
//
// Per tile and wave: 2 KS2 CB MFMAs, the next tile's 2 KS2 + 2 LDS reads, and the SCREEN -- per column block the minimum of the
// lane's 8 scores (3 v_min3_i32 + 1 v_min_i32) and one v_cmp_le_i32 against thr8 into a scalar mask: 5 vector instructions per
// 2 KS2 MFMAs (KS2 = 2: 40 beside 32 MFMAs, 20 cycles of vector issue in the 32 the MFMAs of a column block leave free), one
// s_or_b64 per column block and ONE wave-uniform branch per tile.  Results are rare (about 1e-5 of the pairs at the radius of the
// 10th neighbour), so the extraction -- v_cmp + v_cndmask + v_or per accumulator register, 24 per column block, and 8 to place
// the byte in the lane's words -- runs only for a column block whose mask is not empty.  The comparison's scalar masks are turned
// into vector registers by v_cndmask; the bitmap is written from vector registers with ordinary 16-byte stores.
// Not shipped: compare into the carry mask and shift the bit in with an add-with-carry (2 per register) -- it has to run on every
// tile to keep the bit positions, which is what the screen avoids; and folding thr8 into the accumulator init to gather sign bits
// -- the init is shared by the CB column blocks of a tile (one LDS read), a per-query init would take CB of them.  Neither was
// measured.
// Output: the bitmap of range_scan_x16_kernel.  Lane (q = lane & 15, g = lane >> 4) owns rows 512 s + 128 g .. + 127 of its query
// = four whole words, built in registers and stored as one 16-byte vector per (query, span, g), every word masked by row number
// (rows >= N are never masked by kI8PadBias: thr8 = INT32_MAX passes it).  Every (query < nq, word) is written: spans past the
// panels get zeros, queries with flag[q] != 0 all ones.
// Resources (gfx950, -O3, resource report of the build; VGPR / AGPR / scratch bytes / waves per SIMD / LDS bytes):
//   <KS2 = 1, CB = 8> 195 / 0 / 0 / 2 / 34 816     <1, 4> 119 / 0 / 0 / 4 / 34 816
//   <KS2 = 2, CB = 8> 254 / 0 / 0 / 2 / 67 584     <2, 4> 150 / 0 / 0 / 3 / 67 584
// The CB = 8 forms therefore run ONE workgroup per CU (2 waves per SIMD): while its eight waves sit in the full wait and the barrier
// at the end of a stage nothing else on the CU issues -- the cost the three-buffer ring of the scan was built to remove.
// Measured (profiles/r27_bench_range_i8.json): this shape only; none of the variants named above.
#pragma once
#include "range.hpp"
#include "scan_i8x16.hpp"

namespace vdb {

// ---- per-query integer threshold ---------------------------------------------------------------------------------------------
// i8_mode != 0: thr8[q] from the query's ||q||^2 and sum(q) (integers in the byte window: exact), flag 0.
// i8_mode == 0: nothing on a handle that also has the fp16 prefilter; on an "int8_only" handle (fill) flag 1 -- every row is a
// candidate -- and the query is counted as a fallback query.
struct RangeThr8Args {
    const float *Q;          // [nq][D]
    int64_t nq;
    int D, metric;
    float radius;
    int cx;                  // byte window of the corpus copy: 128 or 0
    int fill;                // no fp16 prefilter on this handle
    const QueryBatchInfo *info;
    int *thr8;               // [nq]
    int *flag;               // [nq]
    unsigned long long *stat;    // sharded counters: [1] += fallback queries
};

__global__ __launch_bounds__(256) void range_thr8_kernel(RangeThr8Args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nq) return;
    const int mode = a.info->i8_mode;
    if (!mode) {
        if (!a.fill) return;
        a.thr8[q] = kRangeThr8All;
        a.flag[q] = 1;
        stat_add(a.stat, q, 1, 1ull);
        return;
    }
    const int cq = (mode & 3) == 1 ? 127 : -1;
    const float *row = a.Q + (size_t)q * a.D;
    long long q2 = 0, sq = 0;
    for (int d = 0; d < a.D; ++d) {
        const long long v = (long long)row[d];
        q2 += v * v;
        sq += v;
    }
    a.thr8[q] = range_i8_thr(a.metric, a.radius, range_i8_kq(a.metric, q2, sq, a.D, a.cx, cq), kI8Offset);
    a.flag[q] = 0;
}

// ---- the prefilter -------------------------------------------------------------------------------------------------------------
struct RangeI8Args {
    const int4v *panels;     // [ntiles][2 KS2][64], layout "x16"
    const int32_t *bias8;    // [2][Npad]
    const int4v *qpanels;    // B fragments of the slab, [qpad / 16][KS2][64]
    const QueryBatchInfo *info;
    const int *thr8;         // [nq] of the slab
    const int *flag;
    int64_t nq, N, Npad, W;
    int64_t nspans;          // spans of the panels (Npad / 512)
    int64_t bspans;          // spans of a bitmap row (W / 16 >= nspans)
    int spans_per_chunk;
    int fill;                // i8_mode == 0: write all ones (an "int8_only" handle) instead of returning
    unsigned *bitmap;        // [nq][W]
};

template <int KS2, int CB>
__global__ __launch_bounds__(kRangeI8Waves * 64, 2) void range_scan_i8x16_kernel(RangeI8Args a) {
    constexpr int NW = kRangeI8Waves, ST = kRangeI8StageTiles, NV = 2 * KS2, TPS = kTilesPerSpan, SPS = TPS / ST;
    constexpr int kStageVec = ST * NV * 64, kABytes = kStageVec * 16, kBBytes = ST * 32 * 4;
    constexpr int kPieces = kStageVec / 64;
    static_assert(kRangeI8Buffers == 2 && TPS % ST == 0 && kPieces % NW == 0 && ST / 2 <= NW, "bad geometry");
    static_assert(range_i8_lds_bytes(KS2) == kRangeI8Buffers * (kABytes + kBBytes), "LDS size");
    __shared__ __attribute__((aligned(16))) unsigned char smem[range_i8_lds_bytes(KS2)];
    auto lds_a = [&](int buf) { return reinterpret_cast<int4v *>(smem + buf * kABytes); };
    auto lds_b = [&](int buf) { return reinterpret_cast<int *>(smem + kRangeI8Buffers * kABytes + buf * kBBytes); };

    const int mode = a.info->i8_mode;
    if (!mode && !a.fill) return;                              // this batch is served by the fp16 prefilter
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t span0 = (int64_t)blockIdx.x * a.spans_per_chunk;
    int64_t span1 = span0 + a.spans_per_chunk;
    if (span1 > a.bspans) span1 = a.bspans;
    if (span0 >= span1) return;
    const int64_t q0 = ((int64_t)blockIdx.y * NW + wave) * (16 * CB);
    const bool live = q0 < a.nq;                               // (wave-uniform) some query column of this wave is real
    const int64_t qlane = q0 + (lane & 15);

    // one 16-byte store per (query, span, lane group): words 16 s + 4 g .. + 3 of the query's row
    auto store_span = [&](int64_t span, int cb, unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
        const int64_t q = qlane + cb * 16, wbase = span * kRangeI8SpanWords + g * 4;
        if (q >= a.nq) return;
        range_uint4 o;
        o[0] = w0 & range_mask_dev(wbase, a.N);
        o[1] = w1 & range_mask_dev(wbase + 1, a.N);
        o[2] = w2 & range_mask_dev(wbase + 2, a.N);
        o[3] = w3 & range_mask_dev(wbase + 3, a.N);
        *reinterpret_cast<range_uint4 *>(a.bitmap + (size_t)q * a.W + wbase) = o;
    };
    if (!mode) {                                               // "int8_only", a batch outside the byte window: every row is a candidate
        if (!live) return;
        for (int64_t s = span0; s < span1; ++s)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) store_span(s, cb, ~0u, ~0u, ~0u, ~0u);
        return;
    }

    const int32_t *bias = a.bias8 + ((mode & 3) == 1 ? 0 : a.Npad);
    int64_t scan1 = span1 < a.nspans ? span1 : a.nspans;       // spans [span0, scan1) have panels, [scan1, span1) get zeros
    if (scan1 < span0) scan1 = span0;
    const int nstages = (int)(scan1 - span0) * SPS;

    int4v bq[CB][KS2];
    int thr[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int64_t q = qlane + cb * 16;
        const bool valid = q < a.nq;
        thr[cb] = valid ? (a.flag[q] ? kRangeThr8All : a.thr8[q]) : kRangeThr8None;
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) {
            const int4v zero = {0, 0, 0, 0};
            bq[cb][ks] = live ? a.qpanels[((size_t)(q0 / 16 + cb) * KS2 + ks) * 64 + lane] : zero;
        }
    }

    // stage st of the chunk into buffer buf: the A fragments in kPieces pieces of 64 x 16 bytes, dealt over the waves, and the
    // accumulator inits in ST / 2 pieces of 64 ints = two tiles x [lane group][8 consecutive rows] (bias8 is in corpus order)
    auto stage_issue = [&](int st, int buf) {
        const int64_t span = span0 + st / SPS;
        const int sq = st % SPS;
        const int4v *src = a.panels + ((size_t)(span * TPS + sq * ST) * NV) * 64;
        int4v *dst = lds_a(buf);
#pragma unroll
        for (int i = 0; i < kPieces / NW; ++i) {
            const int p = wave + i * NW;
            const int4v *gp = src + p * 64 + lane;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(gp)),
                reinterpret_cast<__attribute__((address_space(3))) void *>(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst + p * 64))),
                16, 0, 0);
        }
        if (wave < ST / 2) {
            const int t = 2 * wave + (lane >> 5), gg = (lane >> 3) & 3, e = lane & 7;
            const int32_t *gp = bias + span * kSpanRows + gg * 128 + (sq * ST + t) * 8 + e;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(gp)),
                reinterpret_cast<__attribute__((address_space(3))) void *>(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_b(buf) + wave * 64))),
                4, 0, 0);
        }
    };
    auto stage_wait = [&]() {                                  // this wave's pieces have landed, then everybody's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };

    unsigned w[CB][4];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) w[cb][0] = w[cb][1] = w[cb][2] = w[cb][3] = 0u;

    if (nstages > 0) {
        stage_issue(0, 0);
        stage_wait();
    }
    for (int st = 0; st < nstages; ++st) {
        const int buf = st & 1;
        if (st + 1 < nstages) stage_issue(st + 1, buf ^ 1);
        if (live) {
            const int4v *A = lds_a(buf) + lane;
            const int4v *B4 = reinterpret_cast<const int4v *>(lds_b(buf)) + g * 2;
            const int ts0 = (st % SPS) * ST;                   // first tile of the stage in its span (wave-uniform)
            int4v fr[NV], cin[2], acc[2][CB];
#pragma unroll
            for (int v = 0; v < NV; ++v) fr[v] = A[v * 64];
            cin[0] = B4[0];
            cin[1] = B4[1];
#pragma unroll
            for (int t = 0; t < ST; ++t) {
#pragma unroll
                for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb)
                            acc[rb][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fr[2 * ks + rb], bq[cb][ks], ks == 0 ? cin[rb] : acc[rb][cb], 0, 0, 0);
                if (t + 1 < ST) {                              // the next tile's operands, behind the MFMAs that read these registers
#pragma unroll
                    for (int v = 0; v < NV; ++v) fr[v] = A[((t + 1) * NV + v) * 64];
                    cin[0] = B4[(t + 1) * 8];
                    cin[1] = B4[(t + 1) * 8 + 1];
                }
                // screen: does any of the lane's 8 rows pass, in any lane, in any column block?
                unsigned long long hit[CB], any = 0ull;
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const int t1 = imin(imin(acc[0][cb][0], acc[0][cb][1]), acc[0][cb][2]);
                    const int t2 = imin(imin(acc[0][cb][3], acc[1][cb][0]), acc[1][cb][1]);
                    const int m = imin(imin(imin(acc[1][cb][2], acc[1][cb][3]), t1), t2);
                    hit[cb] = __ballot(m <= thr[cb]);
                    any |= hit[cb];
                }
                if (any) {                                     // rare: extract the bits of the column blocks that have one
                    const int jw = (ts0 + t) >> 2;             // word of this tile among the lane's four (wave-uniform)
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) {
                        if (!hit[cb]) continue;
                        unsigned bits = 0u;
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                            for (int i = 0; i < 4; ++i) bits |= acc[rb][cb][i] <= thr[cb] ? 1u << (4 * rb + i) : 0u;
                        bits <<= 8 * (t & 3);                  // (ST is a multiple of 4: tile t of the stage and of the span share t & 3)
#pragma unroll
                        for (int j = 0; j < 4; ++j) w[cb][j] |= j == jw ? bits : 0u;
                    }
                }
            }
            if (ts0 + ST == TPS) {                             // the span is complete
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    store_span(span0 + st / SPS, cb, w[cb][0], w[cb][1], w[cb][2], w[cb][3]);
                    w[cb][0] = w[cb][1] = w[cb][2] = w[cb][3] = 0u;
                }
            }
        }
        stage_wait();
    }
    if (!live) return;
    for (int64_t s = scan1; s < span1; ++s)                    // bitmap spans past the panels
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) store_span(s, cb, 0u, 0u, 0u, 0u);
}

}  // namespace vdb

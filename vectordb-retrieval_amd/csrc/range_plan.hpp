// range_plan.hpp -- the sizes of a range search (range.hpp, range.inc): words of a query's bitmap row, segments of the exact
// filter, query slabs under the bitmap budget.  No HIP: tests/host/range_plan_main.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

namespace vdb {

// One bit per (query, row): bit r % 32 of word r / 32 of the query's bitmap row.  A row of the bitmap covers the corpus padded to
// whole 1024-row spans (the larger of the two scan layouts: "x16" spans are 512 rows, p16 spans 1024), so a lane of either scan
// stores whole 16-byte groups of words and every query's row starts 16-byte aligned.
constexpr int kRangeWordBits = 32;
constexpr int kRangeRowAlign = 1024;          // rows a bitmap row is padded to
constexpr int kRangeSegWords = 64;            // words per segment of the exact filter: one wave, one word per lane (2048 rows)
constexpr int kRangeQueryTile = 128;          // queries per workgroup of the prefilter scans (4 waves x 2 blocks of 16)
constexpr int kRangeBitmapMbDefault = 256;    // option "range_bitmap_mb" = 0
constexpr int64_t kRangeSlabMaxQueries = 1 << 20;   // tiny corpora: the query tiles of a slab stay inside one grid dimension (8192 of 65 535)

inline int64_t range_words(int64_t N) {       // words per query row
    return (N + kRangeRowAlign - 1) / kRangeRowAlign * (kRangeRowAlign / kRangeWordBits);
}
inline int64_t range_segments(int64_t N) {    // segments per query row (the last one may be short)
    return (range_words(N) + kRangeSegWords - 1) / kRangeSegWords;
}
// bits of word `w` that name rows below N
inline uint32_t range_word_mask(int64_t w, int64_t N) {
    const int64_t left = N - w * kRangeWordBits;
    return left >= kRangeWordBits ? 0xffffffffu : left <= 0 ? 0u : ((1u << (int)left) - 1u);
}
inline int64_t range_budget_bytes(int bitmap_mb) {
    return (int64_t)(bitmap_mb > 0 ? bitmap_mb : kRangeBitmapMbDefault) << 20;
}
// queries per slab: as many bitmap rows as the budget holds, in whole query tiles once it holds one; never less than one query
// (a budget below one row: one query per slab), never more than the batch
inline int64_t range_slab_queries(int64_t nq, int64_t N, int bitmap_mb) {
    const int64_t row_bytes = range_words(N) * 4;
    int64_t fit = row_bytes > 0 ? range_budget_bytes(bitmap_mb) / row_bytes : nq;
    if (fit >= kRangeQueryTile) fit -= fit % kRangeQueryTile;
    if (fit > kRangeSlabMaxQueries) fit = kRangeSlabMaxQueries;
    if (fit < 1) fit = 1;
    return fit < nq ? fit : (nq > 0 ? nq : 1);
}
inline int64_t range_slabs(int64_t nq, int64_t N, int bitmap_mb) {
    const int64_t s = range_slab_queries(nq, N, bitmap_mb);
    return (nq + s - 1) / s;
}

// ---- the int8 prefilter (range_i8.hpp; option "range_i8") ----------------------------------------------------------------------
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VDB_RANGE_HD __host__ __device__
#else
#define VDB_RANGE_HD
#endif

// the handles it serves: an int8 scan copy in layout "x16" (both the default byte-valued handle and the "int8_only" one)
inline bool range_i8_route(int opt_range_i8, bool i8_ok, bool x16, bool has_panels8, bool has_bias8) {
    return opt_range_i8 != 0 && i8_ok && x16 && has_panels8 && has_bias8;
}

// Workgroup form: 8 waves, each CB column blocks of 16 queries, against a run of 512-row spans; A fragments and accumulator inits
// pass through two LDS buffers of ST = 8 tiles.  Slabs of up to 512 queries take the narrower form (CB = 4).
constexpr int kRangeI8Waves = 8;
constexpr int kRangeI8StageTiles = 8;
constexpr int kRangeI8Buffers = 2;
constexpr int kRangeI8SpanWords = 16;         // bitmap words per 512-row span
constexpr int kRangeI8MaxSpansPerChunk = 16;
constexpr int kRangeI8MinSpansPerChunk = 2;
constexpr int kRangeI8TargetBlocks = 512;     // two ROUNDS of the chip's 256 CUs: the CB = 8 forms need 195 / 254 VGPRs = 2 waves per SIMD,
                                              // i.e. ONE 8-wave workgroup per CU at a time (CB = 4: 4 / 3 waves per SIMD, one or two)

inline int range_i8_cb(int64_t slab_queries) { return slab_queries > 512 ? 8 : 4; }
inline int range_i8_query_tile(int cb) { return kRangeI8Waves * 16 * cb; }
struct RangeI8Grid {
    int cb = 0;               // column blocks per wave: 8 (1024-query tiles) or 4 (512)
    int spans_per_chunk = 0;  // bitmap spans a workgroup walks
    unsigned chunks = 0, qtiles = 0;          // grid.x, grid.y
    int64_t qpad = 0;         // queries the B fragments are built for: whole query tiles
};
// W: words per bitmap row (range_words): the bitmap has W / 16 spans, the last of which may lie past the panels
inline RangeI8Grid range_i8_grid(int64_t slab_queries, int64_t W) {
    RangeI8Grid g;
    g.cb = range_i8_cb(slab_queries);
    const int64_t qt = range_i8_query_tile(g.cb), bspans = W / kRangeI8SpanWords;
    g.qtiles = (unsigned)((slab_queries + qt - 1) / qt);
    g.qpad = (int64_t)g.qtiles * qt;
    int64_t spc = bspans * g.qtiles / kRangeI8TargetBlocks;
    if (spc > kRangeI8MaxSpansPerChunk) spc = kRangeI8MaxSpansPerChunk;
    if (spc < kRangeI8MinSpansPerChunk) spc = kRangeI8MinSpansPerChunk;
    g.spans_per_chunk = (int)spc;
    g.chunks = (unsigned)((bspans + spc - 1) / spc);
    return g;
}
// LDS of a workgroup: per buffer ST tiles x 2 KS2 fragments x 64 lanes x 16 bytes of A and ST x 32 accumulator inits
constexpr int range_i8_lds_bytes(int ks2) {
    return kRangeI8Buffers * (kRangeI8StageTiles * 2 * ks2 * 64 * 16 + kRangeI8StageTiles * 32 * 4);
}

// Threshold in accumulator units.  The accumulator of an integer pair holds t' with (common.hpp, "int8 scan copy")
//   L2: key = ||x - q||^2 = 2 (t' - offset) + parity + Kq,  Kq = ||q||^2 - 2 cx sum(q) + 2 D cx cq,  parity = ||x||^2 mod 2
//   IP: key = -x.q        =   (t' - offset) + Kq,           Kq = -cx sum(q) + D cx cq
// and the contract keeps a row when (float)key < radius (L2) / (float)(-key) > radius (IP).
constexpr int32_t kRangeThr8None = INT32_MIN, kRangeThr8All = INT32_MAX;
VDB_RANGE_HD inline int64_t range_i8_kq(int metric, int64_t q2, int64_t sq, int D, int cx, int cq) {
    return metric == 0 ? q2 - 2 * (int64_t)cx * sq + 2 * (int64_t)D * cx * cq : -(int64_t)cx * sq + (int64_t)D * cx * cq;
}
// the largest t' whose key can pass: IP exactly the pairs that pass; L2 those and the keys in [radius, radius + 1) that the
// dropped parity bit cannot tell apart.  Both statements hold for |radius| < 2^27: the search below for the integer next to the
// radius whose float32 image is strictly on its passing side takes at most 8 steps, which crosses a float32 gap of up to 8; beyond,
// the threshold errs towards MORE candidates (a superset, never a miss).  Every key of a byte-valued pair at D <= 128 is below 2^25.
// offset: kI8Offset.  Every step in double or int64; the result is clamped to int32.
VDB_RANGE_HD inline int32_t range_i8_thr(int metric, float radius, int64_t Kq, int32_t offset) {
    const double lim = 4.0e15;                // beyond every key; integers of this size are exact in double and int64
    const double r = (double)radius;
    double t;
    if (metric == 0) {
        if (!(radius > 0.f)) return kRangeThr8None;
        if (r > lim) return kRangeThr8All;
        int64_t m = (int64_t)__builtin_ceil(r) - 1;           // the largest integer below the radius ...
        for (int i = 0; i < 8 && !((float)m < radius); ++i) --m;   // ... whose float32 image is below it too (keys past 2^24)
        const int64_t a = m - Kq;
        t = (double)offset + (double)(a >= 0 ? a / 2 : -((-a + 1) / 2));      // floor(a / 2)
    } else {
        if (r > lim) return kRangeThr8None;
        if (r < -lim) return kRangeThr8All;
        int64_t v = (int64_t)__builtin_floor(r) + 1;          // the smallest integer score above the radius
        for (int i = 0; i < 8 && !((float)v > radius); ++i) ++v;
        t = (double)offset - (double)v - (double)Kq;
    }
    return t >= 2147483647.0 ? kRangeThr8All : t <= -2147483648.0 ? kRangeThr8None : (int32_t)t;
}

}  // namespace vdb

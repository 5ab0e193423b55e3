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

}  // namespace vdb

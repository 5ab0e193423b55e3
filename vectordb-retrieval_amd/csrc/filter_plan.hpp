// filter_plan.hpp -- the routing and sizing rules of a filtered search (filter.hpp, filter.inc): words of the allow
// bitmap, when the allowed-row list is kept, which route a call takes, how the sparse route cuts the list into splits.  No HIP:
// tests/host/filter_plan_main.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

#include "range_plan.hpp"

namespace vdb {

// One bit per row, the layout of range_plan.hpp: bit r % 32 of word r / 32 admits row r.
constexpr int kFilterSegWords = 64;                       // words per segment of the list prefix / emit: one wave, one word per lane
constexpr int kFilterMaxK = 2048;                         // vdb_search's largest k
constexpr int64_t kFilterSparsePairsDefault = 1 << 13;    // option "filter_sparse_pairs" as a handle starts out: the measured crossover
constexpr int kFilterRowsQB = 4;                          // queries per wave of the query-blocked sparse kernel
constexpr int kFilterSplitRows = 128;                     // list entries a split of the sparse route is worth: two wave iterations
constexpr int kFilterMaxSplits = 1024;
constexpr int64_t kFilterPartialBytes = (int64_t)256 << 20;   // partial lists of one sparse call: (query, split, k) x 16 bytes

inline int64_t filter_words_in(int64_t nbits) { return (nbits + kRangeWordBits - 1) / kRangeWordBits; }      // words the caller passes
inline int64_t filter_words(int64_t Npad) { return Npad / kRangeWordBits; }                                  // words the handle keeps (Npad: whole spans)
inline int64_t filter_segments(int64_t Npad) { return (filter_words(Npad) + kFilterSegWords - 1) / kFilterSegWords; }
inline uint32_t filter_word_mask(int64_t w, int64_t N) { return range_word_mask(w, N); }

// below this many admitted rows the select cannot find k live superbins reliably: every query would take the exhaustive fallback
inline int64_t filter_few_rows(int k) { return 2 * (int64_t)k + 64; }

// is the ascending list of admitted rows built at install?  Whenever some later call could take the sparse route: k is not known
// yet (so the largest k decides the first rule) and a call has at least one query (so n_allowed < sparse_pairs decides the second)
inline bool filter_keeps_list(int64_t n_allowed, int64_t sparse_pairs) {
    const int64_t few = filter_few_rows(kFilterMaxK);
    return n_allowed < (sparse_pairs > few ? sparse_pairs : few);
}

// does this call take the sparse route (VDB_PATH_FILTER_ROWS)?  force_path 1 / 2 / 3 keep their meaning: the exact kernels /
// the scan, masked.
inline bool filter_route_sparse(int64_t nq, int k, int64_t n_allowed, int64_t sparse_pairs, int force_path) {
    if (force_path != 0) return false;
    if (n_allowed < filter_few_rows(k)) return true;
    // (nq * n_allowed < sparse_pairs without the product: nq >= 1, n_allowed >= 1 here)
    return n_allowed < sparse_pairs && nq <= (sparse_pairs - 1) / n_allowed;
}

// the sparse kernel scores QB queries per wave only where a batch has whole groups to give and the top-k lists of QB queries fit
// the registers (k <= 128), as search_exact decides it for the exhaustive kernel
inline bool filter_rows_blocked(int64_t nq, int k) { return k <= 128 && nq >= 2 * kFilterRowsQB; }

// splits of the list per query (group): enough (group, split) units to cover the chip, none below kFilterSplitRows entries, the
// partial lists within their budget
inline int filter_rows_splits(int64_t nq, int k, int64_t n_allowed) {
    const int64_t groups = filter_rows_blocked(nq, k) ? (nq + kFilterRowsQB - 1) / kFilterRowsQB : nq;
    int64_t S = (4096 + groups - 1) / groups;
    const int64_t by_rows = n_allowed / kFilterSplitRows;
    if (S > by_rows) S = by_rows;
    if (S > kFilterMaxSplits) S = kFilterMaxSplits;
    const int64_t cap = kFilterPartialBytes / (nq * (int64_t)k * 16);
    if (S > cap) S = cap;
    return S < 1 ? 1 : (int)S;
}
// entries per split: whole 64-entry wave iterations
inline int64_t filter_rows_per_split(int64_t n_allowed, int S) {
    const int64_t per = ((n_allowed + S - 1) / S + 63) / 64 * 64;
    return per < 64 ? 64 : per;
}

// device bytes an installed filter adds to bytes_resident: words + count, the masked bias copies the handle has the originals of,
// and the list with its segment offsets when it is kept (every buffer is sized exactly)
inline int64_t filter_bytes(int64_t Npad, bool has_bias, bool has_bias8, bool keeps_list, int64_t n_allowed) {
    int64_t b = filter_words(Npad) * 4 + 8;
    if (has_bias) b += Npad * 4;
    if (has_bias8) b += 2 * Npad * 4;
    if (keeps_list) b += (n_allowed > 4 ? n_allowed : 4) * 4 + filter_segments(Npad) * 4;
    return b;
}

}  // namespace vdb

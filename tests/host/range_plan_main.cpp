// The sizes of a range search (csrc/range_plan.hpp) as a host program: tests/test_range_plan_host.py compares its output with a
// Python restatement.  Input: one case per line, "nq N bitmap_mb".  Output: one JSON object per case.
#include <stdio.h>

#include <cinttypes>

#include "../../vectordb-retrieval_amd/csrc/range_plan.hpp"

int main() {
    long long nq, N;
    int mb;
    while (scanf("%lld %lld %d", &nq, &N, &mb) == 3) {
        const int64_t W = vdb::range_words(N), S = vdb::range_segments(N);
        const int64_t slab = vdb::range_slab_queries(nq, N, mb), slabs = vdb::range_slabs(nq, N, mb);
        // the masks of the word that holds row N - 1, the one behind it and the last word of the row
        const int64_t wl = N > 0 ? (N - 1) / vdb::kRangeWordBits : 0;
        printf("{\"words\": %" PRId64 ", \"segments\": %" PRId64 ", \"slab\": %" PRId64 ", \"slabs\": %" PRId64
               ", \"budget\": %" PRId64 ", \"mask_first\": %u, \"mask_tail\": %u, \"mask_next\": %u, \"mask_last\": %u}\n",
               W, S, slab, slabs, vdb::range_budget_bytes(mb), vdb::range_word_mask(0, N), vdb::range_word_mask(wl, N),
               vdb::range_word_mask(wl + 1, N), vdb::range_word_mask(W - 1, N));
    }
    return 0;
}

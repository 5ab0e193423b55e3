// ivf_filter_plan.hpp -- the sizing and routing rules of a filtered search on an IVF-Flat index (ivf_filter.hpp, ivf_filter.inc;
// DESIGN 4.15): words of the list-order allow bitmap, bytes an installed filter holds, and when the exact list scan answers a
// batch instead of the list-major MFMA scan.  No HIP: tests/host/ivf_filter_plan_main.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

#include "ivf_plan.hpp"

namespace vdb {

// The handle keeps the bitmap in LIST order (bit r % 32 of word r / 32 admits list-order row r): whole 64-row wave units, two
// words each, so the install's ballots store without a tail case.
constexpr int kIvfFilterUnitRows = 64;
inline int64_t ivf_filter_words(int64_t N) { return (N + kIvfFilterUnitRows - 1) / kIvfFilterUnitRows * 2; }

// device bytes an installed filter adds to bytes_resident: the list-order words, the admitted count (8 bytes) and the masked
// copies of the panel space's accumulator inits the handle has the originals of -- bias_f over `panel_rows` = pspans * span_rows
// slots, both windows of bias8_f on a byte-valued corpus.  Every buffer is sized exactly.
inline int64_t ivf_filter_bytes(int64_t N, int64_t panel_rows, bool has_bias, bool has_bias8) {
    int64_t b = ivf_filter_words(N) * 4 + 8;
    if (has_bias) b += panel_rows * 4;
    if (has_bias8) b += 2 * panel_rows * 4;
    return b;
}

// Routing.  ivf_geometry declines a batch whose probed lists give fewer than 4 k bins per query (est_entries): the select needs
// that many to find k of them.  Under a filter only a bin with an admitted row is live, and there are at most as many live bins
// as admitted rows probed -- nprobe * n_allowed / nlist for admitted rows spread like the rows themselves.  The same test on the
// smaller of the two: below it most queries would be flagged and pay the scan AND the fallback.  A filter that admits every row
// routes as vdb_ivf_search does (same bins, same select).  Correctness never depends on the rule: a query with too few live bins
// is flagged by the select and answered by the exact fallback.
inline bool ivf_filter_declines(const IvfIndexShape &s, const IvfGeom &g, int k, int nprobe, int64_t n_allowed) {
    if (n_allowed >= s.N) return false;
    const double est_entries = (double)nprobe * g.bins_per_span * ((double)s.pspans / (double)s.nlist);
    const double live = (double)nprobe * (double)n_allowed / (double)s.nlist;
    return (est_entries < live ? est_entries : live) < 4.0 * k;
}

// ivf_geometry of a filtered batch.  force_path keeps its meaning: 1 / 3 decline inside ivf_geometry; 2 asks for the list-major
// scan wherever ivf_geometry itself admits the batch, so the filter rule stands aside.
inline IvfGeom ivf_filter_geometry(const IvfIndexShape &s, const Options &opt, int64_t nb, int k, int nprobe, int64_t n_allowed) {
    const IvfGeom g = ivf_geometry(s, opt, nb, k, nprobe);
    if (g.ok && opt.force_path != 2 && ivf_filter_declines(s, g, k, nprobe, n_allowed)) return IvfGeom{};
    return g;
}

}  // namespace vdb

// ivf_range_plan.hpp -- the rules of a range search on an IVF-Flat index (ivf_range.hpp, ivf_range.inc): query slabs and
// their bitmap bytes, the route of a slab and the LDS of the mark kernel.  No HIP: tests/host/ivf_range_plan_main.cpp compiles it
// with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "range_plan.hpp"

namespace vdb {

constexpr int64_t kIvfRangeBatch = 16384;     // queries of one IVF batch (ivf_search_device_impl): a slab is a batch of its own

// queries per slab: what the bitmap budget holds (range_slab_queries), at most one IVF batch
inline int64_t ivf_range_slab_queries(int64_t nq, int64_t N, int bitmap_mb) {
    const int64_t s = range_slab_queries(nq, N, bitmap_mb);
    return s < kIvfRangeBatch ? s : kIvfRangeBatch;
}
inline int64_t ivf_range_slabs(int64_t nq, int64_t N, int bitmap_mb) {
    const int64_t s = ivf_range_slab_queries(nq, N, bitmap_mb);
    return (nq + s - 1) / s;
}
// bytes of the candidate bitmap of one slab: [query][list-order row / 32], the row pitch of the flat range search
inline int64_t ivf_range_bitmap_bytes(int64_t nq, int64_t N, int bitmap_mb) {
    return ivf_range_slab_queries(nq, N, bitmap_mb) * range_words(N) * 4;
}

// the route of a slab: 1 = list-major (fp16 list scan, then the marks from the kept bin minima), 0 = exact (every probed row is a
// candidate, no scan).  geometry_ok: ivf_geometry(.., k = 1, ..).ok, which already declines under force_path 1 / 3; force_path 2
// cannot make a declined batch list-major (there are no panels to scan, or no plan that fits)
inline int ivf_range_route(bool geometry_ok, int force_path) {
    if (force_path == 1 || force_path == 3) return 0;
    return geometry_ok ? 1 : 0;
}

// 32-bit LDS words per wave of ivf_range_mark_kernel: p_off[probe_cap + 32] | p_base lo / hi [2 probe_cap] | p_list[probe_cap] (+ 32)
inline int ivf_range_probe_cap(int nprobe) { return (nprobe + 63) / 64 * 64; }
inline size_t ivf_range_mark_lds_words(int nprobe) { return 4 * (size_t)ivf_range_probe_cap(nprobe) + 64; }

}  // namespace vdb

// ivf_i8k_plan.hpp -- the int8 K-loop LIST scan (ivf_kloop_i8.hpp; option "ivf_i8_kloop"; IVF-Flat over a byte-valued corpus of
// D > 128): which handles get the int8 copy of the panel space, which batches the kernel serves, and its launch.  Plain host C++
// beside ivf_plan.hpp (no HIP header, no handle): tests/host/ivf_i8k_plan_main.cpp prints what the rules give.  The key format of
// the handle is the flat scan's: i8k_key_rule(D padded to 64, corpus window, metric), i8k_plan.hpp.
#pragma once
#include "i8k_plan.hpp"
#include "ivf_plan.hpp"

namespace vdb {

// ---- the build rule: an add gives the handle the copy (int8 p16 panels over the list-padded panel space, accumulator inits of both
// query windows, row statistics, list-order int8 rows with a pitch of D padded to 64) ------------------------------------------------
// codec: 0 = IVF-Flat (SQ8, IVF-PQ and IVF-I8 lists are out of scope); tile16: D > 128, the p16 panel space; byte_valued: the flags
// of corpus_stats_kernel (every value a finite integer of the u8 or of the s8 window)
inline bool ivf_i8k_build(int opt_ivf_i8_kloop, int codec, bool tile16, bool byte_valued, int dim) {
    return opt_ivf_i8_kloop != 0 && codec == 0 && tile16 && byte_valued && dim <= kI8kMaxDim;
}

// ---- the launch rule: the handle has the copy | option "panel_dtype" = 0 | not the square workgroup tile (option "ivf_tile" = 2 has
// no int8 form) | an unfiltered vdb_ivf_search / _device / _partial_device batch (a filtered call reads masked accumulator inits
// with the D <= 128 key constants; a range call never comes here) | on the list-major path.  Everything else runs as without the
// option, on the fp16 K-loop scan or the exact list scan.
inline bool ivf_i8k_serves(bool has_copy, int panel_dtype, int ivf_tile, bool filtered, bool list_major) {
    return has_copy && panel_dtype == 0 && ivf_tile != 2 && !filtered && list_major;
}

// ---- the launch: the fp16 K-loop plan's grid and row parts (plan_ivf_kloop), ivf_kloop_i8_scan_kernel<TPS, BS, GROUP> -----------------
// (only for batches the launch rule admits: the square tile never gets here)
inline IvfLaunch plan_ivf_kloop_i8(const IvfIndexShape &s, const Options &opt, const IvfGeom &g, int kgroup) {
    const IvfLaunch f = plan_ivf_kloop(s, opt, g, kgroup);
    const IvfParts parts{f.part_spans, f.grid_x, f.grid_y};
    return ivf_launch_of(ScanFamily::ivf_kloop_i8, parts, 512, {f.key.t[0], kI8kBarrierSteps, f.key.t[2]});
}

// every instantiation, once: 64-row bins with single rows, pairs and quads as candidate groups | 256-row bins with quads
#define VDB_KERNELS_IVF_KLOOP_I8(X) X(16, 2, 1) X(16, 2, 2) X(16, 2, 4) X(64, 2, 4)
constexpr ScanKey kKeysIvfKloopI8[] = {VDB_KERNELS_IVF_KLOOP_I8(VDB_SCAN_KEY)};
static_assert(kI8kBarrierSteps == 2, "the instantiations above are written for a barrier every 2 K-steps");

}  // namespace vdb

// ivf_sq8d_plan.hpp -- the direct list scan of an IVF-SQ8 index (ivf_sq8_scan.hpp; option "ivf_sq8_direct"): which batches it serves,
// the 16-byte chunks a row of codes is read in, its launch and its LDS bytes.  Plain host C++ beside ivf_plan.hpp, so
// tests/host/ivf_sq8d_plan_main.cpp prints what the rules give.
#pragma once
#include "ivf_plan.hpp"

namespace vdb {

#if defined(__HIPCC__)
#define VDB_SQ8D_HD __host__ __device__
#else
#define VDB_SQ8D_HD
#endif

// The scan serves a batch of the list-major path (ivf_geometry ok, D <= 128: never the K-loop geometry) of an SQ8 handle with the
// option set, unfiltered.  A row of codes is read in whole 16-byte chunks that never leave the row: D4 >= 16.
inline bool ivf_sq8d_serves(int opt_direct, int codec, bool geom_ok, bool kloop, int D4, bool filtered) {
    return opt_direct != 0 && codec == 1 && geom_ok && !kloop && D4 >= 16 && !filtered;
}

// Chunk c of a row (c < KSTEPS: 4 or 8) is the 16 bytes at chunk_base: dims 16c .. 16c + 15 where the row has them; the chunk that
// would cross the row's end (D4 is a multiple of 4, not of 16) is the row's LAST 16 bytes instead, and a chunk behind the end is the
// row's first.  The query operand of a chunk names the same dims and is zero for those another chunk already covers (chunk_dim).
VDB_SQ8D_HD inline int ivf_sq8d_chunk_base(int c, int D4) {
    const int b = 16 * c;
    return b + 16 <= D4 ? b : (b < D4 ? D4 - 16 : 0);
}
// the dimension element j of chunk c multiplies, or -1: none (its operand is zero)
VDB_SQ8D_HD inline int ivf_sq8d_chunk_dim(int c, int j, int D, int D4) {
    const int d = ivf_sq8d_chunk_base(c, D4) + j;
    return (16 * c < D4 && d >= 16 * c && d < D) ? d : -1;
}

constexpr int kSq8dStageTiles = 2;      // 32-row tiles per LDS stage (the items-mode ST)
// static LDS of ivf_sq8_scan_kernel<KSTEPS, ..>: two stages of ST tiles x 32 rows x 16 KSTEPS code bytes + their 32 bias floats per tile
constexpr size_t ivf_sq8d_lds_bytes(int ksteps) { return 2 * ((size_t)kSq8dStageTiles * 32 * 16 * ksteps + kSq8dStageTiles * 32 * 4); }

// the launch: the fp16 items-mode scan's grid, row parts, waves and bins (plan_ivf_f16), so the bins it writes are the ones the select
// and the tail expect.  ivf_sq8_scan_kernel<KSTEPS, NWAVES, BT>
inline IvfLaunch plan_ivf_sq8d(const IvfIndexShape &s, const Options &opt, const IvfGeom &g) {
    const IvfLaunch f = plan_ivf_f16(s, opt, g);
    return ivf_launch_of(ScanFamily::ivf_sq8d, IvfParts{f.part_spans, f.grid_x, f.grid_y}, f.block, {f.key.t[0], f.key.t[1], f.key.t[4]});
}

#define VDB_KERNELS_IVF_SQ8D_K(X, K) X(K, 2, 4) X(K, 2, 8) X(K, 4, 4) X(K, 4, 8) X(K, 8, 4) X(K, 8, 8)
#define VDB_KERNELS_IVF_SQ8D(X) VDB_KERNELS_IVF_SQ8D_K(X, 4) VDB_KERNELS_IVF_SQ8D_K(X, 8)
constexpr ScanKey kKeysIvfSq8d[] = {VDB_KERNELS_IVF_SQ8D(VDB_SCAN_KEY)};

}  // namespace vdb

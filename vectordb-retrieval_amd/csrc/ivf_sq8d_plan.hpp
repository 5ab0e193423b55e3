// ivf_sq8d_plan.hpp -- the direct list scan of an IVF-SQ8 index (ivf_sq8_scan.hpp; option "ivf_sq8_direct"): which batches it serves,
// the 16-byte chunks a row of codes is read in, its launch and its LDS bytes.  Plain host C++ beside ivf_plan.hpp, so
// tests/host/ivf_sq8d_plan_main.cpp prints what the rules give.  Below them the same for its K-loop form at D > 128 (ivf_sq8_kloop.hpp;
// option "ivf_sq8_kloop").
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

// ---- D > 128: the K-loop scan of the codes (ivf_sq8_kloop.hpp; option "ivf_sq8_kloop", takes effect at an add) -------------------------
constexpr int kSq8kMaxDim = 4096;       // the K-loop's limit (ivf_build_panel_space)
// does an add build the bookkeeping of the route (span tables, accumulator inits, maxnorm2 -- no panels)?
inline bool ivf_sq8k_builds(int opt_kloop, int codec, int ksteps, int dim) {
    return opt_kloop != 0 && codec == 1 && ksteps > kMaxKSteps && dim <= kSq8kMaxDim;
}
// The scan serves a batch of the list-major path in the K-loop geometry (`kloop_geom` = ivf_geometry ok && kloop) of an SQ8 handle whose
// last add built that bookkeeping, with the option still set, unfiltered.  There is no fp16 scan behind it: a batch it does not serve
// takes the exact list scan.
inline bool ivf_sq8k_serves(int opt_kloop, int codec, bool built, bool kloop_geom, bool filtered) {
    return opt_kloop != 0 && codec == 1 && built && kloop_geom && !filtered;
}
// the square workgroup tile (option "ivf_tile" = 2) is not built for this route: an SQ8 handle plans as if the option were 0
inline Options ivf_sq8k_options(Options opt) {
    opt.ivf_tile = 0;
    return opt;
}

// A row of codes is read in the 16-byte chunks of the D <= 128 scan: chunk c = 4 kk + kq of K-step kk and lane quarter kq, under the
// same rule at the row's end (ivf_sq8d_chunk_base / _chunk_dim: D4 is a multiple of 4, not of 64 -- the crossing chunk is the row's
// last 16 bytes, with a zero operand for the dimensions the chunk before it covered; a chunk behind the end has a zero operand).
// Bytes 0..7 of a chunk feed the first MFMA of the K-step (ks = 0), bytes 8..15 the second, so element p = 64 kk + 32 ks + 8 kq + j of
// an operand row multiplies element 8 ks + j of chunk 4 kk + kq.  Returns that dimension, or -1: none (the operand is zero)
VDB_SQ8D_HD inline int ivf_sq8k_operand_dim(int p, int D, int D4) {
    const int kk = p >> 6, ks = (p >> 5) & 1, kq = (p >> 3) & 3, j = p & 7;
    return ivf_sq8d_chunk_dim(4 * kk + kq, 8 * ks + j, D, D4);
}

constexpr int kSq8kStageTiles = 8;      // 16-row tiles per LDS stage: one pass of the scan, one per wave
// a stage: 8 tiles x 16 rows x 64 code bytes of one K-step (the fp16 K-loop scan's is twice that)
constexpr size_t ivf_sq8k_stage_bytes() { return (size_t)kSq8kStageTiles * 16 * 64; }
// static LDS of ivf_sq8_kloop_scan_kernel<TPS, BS, GROUP>: the ring of 2 BS stages + the running minima of 8 waves x 4 column blocks
constexpr size_t ivf_sq8k_lds_bytes(int bs) { return 2 * (size_t)bs * ivf_sq8k_stage_bytes() + (size_t)8 * kIvfKloopMinima * 4 * 64 * 4; }

// the launch: grid, row parts and candidate groups of the fp16 K-loop scan (plan_ivf_kloop) with RH = 1, so the bins are the ones the
// select and the tail expect.  ivf_sq8_kloop_scan_kernel<TPS, BS, GROUP>
inline IvfLaunch plan_ivf_sq8k(const IvfIndexShape &s, const Options &opt, const IvfGeom &g, int kgroup) {
    const IvfLaunch f = plan_ivf_kloop(s, ivf_sq8k_options(opt), g, kgroup);
    return ivf_launch_of(ScanFamily::ivf_sq8k, IvfParts{f.part_spans, f.grid_x, f.grid_y}, f.block, {f.key.t[0], f.key.t[1], f.key.t[2]});
}

#define VDB_KERNELS_IVF_SQ8K(X) X(16, 2, 1) X(16, 2, 2) X(16, 2, 4) X(64, 2, 4)
constexpr ScanKey kKeysIvfSq8k[] = {VDB_KERNELS_IVF_SQ8K(VDB_SCAN_KEY)};

}  // namespace vdb

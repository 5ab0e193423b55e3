// ivf_pq_kloop_plan.hpp -- the K-loop list scan of an IVF-PQ index straight from the product codes (ivf_pq_kloop.hpp; option
// "ivf_pq_kloop", D > 128): which adds build its bookkeeping, which batches it serves, the padded operand space, the LDS a workgroup
// holds and its launch.  Plain host C++ beside ivf_sq8d_plan.hpp, so tests/host/ivf_pq_kloop_plan_main.cpp prints what the rules give.
#pragma once
#include "ivf_plan.hpp"

#if defined(__HIPCC__)
#define VDB_PQK_HD __host__ __device__
#else
#define VDB_PQK_HD
#endif

namespace vdb {

// ---- the operand space --------------------------------------------------------------------------------------------------------------
// dsub = D / M need not be a multiple of the 8-element MFMA fragment (12 and 6 at 768 / 384 dims under PQ64), and the K order of an
// MFMA is the kernel's to choose: every sub-space is padded to P = 8 ceil(dsub / 8) operand dimensions, so that each 8-element A
// fragment is one aligned 16-byte piece of one entry of the fp16 table T[m][256][P].  Operand dimension m P + j is dimension
// m dsub + j for j < dsub and carries zero otherwise; Kp = M P, scanned in nk = ceil(Kp / 64) K-steps.  Cost: Kp / D of the MFMA work.
constexpr int kPqkMaxDim = 4096;        // the K-loop's limit on D (ivf_build_panel_space) and on Kp
constexpr int kPqkMaxM = 256;           // code bytes of a row the kernel stages (two passes of 128 rows x 256 bytes in LDS)
VDB_PQK_HD inline int ivf_pqk_p(int dsub) { return 8 * ((dsub + 7) / 8); }
VDB_PQK_HD inline int ivf_pqk_kp(int M, int dsub) { return M * ivf_pqk_p(dsub); }
VDB_PQK_HD inline int ivf_pqk_nk(int M, int dsub) { return (ivf_pqk_kp(M, dsub) + 63) / 64; }
// the dimension behind operand position p of [0, 64 nk), or -1: none (sub-space padding, or the tail of the last K-step behind Kp)
VDB_PQK_HD inline int ivf_pqk_operand_dim(int p, int M, int dsub) {
    const int P = ivf_pqk_p(dsub), m = p / P, j = p - m * P;
    return (m < M && j < dsub) ? m * dsub + j : -1;
}

// does an add build the bookkeeping of the route (span tables, accumulator inits, the fp16 table, the constants of the bound)?
inline bool ivf_pqk_builds(int opt_kloop, int codec, int ksteps, int dim, int M, int dsub) {
    return opt_kloop != 0 && codec == 2 && ksteps > kMaxKSteps && dim <= kPqkMaxDim && M >= 1 && M <= kPqkMaxM && dsub >= 1 &&
           ivf_pqk_kp(M, dsub) <= kPqkMaxDim;
}
// The scan serves a batch of the list-major path in the K-loop geometry (`kloop_geom` = ivf_geometry ok && kloop) of an IVF-PQ handle
// whose last add built that bookkeeping, with the option still set, unfiltered.  There is no fp16 scan behind it: a batch it does not
// serve takes the exact list scan (or, admitted by "ivfpq_adc_max_batch", the lookup-table scan: such a batch has no geometry).
inline bool ivf_pqk_serves(int opt_kloop, int codec, bool built, bool kloop_geom, bool filtered) {
    return opt_kloop != 0 && codec == 2 && built && kloop_geom && !filtered;
}
// the square workgroup tile (option "ivf_tile" = 2) is not built for this route: such a handle plans as if the option were 0
inline Options ivf_pqk_options(Options opt) {
    opt.ivf_tile = 0;
    return opt;
}

// ---- LDS of ivf_pq_kloop_scan_kernel<TPS, BS, GROUP, CP> ------------------------------------------------------------------------------
// A stage is what the fp16 K-loop scan's is: 8 tiles x 16 rows x 64 operand dims of fp16 = 16 KiB, in a ring of 2 BS stages (one
// barrier per BS K-steps).  Next to it the running minima of 8 waves x 4 column blocks (40 KiB) and the codes of two passes (the one
// scanned and the one whose gathers are already issued): 2 x 128 rows x CP bytes, CP = the row pitch class of M.  One workgroup of 512
// lanes and 256 registers runs per CU (the occupancy of ivf_kloop_scan_kernel), so the budget is the CU's 160 KiB:
//   M <=  64: CP =  64, BS = 2:  64 + 40 + 16 = 120 KiB
//   M <= 256: CP = 256, BS = 1:  32 + 40 + 64 = 136 KiB   (the deeper ring would need 168)
constexpr size_t kPqkLdsBudget = 160 * 1024;
constexpr int ivf_pqk_code_pitch(int M) { return M <= 64 ? 64 : 256; }
constexpr int ivf_pqk_ring_bs(int M) { return M <= 64 ? 2 : 1; }
constexpr size_t ivf_pqk_stage_bytes() { return (size_t)8 * 16 * 64 * 2; }
constexpr size_t ivf_pqk_lds_bytes(int bs, int cp) {
    return 2 * (size_t)bs * ivf_pqk_stage_bytes() + (size_t)8 * kIvfKloopMinima * 4 * 64 * 4 + (size_t)2 * 128 * cp;
}

// the launch: grid, row parts and candidate groups of the fp16 K-loop scan (plan_ivf_kloop) with the square tile off, so the bins are
// the ones the select and the tail expect; ring depth and code pitch from M
inline IvfLaunch plan_ivf_pqk(const IvfIndexShape &s, const Options &opt, const IvfGeom &g, int kgroup, int M) {
    const IvfLaunch f = plan_ivf_kloop(s, ivf_pqk_options(opt), g, kgroup);
    return ivf_launch_of(ScanFamily::ivf_pqk, IvfParts{f.part_spans, f.grid_x, f.grid_y}, f.block,
                         {f.key.t[0], ivf_pqk_ring_bs(M), f.key.t[2], ivf_pqk_code_pitch(M)});
}

#define VDB_KERNELS_IVF_PQK_C(X, BS, CP) X(16, BS, 1, CP) X(16, BS, 2, CP) X(16, BS, 4, CP) X(64, BS, 4, CP)
#define VDB_KERNELS_IVF_PQK(X) VDB_KERNELS_IVF_PQK_C(X, 2, 64) VDB_KERNELS_IVF_PQK_C(X, 1, 256)
constexpr ScanKey kKeysIvfPqk[] = {VDB_KERNELS_IVF_PQK(VDB_SCAN_KEY)};

}  // namespace vdb

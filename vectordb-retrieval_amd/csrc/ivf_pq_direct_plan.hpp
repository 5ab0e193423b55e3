// ivf_pq_direct_plan.hpp -- the direct list scan of an IVF-PQ index at D <= 128 (ivf_pq_scan.hpp; option "ivf_pq_direct"): which batches
// it serves, the dynamic LDS a workgroup holds by (D, M, KSTEPS), its launch and its kernel list.  Plain host C++ beside
// ivf_sq8d_plan.hpp, so tests/host/ivf_pqd_plan_main.cpp prints what the rules give.
#pragma once
#include "ivf_plan.hpp"

#if defined(__HIPCC__)
#define VDB_PQD_HD __host__ __device__
#else
#define VDB_PQD_HD
#endif

namespace vdb {

// The scan serves a batch of the list-major path in its D <= 128 form (ivf_geometry ok, never the K-loop geometry) of an IVF-PQ handle
// with the option set, unfiltered.  (A batch "ivfpq_adc_max_batch" admits has no geometry: the lookup-table scan keeps it.)
inline bool ivf_pqd_serves(int opt_direct, int codec, bool geom_ok, bool kloop, bool filtered) {
    return opt_direct != 0 && codec == 2 && geom_ok && !kloop && !filtered;
}

// ---- LDS of ivf_pq_scan_kernel<KSTEPS, NWAVES, BT>, all of it dynamic -----------------------------------------------------------------
//   table   T[m][256][dsub] fp16 = 512 D bytes, copied in whole 1-KiB pieces (the device buffer is zero padded to them)
//   stages  two buffers of ST = 2 tiles x KSTEPS k-steps x 1 KiB: the decoded A fragments, in the fp16 panels' layout
//   codes   two buffers of 64 rows (two tiles x two runs of 16 list-order rows) x CP bytes; CP = M rounded up to an ODD number of
//           dwords, so the 32 rows a decode reads one code of lie in 32 banks
//   bias    two buffers of 64 floats
constexpr int kPqdStageTiles = 2;
VDB_PQD_HD constexpr int ivf_pqd_code_pitch(int M) { return (((M + 3) / 4) | 1) * 4; }
VDB_PQD_HD constexpr size_t ivf_pqd_table_bytes(int D) { return ((size_t)512 * D + 1023) / 1024 * 1024; }
VDB_PQD_HD constexpr size_t ivf_pqd_stage_bytes(int ksteps) { return (size_t)kPqdStageTiles * ksteps * 1024; }
VDB_PQD_HD constexpr size_t ivf_pqd_codes_bytes(int M) { return (size_t)kPqdStageTiles * 32 * ivf_pqd_code_pitch(M); }
VDB_PQD_HD constexpr size_t ivf_pqd_lds_bytes(int D, int M, int ksteps) {
    return ivf_pqd_table_bytes(D) + 2 * ivf_pqd_stage_bytes(ksteps) + 2 * ivf_pqd_codes_bytes(M) + 2 * (size_t)kPqdStageTiles * 32 * 4;
}
constexpr size_t kPqdLdsBudget = 160 * 1024;     // a CU's LDS; above 64 KiB a launch opts in (hipFuncAttributeMaxDynamicSharedMemorySize)
// workgroups of one CU the LDS leaves room for (D = 128 / PQ64: 105 KiB -> 1; D = 64 / PQ16: 51 KiB -> 3)
inline int ivf_pqd_wgs_per_cu(int D, int M, int ksteps) { return (int)(kPqdLdsBudget / ivf_pqd_lds_bytes(D, M, ksteps)); }

// the launch: the fp16 items-mode scan's grid, row parts, waves and bins (plan_ivf_f16), so the bins it writes are the ones the select
// and the tail expect.  ivf_pq_scan_kernel<KSTEPS, NWAVES, BT>
inline IvfLaunch plan_ivf_pqd(const IvfIndexShape &s, const Options &opt, const IvfGeom &g) {
    const IvfLaunch f = plan_ivf_f16(s, opt, g);
    return ivf_launch_of(ScanFamily::ivf_pqd, IvfParts{f.part_spans, f.grid_x, f.grid_y}, f.block, {f.key.t[0], f.key.t[1], f.key.t[4]});
}

#define VDB_KERNELS_IVF_PQD_K(X, K) X(K, 2, 4) X(K, 2, 8) X(K, 4, 4) X(K, 4, 8) X(K, 8, 4) X(K, 8, 8)
#define VDB_KERNELS_IVF_PQD(X) VDB_KERNELS_IVF_PQD_K(X, 4) VDB_KERNELS_IVF_PQD_K(X, 8)
constexpr ScanKey kKeysIvfPqd[] = {VDB_KERNELS_IVF_PQD(VDB_SCAN_KEY)};

}  // namespace vdb

// pq_kloop_plan.hpp -- the K-loop scan of a flat PQ index straight from the product codes (pq_kloop.hpp; option "pq_kloop", D > 128):
// which batches it serves, the LDS a workgroup holds and its launch.  The padded operand space is the one of ivf_pq_kloop_plan.hpp
// (ivf_pqk_p / _kp / _nk / _operand_dim).  Plain host C++ beside scan_plan.hpp, so tests/host/pq_kloop_plan_main.cpp prints what the
// rules give.
#pragma once
#include "ivf_pq_kloop_plan.hpp"

namespace vdb {

// The scan serves an unfiltered k-NN batch of a flat PQ handle with D > 128 that the panel pass + K-loop scan would serve today
// (`scan_path`: search_batch chose the MFMA scan; `direct_rows` == 0: on the standard 256-row-bin geometry), after the ADC scan had
// its pick (`adc`: "pq_adc_max_batch" admitted the batch), when the codes of a row and the operand space fit what the kernel stages.
// Everything else takes the panel pass as before.
inline bool pq_kloop_serves(int opt_kloop, bool pq, int ksteps, int M, int dsub, bool scan_path, int direct_rows, bool adc, bool filtered) {
    return opt_kloop != 0 && pq && ksteps > kMaxKSteps && scan_path && direct_rows == 0 && !adc && !filtered && M >= 1 && M <= kPqkMaxM &&
           dsub >= 1 && ivf_pqk_kp(M, dsub) <= kPqkMaxDim;
}

// ---- LDS of pq_kloop_scan_kernel<BS, NARROW, CP> -------------------------------------------------------------------------------------
// A stage is the flat K-loop scan's: 8 tiles x 16 rows x 64 operand dims of fp16 = 16 KiB, in a ring of 2 BS stages (one barrier per
// BS K-steps).  Next to it only the codes of two passes (the one scanned and the one whose gathers are already issued), 2 x 128 rows x
// CP bytes: the running minima of the flat scan live in registers, so unlike the list scan there is no block of minima in LDS and the
// deep ring fits both pitch classes:
//   M <=  64: CP =  64, BS = 2:  64 + 16 =  80 KiB   half a CU's LDS: the LDS never allows fewer workgroups per CU than the registers
//   M <= 256: CP = 256, BS = 2:  64 + 64 = 128 KiB   one workgroup per CU
// (scan16_kloop_kernel holds 64 KiB at BS = 2; both are __launch_bounds__(512, 2) kernels of 8 waves.)
constexpr size_t kPqKloopLdsCu = 160 * 1024;
constexpr int pq_kloop_code_pitch(int M) { return M <= 64 ? 64 : 256; }
constexpr int pq_kloop_ring_bs(int) { return 2; }
constexpr size_t pq_kloop_lds_bytes(int bs, int cp) { return 2 * (size_t)bs * ivf_pqk_stage_bytes() + (size_t)2 * 128 * cp; }
constexpr int pq_kloop_wgs_per_cu_lds(int M) { return (int)(kPqKloopLdsCu / pq_kloop_lds_bytes(pq_kloop_ring_bs(M), pq_kloop_code_pitch(M))); }

// NARROW = 1 under the rule of the flat K-loop scan (plan_f16): a batch below 64 queries with option "small_batch" on -- one wave per
// workgroup holds queries and does MFMAs and select work only for its column blocks that do.  (The LDS-resident query block of
// scan16_kloop_kernel<3, 8, 2> is not built for this route: 1 ... 16 queries take NARROW = 1 too.)
inline int pq_kloop_narrow(const Options &opt, int64_t nq) { return nq > 0 && nq < 64 && opt.small_batch ? 1 : 0; }

// the launch: grid, query tiles and block order of the flat K-loop scan (plan_f16 on the standard geometry); ring depth and code
// pitch from M
inline ScanLaunch plan_pq_kloop(const ScanIndexShape &s, const Options &opt, int nchunks, int64_t Qpad, int64_t nq, int M) {
    const ScanLaunch f = plan_f16(s, opt, nchunks, Qpad, nq, 0, 8);
    ScanLaunch p = scan_launch(ScanFamily::pq_kloop, f.nqtiles, f.grid, f.block, {pq_kloop_ring_bs(M), pq_kloop_narrow(opt, nq), pq_kloop_code_pitch(M)});
    p.qgroup = f.qgroup;
    return p;
}

#define VDB_KERNELS_PQ_KLOOP(X) X(2, 0, 64) X(2, 1, 64) X(2, 0, 256) X(2, 1, 256)
constexpr ScanKey kKeysPqKloop[] = {VDB_KERNELS_PQ_KLOOP(VDB_SCAN_KEY)};

}  // namespace vdb

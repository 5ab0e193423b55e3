// Diagnostic build of the int8 x16 batch scan with IN-KERNEL STAMPS (round 9): where a stage of scan_i8x16_batch_loop spends the
// cycles that are not MFMA stream.  The production header marks four points with VDB_X16_STAMP (empty in the library); here they read
// s_memtime into per-wave sums of their own and the kernel is launched alone, over synthetic byte data in the bench shape (sift1m:
// 1M rows x 128 dims, 10 000 queries -> 128 chunks of 15 / 16 spans, ten 1024-query tiles, 1 280 workgroups).  Reported per wave
// (medians over the computing waves): cycles from the last MFMA of a stage to the first MFMA of the next (the hand-over, the barrier
// wait included), cycles inside flush_bin, and both as a share of the loop.  A stamp costs a scalar memory wait; the stamped kernel
// is not the benchmarked one.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I ../../vectordb-retrieval_amd/csrc stamp_i8x16.hip -o stamp_i8x16
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

__device__ unsigned long long *g_x16_stamps;      // [wave][6]: hand-over cycles, hand-overs, flush cycles, flushes, loop cycles, stages
__device__ __forceinline__ unsigned long long x16_clock() {
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define VDB_X16_STAMP_BEGIN \
    unsigned long long sx_t0 = 0, sx_f0 = 0, sx_hand = 0, sx_flush = 0, sx_nh = 0, sx_nf = 0; \
    const unsigned long long sx_start = x16_clock();
#define VDB_X16_STAMP(point)                                         \
    do {                                                             \
        const unsigned long long sx_now = x16_clock();               \
        if ((point) == 0) sx_t0 = sx_now;                            \
        else if ((point) == 1) { if (sx_t0) { sx_hand += sx_now - sx_t0; ++sx_nh; } } \
        else if ((point) == 2) sx_f0 = sx_now;                       \
        else { sx_flush += sx_now - sx_f0; ++sx_nf; }                \
    } while (0)
#define VDB_X16_STAMP_END                                            \
    if ((threadIdx.x & 63) == 0) {                                   \
        unsigned long long *sx_o = g_x16_stamps + ((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 6; \
        sx_o[0] = sx_hand; sx_o[1] = sx_nh; sx_o[2] = sx_flush; sx_o[3] = sx_nf; \
        sx_o[4] = x16_clock() - sx_start; sx_o[5] = (unsigned long long)nstages; \
    }

#include "scan_i8x16.hpp"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

using namespace vdb;

template <class T>
static T *dev(size_t n, const std::vector<T> *init = nullptr) {
    T *p;
    CK(hipMalloc(&p, n * sizeof(T)));
    if (init) CK(hipMemcpy(p, init->data(), n * sizeof(T), hipMemcpyHostToDevice));
    else CK(hipMemset(p, 0, n * sizeof(T)));
    return p;
}

int main() {
    const int64_t N = 1000000, nq = 10000, Qpad = 10240, nspans = (N + kSpanRows - 1) / kSpanRows, Npad = nspans * kSpanRows;
    const int nchunks = 128, nqtiles = (int)(Qpad / 1024), KS2 = 2;
    const unsigned grid = 8u * ((nchunks + 7) / 8) * nqtiles;
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    std::vector<int4v> panels((size_t)nspans * kTilesPerSpan * 2 * KS2 * 64), qpanels((size_t)(Qpad / 16) * KS2 * 64);
    for (auto &v : panels) for (int j = 0; j < 4; ++j) v[j] = (int)(rnd() & 0x3f3f3f3f);        // bytes 0 .. 63
    for (auto &v : qpanels) for (int j = 0; j < 4; ++j) v[j] = (int)(rnd() & 0x3f3f3f3f);
    std::vector<int32_t> bias((size_t)2 * Npad);
    for (auto &v : bias) v = (int32_t)(1 << 20) + (int32_t)(rnd() & 0xffff);
    QueryBatchInfo info{};
    info.i8_mode = 5;                                            // u8 window, octs
    std::vector<QueryBatchInfo> infov(1, info);

    ScanI8Args a{};
    a.panels = dev<int4v>(panels.size(), &panels);
    a.qpanels = dev<int4v>(qpanels.size(), &qpanels);
    a.bias8 = dev<int32_t>(bias.size(), &bias);
    a.info = dev<QueryBatchInfo>(1, &infov);
    a.bin_m1 = dev<float>((size_t)nspans * 2 * Qpad);
    a.bin_m2 = dev<float>((size_t)nspans * 2 * Qpad);
    a.sb_m1 = dev<float>((size_t)nchunks * 2 * Qpad);
    a.sb_m2 = dev<float>((size_t)nchunks * 2 * Qpad);
    a.sb_span = dev<int32_t>((size_t)nchunks * 2 * Qpad);
    a.nspans = nspans; a.Npad = Npad; a.Qpad = Qpad; a.nq_valid = nq;
    a.nchunks = nchunks; a.nqtiles = nqtiles;
    a.spans_per_chunk = (int)(nspans / nchunks); a.chunk_rem = (int)(nspans % nchunks);
    const size_t nw = (size_t)grid * 8;
    unsigned long long *stamps = dev<unsigned long long>(nw * 6);
    CK(hipMemcpyToSymbol(HIP_SYMBOL(g_x16_stamps), &stamps, sizeof(stamps)));

    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float ms = 0;
    for (int rep = 0; rep < 4; ++rep) {
        CK(hipMemset(stamps, 0, nw * 6 * 8));
        CK(hipEventRecord(e0));
        scan_i8x16_kernel<2, 8, 8, 8, 2, 0><<<grid, 512>>>(a);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("launch %d: %.3f ms (stamped)\n", rep, ms);
    }
    std::vector<unsigned long long> h(nw * 6);
    CK(hipMemcpy(h.data(), stamps, nw * 6 * 8, hipMemcpyDeviceToHost));
    for (int half = 0; half < 2; ++half) {                       // waves 0-3 / waves 4-7 of a workgroup
        std::vector<double> hand, flush, per_stage, hshare, fshare;
        for (size_t w = 0; w < nw; ++w) {
            if ((int)((w & 7) >> 2) != half || h[w * 6 + 5] == 0 || h[w * 6 + 1] == 0) continue;   // padded waves record nothing
            const double st = (double)h[w * 6 + 5], loop = (double)h[w * 6 + 4];
            hand.push_back((double)h[w * 6] / (double)h[w * 6 + 1]);
            if (h[w * 6 + 3]) flush.push_back((double)h[w * 6 + 2] / (double)h[w * 6 + 3]);
            per_stage.push_back(loop / st);
            hshare.push_back((double)h[w * 6] / loop);
            fshare.push_back((double)h[w * 6 + 2] / loop);
        }
        auto med = [](std::vector<double> &v) { if (v.empty()) return 0.0; std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end()); return v[v.size() / 2]; };
        printf("waves %d-%d: %zu computing waves | cycles per stage %.0f | hand-over (last MFMA of a stage -> first of the next) %.0f cycles = %.4f of the loop | "
               "flush_bin %.0f cycles per flush (one per 2 stages) = %.4f of the loop\n",
               half * 4, half * 4 + 3, hand.size(), med(per_stage), med(hand), med(hshare), med(flush), med(fshare));
    }
    return 0;
}

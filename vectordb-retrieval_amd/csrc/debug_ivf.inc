// debug_ivf.inc -- test hook for the fp16 scan error bound + IVF-Flat entry points.
// Included at the end of vdbhip.hip (same translation unit).

namespace {

// one wave = one 32x32 score tile, computed with exactly the MFMA sequence of scan_kernel
template <int KSTEPS>
__global__ __launch_bounds__(64) void debug_scores_kernel(const half8 *panels, const float *bias, const half8 *qpanels,
                                                          const QueryBatchInfo *info, int64_t tile0, int64_t ntiles,
                                                          int64_t nq, int64_t row0, int64_t nrows, int64_t N,
                                                          float *out) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int64_t tile = tile0 + blockIdx.x;
    const int64_t qt = blockIdx.y;
    if (tile >= tile0 + ntiles) return;
    const float cs = info->cs;
    const int64_t span = tile / kTilesPerSpan;
    const int t = (int)(tile - span * kTilesPerSpan);
    float16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float bv = bias[span * kSpanRows + h * kBinRows + t * 16 + r];
        acc[r] = (bv >= 0.9e38f) ? kPadBias : bv * cs;
    }
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const half8 af = panels[((size_t)tile * KSTEPS + ks) * 64 + lane];
        const half8 bf = qpanels[((size_t)qt * KSTEPS + ks) * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc, 0, 0, 0);
    }
    const int64_t q = qt * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = span * kSpanRows + (int64_t)h * kBinRows + t * 16 + r;
        if (q < nq && row >= row0 && row < row0 + nrows && row < N) out[(size_t)q * nrows + (row - row0)] = acc[r];
    }
}

// p16 layout (D > 128): one wave = one 16x16 score tile, the MFMA sequence of scan16_kloop_kernel (KS 32-dim k-steps)
__global__ __launch_bounds__(64) void debug_scores16_kernel(const half8 *panels, const float *bias, const half8 *qpanels,
                                                            const QueryBatchInfo *info, int64_t tile0, int64_t ntiles,
                                                            int64_t nq, int64_t row0, int64_t nrows, int64_t N,
                                                            float *out, int KS) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int64_t tile = tile0 + blockIdx.x;
    const int64_t qb = blockIdx.y;
    if (tile >= tile0 + ntiles) return;
    const float cs = info->cs;
    const int64_t span = tile / kTilesPerSpan16;
    const int t = (int)(tile - span * kTilesPerSpan16);
    const int64_t rbase = span * kSpanRows16 + (int64_t)g * kBinRows + 4 * t;
    float4v acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float bv = bias[rbase + i];
        acc[i] = (bv >= 0.9e38f) ? kPadBias : bv * cs;
    }
    for (int ks = 0; ks < KS; ++ks) {
        const half8 af = panels[((size_t)tile * KS + ks) * 64 + lane];
        const half8 bf = qpanels[((size_t)qb * KS + ks) * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc, 0, 0, 0);
    }
    const int64_t q = qb * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = rbase + i;
        if (q < nq && row >= row0 && row < row0 + nrows && row < N) out[(size_t)q * nrows + (row - row0)] = acc[i];
    }
}

// layout "x16" (D <= 128): one wave = one 32-row tile x one 16-query block, the MFMA sequence of scan_x16_body's mfma_phase
// (KS2 32-dim k-steps) for each of the tile's two 16-row blocks rb.  Accumulator register i of lane l: query 16 qb + (l & 15),
// corpus row 512 s + 128 (l >> 4) + 8 t + 4 rb + i (build_panels_kernel).
__global__ __launch_bounds__(64) void debug_scores_x16_kernel(const half8 *panels, const float *bias, const half8 *qpanels,
                                                              const QueryBatchInfo *info, int64_t tile0, int64_t ntiles,
                                                              int64_t nq, int64_t row0, int64_t nrows, int64_t N,
                                                              float *out, int KS2) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int64_t tile = tile0 + blockIdx.x;
    const int64_t qb = blockIdx.y;
    if (tile >= tile0 + ntiles) return;
    const float cs = info->cs;
    const int64_t span = tile / kTilesPerSpan;
    const int t = (int)(tile - span * kTilesPerSpan);
    const int64_t q = qb * 16 + (lane & 15);
    for (int rb = 0; rb < 2; ++rb) {
        const int64_t rbase = span * kSpanRows + (int64_t)g * 128 + 8 * t + 4 * rb;
        float4v acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {      // (the scan's LDS bias staging: pad rows start from kPadBias)
            const float bv = bias[rbase + i];
            acc[i] = (bv >= 0.9e38f) ? kPadBias : bv * cs;
        }
        for (int ks2 = 0; ks2 < KS2; ++ks2) {
            const half8 af = panels[((size_t)tile * 2 * KS2 + 2 * ks2 + rb) * 64 + lane];
            const half8 bf = qpanels[((size_t)qb * KS2 + ks2) * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = rbase + i;
            if (q < nq && row >= row0 && row < row0 + nrows && row < N) out[(size_t)q * nrows + (row - row0)] = acc[i];
        }
    }
}

}  // namespace

extern "C" {

int vdb_debug_scan_scores(vdb_handle hh, const float *q_host, int64_t nq, int64_t row0, int64_t nrows,
                          float *scores_host, float *eps_host, double *cscale) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_debug_scan_scores", kAnyKind & ~kMulti);
        if (!h->built || !h->scan_ok || h->panels_streamed || !h->scan.panels.p) throw Error(VDB_ERR_STATE, "scan copy not available for this index");
        // panel layouts with a kernel here: p16 (D > 128), "x16" and the 32x32 form (D <= 128)
        const bool t32 = !h->tile16 && !h->x16;
        if (t32 && h->ksteps > kMaxKSteps) throw Error(VDB_ERR_UNSUPPORTED, "debug scores for D > 128 need the p16 panel layout");
        if (nq <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > h->N) throw Error(VDB_ERR_INVALID, "bad range");
        set_device(h->device);
        hipStream_t st = nullptr;
        const int Dm = h->dim;
        DevBuf dq, info, qpanels, eps, out;
        const int64_t Qpad = (nq + 31) / 32 * 32;
        dq.reserve((size_t)nq * Dm * 4);
        info.reserve(sizeof(QueryBatchInfo));
        qpanels.reserve((size_t)(Qpad / 32) * h->ksteps * 64 * sizeof(half8));
        eps.reserve((size_t)nq * 4);
        out.reserve((size_t)nq * nrows * 4);
        VDB_HIP(hipMemcpyAsync(dq.p, q_host, (size_t)nq * Dm * 4, hipMemcpyHostToDevice, st));
        VDB_HIP(hipMemsetAsync(info.p, 0, sizeof(QueryBatchInfo), st));
        VDB_HIP(hipMemsetAsync(out.p, 0, (size_t)nq * nrows * 4, st));
        const int64_t total = nq * Dm;
        query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, st>>>(dq.as<float>(), total, info.as<QueryBatchInfo>(),
            FinalizeArgs{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2, 0});
        const int64_t threads = (Qpad / 32) * h->ksteps * 64;
        if (t32)
            build_qpanels_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(dq.as<float>(), nq, Dm, h->D4, h->ksteps, Qpad / 32, info.as<QueryBatchInfo>(), qpanels.as<half8>());
        else    // (p16 and "x16" take the same B fragments: [q / 16][32-dim k-step][lane])
            build_qpanels16_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(dq.as<float>(), nq, Dm, h->ksteps / 2, Qpad / 16, info.as<QueryBatchInfo>(), qpanels.as<half8>());
        EpsArgs ea{dq.as<float>(), nq, Dm, h->ksteps * 16, h->metric, sqrtf(h->maxnorm2) * 1.0000002f,
                   h->corpus_fp16_exact ? 1 : 0, h->corpus_int_unscaled ? 1 : 0, h->sx, info.as<QueryBatchInfo>(),
                   eps.as<float>()};
        query_eps_kernel<<<dim3((unsigned)((nq * 16 + 255) / 256)), dim3(256), 0, st>>>(ea);
        const int span_rows = h->tile16 ? kSpanRows16 : kSpanRows, tps = h->tile16 ? kTilesPerSpan16 : kTilesPerSpan;
        const int64_t sp0 = row0 / span_rows, sp1 = (row0 + nrows + span_rows - 1) / span_rows;
        const int64_t tile0 = sp0 * tps, ntiles = (sp1 - sp0) * tps;
        const dim3 grid((unsigned)ntiles, (unsigned)(Qpad / (t32 ? 32 : 16)));
        if (h->tile16)
            debug_scores16_kernel<<<grid, dim3(64), 0, st>>>(h->scan.panels.as<half8>(), h->scan.bias.as<float>(), qpanels.as<half8>(), info.as<QueryBatchInfo>(), tile0, ntiles, nq, row0, nrows, h->N, out.as<float>(), h->ksteps / 2);
        else if (h->x16)
            debug_scores_x16_kernel<<<grid, dim3(64), 0, st>>>(h->scan.panels.as<half8>(), h->scan.bias.as<float>(), qpanels.as<half8>(), info.as<QueryBatchInfo>(), tile0, ntiles, nq, row0, nrows, h->N, out.as<float>(), h->ksteps / 2);
        else if (h->ksteps == 4)
            debug_scores_kernel<4><<<grid, dim3(64), 0, st>>>(h->scan.panels.as<half8>(), h->scan.bias.as<float>(), qpanels.as<half8>(), info.as<QueryBatchInfo>(), tile0, ntiles, nq, row0, nrows, h->N, out.as<float>());
        else
            debug_scores_kernel<8><<<grid, dim3(64), 0, st>>>(h->scan.panels.as<half8>(), h->scan.bias.as<float>(), qpanels.as<half8>(), info.as<QueryBatchInfo>(), tile0, ntiles, nq, row0, nrows, h->N, out.as<float>());
        VDB_HIP(hipGetLastError());
        QueryBatchInfo hi;
        VDB_HIP(hipMemcpyAsync(scores_host, out.p, (size_t)nq * nrows * 4, hipMemcpyDeviceToHost, st));
        VDB_HIP(hipMemcpyAsync(eps_host, eps.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        VDB_HIP(hipMemcpyAsync(&hi, info.p, sizeof(hi), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        if (cscale) *cscale = (double)hi.cs;
    });
}

}  // extern "C"

#include "ivf.inc"

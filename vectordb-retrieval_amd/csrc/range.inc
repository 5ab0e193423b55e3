// range.inc -- host side of the range search (kernels: range.hpp; sizes: range_plan.hpp): vdb_range_search / _results and their
// device variants.  Included by vdbhip.hip; the handle's last result lives in vdb_index_s (range, range_*).

namespace {

// the kinds that keep float32 rows (or their int8 row copy) in insertion order on one device
constexpr unsigned kRangeCalls = kFlat | kLsh | kLsht | kKnng;

// a resident fp16 copy in one of the two layouts the prefilter scans read ("x16", p16); every other handle takes the all-ones path
inline bool range_has_scan(const vdb_index_s *h) {
    return h->scan_ok && !h->panels_streamed && !h->int8_only && h->scan.panels.p && h->scan.bias.p && (h->x16 || h->tile16);
}

void range_check(vdb_index_s *h, const char *what, const void *q, int64_t nq, float radius, const void *lims) {
    admit(h, what, kRangeCalls);
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + " is not available with option 'graph'");
    if (nq <= 0) throw Error(VDB_ERR_INVALID, "the query count must be positive");
    if (!q || !lims) throw Error(VDB_ERR_INVALID, "null pointer");
    if (radius != radius) throw Error(VDB_ERR_INVALID, "the radius is NaN");
}

void range_require_result(vdb_index_s *h, const char *what) {
    admit(h, what, kRangeCalls);
    if (!h->range_valid)
        throw Error(VDB_ERR_STATE, std::string(what) + ": no range result on this handle (none yet, or an add, a reset or an option change dropped it)");
}

// the whole device pipeline of one call; leaves lims (nq + 1), D and I of the result in h->range and the counts in h->range_*
void range_search_impl(vdb_index_s *h, const float *dq, int64_t nq, float radius, hipStream_t st) {
    RangeBufs &rb = h->range;
    h->range_valid = false;
    const int D = h->dim, D4 = h->D4, ks32 = h->ksteps / 2;
    const int64_t N = h->N, W = range_words(N);
    const int S = (int)range_segments(N);
    const bool scan = range_has_scan(h);
    const int64_t slab = range_slab_queries(nq, N, h->opt.range_bitmap_mb);
    const int64_t slab_pad = (slab + 31) / 32 * 32;
    const size_t stat_bytes = (size_t)kStatShards * kStatStride * sizeof(unsigned long long);
    rb.lims.reserve((size_t)(nq + 1) * sizeof(int64_t));
    rb.stat.reserve(stat_bytes);
    rb.bitmap.reserve((size_t)slab * W * sizeof(unsigned));
    rb.seg.reserve((size_t)slab * S * sizeof(int));
    rb.qtot.reserve((size_t)slab * sizeof(int64_t));
    if (D4 != D) rb.qpad.reserve((size_t)nq * D4 * sizeof(float));
    if (scan) {
        rb.info.reserve(sizeof(QueryBatchInfo));
        rb.eps.reserve((size_t)nq * sizeof(float));
        rb.thr.reserve((size_t)nq * sizeof(float));
        rb.flag.reserve((size_t)nq * sizeof(int));
        rb.qpanels.reserve((size_t)(slab_pad / 16) * ks32 * 64 * sizeof(half8));
    }
    VDB_HIP(hipMemsetAsync(rb.stat.p, 0, stat_bytes, st));
    VDB_HIP(hipMemsetAsync(rb.lims.p, 0, sizeof(int64_t), st));
    h->last.last_path = VDB_PATH_RANGE;
    h->last.last_nq = nq;
    h->range_cand = h->range_fb = 0;
    const long tslot = timing_begin(h, st);
    const float *qp = dq;
    if (D4 != D) {
        pad_rows_kernel<<<dim3((unsigned)((nq * D4 + 255) / 256)), dim3(256), 0, st>>>(dq, nq, D, D4, rb.qpad.as<float>());
        qp = rb.qpad.as<float>();
    }
    if (scan) {       // statistics, bound and threshold of the whole batch (the scale cs belongs to the batch, not to a slab)
        VDB_HIP(hipMemsetAsync(rb.info.p, 0, sizeof(QueryBatchInfo), st));
        const int64_t total = nq * D;
        query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, st>>>(dq, total, rb.info.as<QueryBatchInfo>(),
            FinalizeArgs{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2, 0});
        EpsArgs ea{dq, nq, D, h->ksteps * 16, h->metric, sqrtf(h->maxnorm2) * 1.0000002f, h->corpus_fp16_exact ? 1 : 0,
                   h->corpus_int_unscaled ? 1 : 0, h->sx, rb.info.as<QueryBatchInfo>(), rb.eps.as<float>()};
        query_eps_kernel<<<dim3((unsigned)((nq * 16 + 255) / 256)), dim3(256), 0, st>>>(ea);
        RangeThrArgs ta{dq, nq, D, h->metric, radius, rb.info.as<QueryBatchInfo>(), rb.eps.as<float>(), rb.thr.as<float>(),
                        rb.flag.as<int>(), rb.stat.as<unsigned long long>()};
        range_thr_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st>>>(ta);
        VDB_HIP(hipGetLastError());
    }
    int64_t total = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += slab) {
        const int64_t n = std::min<int64_t>(slab, nq - q0);
        if (q0 == 0) timing_mark(h, tslot, 0, st);
        if (scan) {
            const int64_t npad = (n + 31) / 32 * 32;
            const int64_t threads = (npad / 16) * ks32 * 64;
            build_qpanels16_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(dq + (size_t)q0 * D, n, D, ks32, npad / 16,
                                                                                                 rb.info.as<QueryBatchInfo>(), rb.qpanels.as<half8>());
            RangeScanArgs sa{h->scan.panels.as<half8>(), h->scan.bias.as<float>(), rb.qpanels.as<half8>(), rb.info.as<QueryBatchInfo>(),
                             rb.thr.as<float>() + q0, rb.flag.as<int>() + q0, n, N, 0, W, rb.bitmap.as<unsigned>()};
            const unsigned qtiles = (unsigned)((n + kRangeQueryTile - 1) / kRangeQueryTile);
            if (h->tile16) {
                sa.nspans = h->Npad / kSpanRows16;
                range_scan_p16_kernel<<<dim3((unsigned)(W / (kSpanRows16 / kRangeWordBits)), qtiles), dim3(256), 0, st>>>(sa, ks32);
            } else {
                sa.nspans = h->Npad / kSpanRows;
                const dim3 grid((unsigned)(W / (kSpanRows / kRangeWordBits)), qtiles);
                if (ks32 == 2) range_scan_x16_kernel<2><<<grid, dim3(256), 0, st>>>(sa);
                else range_scan_x16_kernel<4><<<grid, dim3(256), 0, st>>>(sa);
            }
        } else {
            range_fill_kernel<<<dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, st>>>(rb.bitmap.as<unsigned>(), n, W, N);
        }
        VDB_HIP(hipGetLastError());
        timing_mark(h, tslot, 1, st);
        RangeTailArgs ta{};
        ta.c = flat_rows(h, qp + (size_t)q0 * D4, 1);
        ta.nq = n;
        ta.W = W;
        ta.S = S;
        ta.radius = radius;
        ta.bitmap = rb.bitmap.as<unsigned>();
        ta.seg = rb.seg.as<int>();
        ta.qtot = rb.qtot.as<int64_t>();
        ta.lims = rb.lims.as<int64_t>() + q0;
        ta.stat = rb.stat.as<unsigned long long>();
        const unsigned unit_blocks = (unsigned)((n * S + 3) / 4);
        range_filter_kernel<<<dim3(unit_blocks), dim3(256), 0, st>>>(ta);
        range_seg_prefix_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st>>>(ta);
        range_lims_kernel<<<dim3(1), dim3(256), 0, st>>>(ta);
        VDB_HIP(hipGetLastError());
        // the one host synchronisation of the slab: its result count sizes the result buffers
        int64_t end = 0;
        VDB_HIP(hipMemcpyAsync(&end, rb.lims.as<int64_t>() + q0 + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        if (end < total) throw Error(VDB_ERR_HIP, "internal: the range result shrank");
        rb.D.grow((size_t)end * sizeof(float), (size_t)total * sizeof(float));
        rb.I.grow((size_t)end * sizeof(int64_t), (size_t)total * sizeof(int64_t));
        ta.D = rb.D.as<float>();
        ta.I = rb.I.as<int64_t>();
        if (end > total) range_emit_kernel<<<dim3(unit_blocks), dim3(256), 0, st>>>(ta);
        VDB_HIP(hipGetLastError());
        total = end;
    }
    timing_mark(h, tslot, 2, st);
    std::vector<unsigned long long> c((size_t)kStatShards * kStatStride);
    VDB_HIP(hipMemcpyAsync(c.data(), rb.stat.p, stat_bytes, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
    for (int sh = 0; sh < kStatShards; ++sh) {
        h->range_cand += (int64_t)c[(size_t)sh * kStatStride];
        h->range_fb += (int64_t)c[(size_t)sh * kStatStride + 1];
    }
    if (!scan) h->range_fb = nq;
    h->range_total = total;
    h->range_nq = nq;
    h->range_valid = true;
}

}  // namespace

extern "C" {

int vdb_range_search_device(vdb_handle hh, const float *q_dev, int64_t nq, float radius, int64_t *lims_dev, int64_t *total_host, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        range_check(h, "vdb_range_search_device", q_dev, nq, radius, lims_dev);
        if (!total_host) throw Error(VDB_ERR_INVALID, "null pointer");
        set_device(h->device);
        hipStream_t st = as_stream(stream);
        range_search_impl(h, q_dev, nq, radius, st);
        VDB_HIP(hipMemcpyAsync(lims_dev, h->range.lims.p, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        *total_host = h->range_total;
    });
}

int vdb_range_search(vdb_handle hh, const float *q_host, int64_t nq, float radius, int64_t *lims_host) {
    return guarded([&] {
        auto *h = check(hh);
        range_check(h, "vdb_range_search", q_host, nq, radius, lims_host);
        set_device(h->device);
        hipStream_t st = nullptr;
        h->range.qstage.reserve((size_t)nq * h->dim * sizeof(float));
        VDB_HIP(hipMemcpyAsync(h->range.qstage.p, q_host, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
        range_search_impl(h, h->range.qstage.as<float>(), nq, radius, st);
        VDB_HIP(hipMemcpyAsync(lims_host, h->range.lims.p, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
    });
}

int vdb_range_results_device(vdb_handle hh, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        range_require_result(h, "vdb_range_results_device");
        if (h->range_total > 0 && (!D_dev || !I_dev)) throw Error(VDB_ERR_INVALID, "null pointer");
        if (h->range_total == 0) return;
        set_device(h->device);
        hipStream_t st = as_stream(stream);
        VDB_HIP(hipMemcpyAsync(D_dev, h->range.D.p, (size_t)h->range_total * sizeof(float), hipMemcpyDeviceToDevice, st));
        VDB_HIP(hipMemcpyAsync(I_dev, h->range.I.p, (size_t)h->range_total * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    });
}

int vdb_range_results(vdb_handle hh, float *D_host, int64_t *I_host) {
    return guarded([&] {
        auto *h = check(hh);
        range_require_result(h, "vdb_range_results");
        if (h->range_total > 0 && (!D_host || !I_host)) throw Error(VDB_ERR_INVALID, "null pointer");
        if (h->range_total == 0) return;
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        VDB_HIP(hipMemcpy(D_host, h->range.D.p, (size_t)h->range_total * sizeof(float), hipMemcpyDeviceToHost));
        VDB_HIP(hipMemcpy(I_host, h->range.I.p, (size_t)h->range_total * sizeof(int64_t), hipMemcpyDeviceToHost));
    });
}

}  // extern "C"

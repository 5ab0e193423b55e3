// ivf_range.inc -- host side of the range search on IVF-Flat indexes (kernels: ivf_range.hpp; rules: ivf_range_plan.hpp):
// vdb_ivf_range_search / _results and their device variants.  Included by vdbhip.hip behind ivf.inc; the handle's last result lives
// where the flat range search keeps its own (vdb_index_s::range, range_*): a handle is of one kind, so only one of the two families
// of calls ever reaches it.

namespace {

// IVF-Flat on one device; a flat handle without centroids is admitted and told what vdb_ivf_search tells it
constexpr unsigned kIvfRangeCalls = kFlat | kIvfFlat;

void ivf_range_admit(vdb_index_s *h, const char *what) {
    admit(h, what, kIvfRangeCalls);
    if (h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + " is not available with option 'graph'");
    ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
}

void ivf_range_check(vdb_index_s *h, const char *what, const void *q, int64_t nq, float radius, const void *lims) {
    ivf_range_admit(h, what);
    if (h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (nq <= 0) throw Error(VDB_ERR_INVALID, "the query count must be positive");
    if (!q || !lims) throw Error(VDB_ERR_INVALID, "null pointer");
    if (radius != radius) throw Error(VDB_ERR_INVALID, "the radius is NaN");
}

void ivf_range_require_result(vdb_index_s *h, const char *what) {
    ivf_range_admit(h, what);
    if (!h->range_valid)
        throw Error(VDB_ERR_STATE, std::string(what) + ": no range result on this handle (none yet, or an add, a reset, an option change or new "
                                                       "centroids dropped it)");
}

// the list-major front of one slab: ivf_search_lists up to the scan, without the int8 scan; then the threshold and the marks
void ivf_range_lists(IvfBatch &b, float radius) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    RangeBufs &rb = h->range;
    b.shape.has_i8 = false;                    // (no int8 query rows, i8_mode stays 0: an integer batch runs on the fp16 panels)
    const IvfLists L = ivf_lists_reserve(b);
    ivf_lists_prep(b, L);
    ivf_lists_plan(b, L);
    ScanArgs sa{};
    sa.panels = h->scan.panels.as<half8>();
    sa.bias = h->scan.bias.as<float>();
    sa.qpanels = nullptr;
    sa.qrows = reinterpret_cast<const _Float16 *>(ws.qpanels.p);
    sa.slot_query = L.d_slot_query;
    sa.info = L.info;
    sa.bin_m1 = ws.bin_m1.as<float>(); sa.bin_m2 = ws.bin_m2.as<float>(); sa.bin_m3 = ws.bin_m3.as<float>();
    sa.item_list = h->plan.ivf_item_list.as<int32_t>(); sa.item_slot0 = h->plan.ivf_item_slot0.as<int32_t>();
    sa.item_bin0 = h->plan.ivf_item_bin0.as<int32_t>();
    sa.n_items = &L.plan->n_items;
    sa.list_pspan0 = h->lists.ivf_list_pspan0.as<int32_t>();
    timing_mark(h, b.tslot, 0, b.st);
    if (b.g.kloop) ivf_scan_kloop(b, L.c.kgroup, sa);
    else ivf_scan_fp16(b, sa);
    timing_mark(h, b.tslot, 1, b.st);
    RangeThrArgs ta{b.q, b.nb, h->dim, h->metric, radius, L.info, ws.eps.as<float>(), rb.thr.as<float>(), rb.flag.as<int>(),
                    rb.stat.as<unsigned long long>()};
    range_thr_kernel<<<dim3((unsigned)((b.nb + 255) / 256)), dim3(256), 0, b.st>>>(ta);
    const IvfSelectCaps sc = ivf_select_caps(b.shape, b.g, L.c, b.k, b.nprobe);
    IvfRangeMarkArgs ma{};
    ma.bin_m[0] = sa.bin_m1; ma.bin_m[1] = sa.bin_m2; ma.bin_m[2] = sa.bin_m3;
    ma.bin_m[3] = b.g.kloop ? ws.bin_m4.as<float>() : nullptr;
    ma.bin_m[4] = b.g.kloop ? ws.bin_m5.as<float>() : nullptr;
    ma.nm = sc.nm;
    ma.thr = rb.thr.as<float>(); ma.flag = rb.flag.as<int>();
    ma.plan = L.plan; ma.probes = L.probes; ma.offsets = h->lists.ivf_offsets.as<int64_t>();
    ma.slot_of = h->plan.ivf_slot_of.as<int32_t>(); ma.slot_off = h->plan.ivf_slot_off.as<int32_t>();
    ma.list_item0 = h->plan.ivf_list_item0.as<int32_t>(); ma.item_bin0 = h->plan.ivf_item_bin0.as<int32_t>();
    ma.list_pspan0 = h->lists.ivf_list_pspan0.as<int32_t>();
    ma.span_row0 = h->lists.ivf_span_row0.as<int32_t>(); ma.span_valid = h->lists.ivf_span_valid.as<int32_t>();
    ma.nq = b.nb; ma.N = h->N; ma.W = range_words(h->N);
    ma.nprobe = b.nprobe; ma.nlist = h->nlist; ma.group = b.g.group;
    ma.max_entries = sc.max_entries; ma.probe_cap = ivf_range_probe_cap(b.nprobe);
    ma.group_rows = b.g.kloop ? L.c.kgroup : 4;
    ma.bins_per_span = b.g.bins_per_span; ma.bin_rows = b.g.bin_rows; ma.run_groups = b.g.run_groups;
    ma.fill = 0;
    ma.bitmap = rb.bitmap.as<unsigned>();
    ma.stat = rb.stat.as<unsigned long long>();
    ivf_range_mark_kernel<<<dim3((unsigned)((b.nb + 1) / 2)), dim3(128), 2 * ivf_range_mark_lds_words(b.nprobe) * 4, b.st>>>(ma);
    VDB_HIP(hipGetLastError());
}

// the exact route of one slab: every row of the probed lists is a candidate, no scan
void ivf_range_exact(const IvfBatch &b) {
    vdb_index_s *h = b.h;
    timing_mark(h, b.tslot, 0, b.st);
    IvfRangeMarkArgs ma{};
    ma.probes = h->plan.ivf_probe_i.as<int64_t>(); ma.offsets = h->lists.ivf_offsets.as<int64_t>();
    ma.nq = b.nb; ma.N = h->N; ma.W = range_words(h->N);
    ma.nprobe = b.nprobe; ma.nlist = h->nlist;
    ma.fill = 1;
    ma.bitmap = h->range.bitmap.as<unsigned>();
    ivf_range_mark_kernel<<<dim3((unsigned)((b.nb + 1) / 2)), dim3(128), 0, b.st>>>(ma);
    VDB_HIP(hipGetLastError());
    timing_mark(h, b.tslot, 1, b.st);
}

// the whole device pipeline of one call; leaves lims (nq + 1), D and I of the result in h->range and the counts in h->range_*
void ivf_range_search_impl(vdb_index_s *h, const float *dq, int64_t nq, float radius, hipStream_t st) {
    RangeBufs &rb = h->range;
    Workspace &ws = h->ws;
    h->range_valid = false;
    const int Dm = h->dim, D4 = h->D4;
    const int64_t N = h->N, W = range_words(N);
    const int S = (int)range_segments(N);
    const int nprobe = std::max(1, std::min(h->nprobe, h->nlist));
    const int64_t slab = ivf_range_slab_queries(nq, N, h->opt.range_bitmap_mb);
    const size_t stat_bytes = (size_t)kStatShards * kStatStride * sizeof(unsigned long long);
    rb.lims.reserve((size_t)(nq + 1) * sizeof(int64_t));
    rb.stat.reserve(stat_bytes);
    rb.bitmap.reserve((size_t)slab * W * sizeof(unsigned));
    rb.seg.reserve((size_t)slab * S * sizeof(int));
    rb.qtot.reserve((size_t)slab * sizeof(int64_t));
    rb.thr.reserve((size_t)slab * sizeof(float));
    rb.flag.reserve((size_t)slab * sizeof(int));
    VDB_HIP(hipMemsetAsync(rb.stat.p, 0, stat_bytes, st));
    VDB_HIP(hipMemsetAsync(rb.lims.p, 0, sizeof(int64_t), st));
    h->last.last_path = VDB_PATH_IVF_RANGE;
    h->last.last_nq = nq;
    h->range_cand = h->range_fb = 0;
    const IvfIndexShape shape = ivf_shape_of(h);
    int64_t total = 0, fb_exact = 0;
    const size_t ev_mark = h->ev_used;
    try {
    for (int64_t q0 = 0; q0 < nq; q0 += slab) {
        IvfBatch b{};
        b.h = h; b.k = 1; b.nprobe = nprobe; b.st = st;
        b.nb = std::min<int64_t>(slab, nq - q0);
        b.q = dq + (size_t)q0 * Dm;
        b.shape = shape;
        b.g = ivf_geometry(shape, h->opt, b.nb, 1, nprobe);
        const bool lists = ivf_range_route(b.g.ok, h->opt.force_path) == 1;
        if (!lists) b.g = IvfGeom{};
        // the front of every IVF batch (ivf_search_device_impl): one memset of what the batch needs zeroed, the coarse search, padded queries
        b.d_cnt = ivf_bind_zero(h, lists ? b.g.cnt_words : 0);
        VDB_HIP(hipMemsetAsync(h->plan.ivf_zero.p, 0, 2 * kZeroSmall + (lists ? b.g.cnt_words * 4 : 0), st));
        h->coarse->small_preset = true;
        b.tslot = timing_begin(h, st);
        h->plan.ivf_probe_d.reserve((size_t)b.nb * nprobe * sizeof(float));
        h->plan.ivf_probe_i.reserve((size_t)b.nb * nprobe * sizeof(int64_t));
        search_device_impl(h->coarse, b.q, b.nb, nprobe, h->plan.ivf_probe_d.as<float>(), h->plan.ivf_probe_i.as<int64_t>(), nullptr, nullptr, st);
        b.qpad = b.q;
        if (D4 != Dm) {
            ws.qpad.reserve((size_t)b.nb * D4 * sizeof(float));
            pad_rows_kernel<<<dim3((unsigned)((b.nb * D4 + 255) / 256)), dim3(256), 0, st>>>(b.q, b.nb, Dm, D4, ws.qpad.as<float>());
            b.qpad = ws.qpad.as<float>();
        }
        // the wave of a query ORs its marks into a cleared bitmap row
        VDB_HIP(hipMemsetAsync(rb.bitmap.p, 0, (size_t)b.nb * W * sizeof(unsigned), st));
        if (lists) {
            ivf_range_lists(b, radius);
        } else {
            ivf_range_exact(b);
            fb_exact += b.nb;
        }
        RangeTailArgs ta{};
        ta.c = RefineCommon{h->rows.x32.as<float>(), b.qpad, N, h->id_base, D4, h->metric, 1, h->lists.ivf_ids.as<int64_t>()};
        ta.nq = b.nb;
        ta.W = W;
        ta.S = S;
        ta.radius = radius;
        ta.bitmap = rb.bitmap.as<unsigned>();
        ta.seg = rb.seg.as<int>();
        ta.qtot = rb.qtot.as<int64_t>();
        ta.lims = rb.lims.as<int64_t>() + q0;
        ta.stat = rb.stat.as<unsigned long long>();
        const unsigned unit_blocks = (unsigned)((b.nb * S + 3) / 4);
        range_filter_kernel<<<dim3(unit_blocks), dim3(256), 0, st>>>(ta);
        range_seg_prefix_kernel<<<dim3((unsigned)((b.nb + 3) / 4)), dim3(256), 0, st>>>(ta);
        range_lims_kernel<<<dim3(1), dim3(256), 0, st>>>(ta);
        VDB_HIP(hipGetLastError());
        // the one host synchronisation of the slab: its result count sizes the result buffers
        int64_t end = 0;
        VDB_HIP(hipMemcpyAsync(&end, rb.lims.as<int64_t>() + q0 + b.nb, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        if (end < total) throw Error(VDB_ERR_HIP, "internal: the range result shrank");
        rb.D.grow((size_t)end * sizeof(float), (size_t)total * sizeof(float));
        rb.I.grow((size_t)end * sizeof(int64_t), (size_t)total * sizeof(int64_t));
        ta.D = rb.D.as<float>();
        ta.I = rb.I.as<int64_t>();
        if (end > total) ivf_range_emit_kernel<<<dim3(unit_blocks), dim3(256), 0, st>>>(ta);
        VDB_HIP(hipGetLastError());
        total = end;
        timing_mark(h, b.tslot, 2, st);
    }
    } catch (...) {
        h->ev_used = ev_mark;
        if (h->coarse) h->coarse->small_preset = false;
        throw;
    }
    std::vector<unsigned long long> c((size_t)kStatShards * kStatStride);
    VDB_HIP(hipMemcpyAsync(c.data(), rb.stat.p, stat_bytes, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
    for (int sh = 0; sh < kStatShards; ++sh) {
        h->range_cand += (int64_t)c[(size_t)sh * kStatStride];
        h->range_fb += (int64_t)c[(size_t)sh * kStatStride + 1];
    }
    h->range_fb += fb_exact;
    h->ivf_last_mfma = fb_exact < nq;          // (as every IVF call leaves it: a list scan served some slab of this one)
    h->range_total = total;
    h->range_nq = nq;
    h->range_valid = true;
}

}  // namespace

extern "C" {

int vdb_ivf_range_search_device(vdb_handle hh, const float *q_dev, int64_t nq, float radius, int64_t *lims_dev, int64_t *total_host, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_range_check(h, "vdb_ivf_range_search_device", q_dev, nq, radius, lims_dev);
        if (!total_host) throw Error(VDB_ERR_INVALID, "null pointer");
        set_device(h->device);
        hipStream_t st = as_stream(stream);
        ivf_range_search_impl(h, q_dev, nq, radius, st);
        VDB_HIP(hipMemcpyAsync(lims_dev, h->range.lims.p, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        *total_host = h->range_total;
    });
}

int vdb_ivf_range_search(vdb_handle hh, const float *q_host, int64_t nq, float radius, int64_t *lims_host) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_range_check(h, "vdb_ivf_range_search", q_host, nq, radius, lims_host);
        set_device(h->device);
        hipStream_t st = nullptr;
        h->range.qstage.reserve((size_t)nq * h->dim * sizeof(float));
        VDB_HIP(hipMemcpyAsync(h->range.qstage.p, q_host, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
        ivf_range_search_impl(h, h->range.qstage.as<float>(), nq, radius, st);
        VDB_HIP(hipMemcpyAsync(lims_host, h->range.lims.p, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
    });
}

int vdb_ivf_range_results_device(vdb_handle hh, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_range_require_result(h, "vdb_ivf_range_results_device");
        if (h->range_total > 0 && (!D_dev || !I_dev)) throw Error(VDB_ERR_INVALID, "null pointer");
        if (h->range_total == 0) return;
        set_device(h->device);
        hipStream_t st = as_stream(stream);
        VDB_HIP(hipMemcpyAsync(D_dev, h->range.D.p, (size_t)h->range_total * sizeof(float), hipMemcpyDeviceToDevice, st));
        VDB_HIP(hipMemcpyAsync(I_dev, h->range.I.p, (size_t)h->range_total * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    });
}

int vdb_ivf_range_results(vdb_handle hh, float *D_host, int64_t *I_host) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_range_require_result(h, "vdb_ivf_range_results");
        if (h->range_total > 0 && (!D_host || !I_host)) throw Error(VDB_ERR_INVALID, "null pointer");
        if (h->range_total == 0) return;
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        VDB_HIP(hipMemcpy(D_host, h->range.D.p, (size_t)h->range_total * sizeof(float), hipMemcpyDeviceToHost));
        VDB_HIP(hipMemcpy(I_host, h->range.I.p, (size_t)h->range_total * sizeof(int64_t), hipMemcpyDeviceToHost));
    });
}

}  // extern "C"

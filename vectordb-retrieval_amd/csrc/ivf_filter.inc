// ivf_filter.inc -- host side of the filtered k-NN search on IVF-Flat indexes (kernels: ivf_filter.hpp; rules: ivf_filter_plan.hpp):
// vdb_ivf_filter_set (+ _device), vdb_ivf_filter_count, vdb_ivf_search_filtered (+ _device).  Included by vdbhip.hip; the installed
// filter lives in vdb_index_s (ivf_filter, ivf_filter_*) and goes with the flat one (filter_drop; vdb_filter_clear frees both).  The
// search is ivf_search_device_impl itself (ivf.inc) with `filtered` set.

namespace {

// IVF-Flat on one device; a flat handle without centroids is admitted and told what vdb_ivf_search tells it
constexpr unsigned kIvfFilterCalls = kFlat | kIvfFlat;

void ivf_filter_admit(vdb_index_s *h, const char *what) {
    admit(h, what, kIvfFilterCalls);
    if (h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + " is not available with option 'graph'");
    ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
}

void ivf_filter_require(vdb_index_s *h, const char *what) {
    if (!h->ivf_filter_valid)
        throw Error(VDB_ERR_STATE, std::string(what) + ": no filter on this handle (none installed, or an add, a reset, an option change, "
                                                       "new centroids or a change of kind dropped it): call vdb_ivf_filter_set first");
}

void ivf_filter_set_check(vdb_index_s *h, const char *what, const void *words, int64_t nbits) {
    ivf_filter_admit(h, what);
    if (h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (!words) throw Error(VDB_ERR_INVALID, "null pointer");
    if (nbits != h->N)
        throw Error(VDB_ERR_INVALID, std::string(what) + ": a filter has one bit per row: nbits must equal ntotal = " + std::to_string(h->N) +
                                         ", got " + std::to_string(nbits));
}

void ivf_filter_search_check(vdb_index_s *h, const char *what, const void *q, int64_t nq, int k, const void *D, const void *I) {
    ivf_filter_admit(h, what);
    if (h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    ivf_filter_require(h, what);
    if (nq <= 0) throw Error(VDB_ERR_INVALID, "the query count must be positive");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (!q || !D || !I) throw Error(VDB_ERR_INVALID, "null pointer");
}

// words_dev: (N + 31) / 32 words in device memory, id order.  One stream synchronisation: the admitted count comes back.
void ivf_filter_install(vdb_index_s *h, const uint32_t *words_dev, hipStream_t st) {
    IvfFilterBufs &fb = h->ivf_filter;
    const int64_t N = h->N;
    const bool has_bias = h->ivf_mfma_ok && h->scan.bias.p != nullptr;
    const bool has_bias8 = has_bias && h->i8_ok && h->scan.panels8.p != nullptr && h->scan.bias8.p != nullptr;
    const int64_t panel_rows = h->ivf_pspans * h->ivf_span_rows;
    // An install that replaces a filter writes into the buffers that one holds: every call that changes the rows or the panel space
    // has dropped it, so the sizes are the same and nothing is freed, allocated or synchronised but the stream (the caller orders an
    // install behind filtered searches still running on other streams).  A filter of the flat calls -- the handle was flat then -- goes.
    if (group_bytes(h->filter) > 0) filter_drop(h);
    h->ivf_filter_valid = false;
    h->ivf_filter_count = 0;
    try {
        fb.words.reserve_exact((size_t)ivf_filter_words(N) * sizeof(uint32_t));
        fb.count.reserve_exact(sizeof(unsigned long long));
        if (has_bias) fb.bias_f.reserve_exact((size_t)panel_rows * sizeof(float));
        else fb.bias_f.release();
        if (has_bias8) fb.bias8_f.reserve_exact((size_t)2 * panel_rows * sizeof(int32_t));
        else fb.bias8_f.release();
        VDB_HIP(hipMemsetAsync(fb.count.p, 0, sizeof(unsigned long long), st));
        IvfFilterRowsArgs ra{};
        ra.words_in = words_dev;
        ra.ids = h->lists.ivf_ids.as<int64_t>();
        ra.N = N;
        ra.id_base = h->id_base;
        ra.words = fb.words.as<uint32_t>();
        ra.count = fb.count.as<unsigned long long>();
        ivf_filter_rows_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st>>>(ra);
        VDB_HIP(hipGetLastError());
        if (has_bias) {
            IvfFilterMaskArgs ma{};
            ma.words = fb.words.as<uint32_t>();
            ma.span_row0 = h->lists.ivf_span_row0.as<int32_t>();
            ma.span_valid = h->lists.ivf_span_valid.as<int32_t>();
            ma.panel_rows = panel_rows;
            ma.span_rows = h->ivf_span_rows;
            ma.bias = h->scan.bias.as<float>();
            ma.bias_f = fb.bias_f.as<float>();
            ma.bias8 = has_bias8 ? h->scan.bias8.as<int32_t>() : nullptr;
            ma.bias8_f = fb.bias8_f.as<int32_t>();
            ivf_filter_mask_kernel<<<dim3((unsigned)((panel_rows / 4 + 255) / 256)), dim3(256), 0, st>>>(ma);
            VDB_HIP(hipGetLastError());
        }
        unsigned long long n = 0;
        VDB_HIP(hipMemcpyAsync(&n, fb.count.p, sizeof(n), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        if ((int64_t)n > N) throw Error(VDB_ERR_HIP, "internal: the filter admits more rows than the index holds");
        h->ivf_filter_count = (int64_t)n;
    } catch (...) {                    // (a failed allocation: the handle keeps its rows and loses only the filter)
        (void)hipGetLastError();
        filter_drop(h);
        throw;
    }
    h->ivf_filter_valid = true;
}

}  // namespace

extern "C" {

int vdb_ivf_filter_set(vdb_handle hh, const uint32_t *words_host, int64_t nbits) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_filter_set_check(h, "vdb_ivf_filter_set", words_host, nbits);
        set_device(h->device);
        hipStream_t st = nullptr;
        DevBuf up;                             // the caller's words (freed when the call returns: the install has synchronised)
        const size_t bytes = (size_t)filter_words_in(nbits) * sizeof(uint32_t);
        up.reserve_exact(bytes);
        VDB_HIP(hipMemcpyAsync(up.p, words_host, bytes, hipMemcpyHostToDevice, st));
        ivf_filter_install(h, up.as<uint32_t>(), st);
    });
}

int vdb_ivf_filter_set_device(vdb_handle hh, const uint32_t *words_dev, int64_t nbits, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_filter_set_check(h, "vdb_ivf_filter_set_device", words_dev, nbits);
        set_device(h->device);
        ivf_filter_install(h, words_dev, as_stream(stream));
    });
}

int vdb_ivf_filter_count(vdb_handle hh, int64_t *n_allowed) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_filter_admit(h, "vdb_ivf_filter_count");
        ivf_filter_require(h, "vdb_ivf_filter_count");
        if (!n_allowed) throw Error(VDB_ERR_INVALID, "null pointer");
        *n_allowed = h->ivf_filter_count;
    });
}

int vdb_ivf_search_filtered(vdb_handle hh, const float *q_host, int64_t nq, int k, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_filter_search_check(h, "vdb_ivf_search_filtered", q_host, nq, k, D, I);
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            ivf_search_device_impl(h, dq, nq, k, dD, dI, nullptr, nullptr, st, true);
        });
    });
}

int vdb_ivf_search_filtered_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        ivf_filter_search_check(h, "vdb_ivf_search_filtered_device", q_dev, nq, k, D_dev, I_dev);
        set_device(h->device);
        ivf_search_device_impl(h, q_dev, nq, k, D_dev, I_dev, nullptr, nullptr, as_stream(stream), true);
    });
}

}  // extern "C"

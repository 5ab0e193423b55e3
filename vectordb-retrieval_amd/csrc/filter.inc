// filter.inc -- host side of the filtered k-NN search (kernels: filter.hpp; rules: filter_plan.hpp): vdb_filter_set / _clear /
// _count, vdb_search_filtered and the device variants.  Included by vdbhip.hip; the installed filter lives in vdb_index_s
// (filter, filter_*).  The masked scan route is search_batch itself (search_flat.inc) with `filtered` set.

namespace {

// the kinds that keep float32 rows (or their int8 row copy) in insertion order on one device: those of the range search
constexpr unsigned kFilterCalls = kFlat | kLsh | kLsht | kKnng;

void filter_admit(vdb_index_s *h, const char *what) {
    admit(h, what, kFilterCalls);
    if (h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + " is not available with option 'graph'");
}

void filter_require(vdb_index_s *h, const char *what) {
    if (h->filter_valid && h->filter_kind != kind_of(h)) filter_drop(h);       // (the handle became another kind since the install)
    if (!h->filter_valid)
        throw Error(VDB_ERR_STATE, std::string(what) + ": no filter on this handle (none installed, or an add, a reset, an option change "
                                                       "or a change of kind dropped it): call vdb_filter_set first");
}

// words_dev: filter_words_in(N) words in device memory.  One stream synchronisation: the admitted count comes back.
void filter_install(vdb_index_s *h, const uint32_t *words_dev, hipStream_t st) {
    FilterBufs &fb = h->filter;
    const int64_t N = h->N, Npad = h->Npad;
    const bool has_bias = h->scan_ok && h->scan.bias.p != nullptr;
    const bool has_bias8 = has_bias && h->i8_ok && h->scan.bias8.p != nullptr;
    h->filter_valid = h->filter_has_list = false;
    try {
        fb.words.reserve_exact((size_t)filter_words(Npad) * sizeof(uint32_t));
        fb.count.reserve_exact(sizeof(unsigned long long));
        if (has_bias) fb.bias_f.reserve_exact((size_t)Npad * sizeof(float));
        else fb.bias_f.release();
        if (has_bias8) fb.bias8_f.reserve_exact((size_t)2 * Npad * sizeof(int32_t));
        else fb.bias8_f.release();
        VDB_HIP(hipMemsetAsync(fb.count.p, 0, sizeof(unsigned long long), st));
        FilterInstallArgs ia{};
        ia.words_in = words_dev;
        ia.N = N;
        ia.Npad = Npad;
        ia.W_in = filter_words_in(N);
        ia.words = fb.words.as<uint32_t>();
        ia.bias = has_bias ? h->scan.bias.as<float>() : nullptr;
        ia.bias_f = fb.bias_f.as<float>();
        ia.bias8 = has_bias8 ? h->scan.bias8.as<int32_t>() : nullptr;
        ia.bias8_f = fb.bias8_f.as<int32_t>();
        ia.count = fb.count.as<unsigned long long>();
        filter_install_kernel<<<dim3((unsigned)((Npad / 4 + 255) / 256)), dim3(256), 0, st>>>(ia);
        VDB_HIP(hipGetLastError());
        unsigned long long n = 0;
        VDB_HIP(hipMemcpyAsync(&n, fb.count.p, sizeof(n), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        if ((int64_t)n > N) throw Error(VDB_ERR_HIP, "internal: the filter admits more rows than the index holds");
        h->filter_count = (int64_t)n;
        if (filter_keeps_list(h->filter_count, h->opt.filter_sparse_pairs)) {
            FilterListArgs la{};
            la.words = fb.words.as<uint32_t>();
            la.W = filter_words(Npad);
            la.S = (int)filter_segments(Npad);
            fb.seg.reserve_exact((size_t)la.S * sizeof(int));
            fb.list.reserve_exact((size_t)std::max<int64_t>(h->filter_count, 4) * sizeof(int32_t));
            la.seg = fb.seg.as<int>();
            la.list = fb.list.as<int32_t>();
            const unsigned seg_blocks = (unsigned)((la.S + 3) / 4);
            filter_seg_count_kernel<<<dim3(seg_blocks), dim3(256), 0, st>>>(la);
            filter_seg_prefix_kernel<<<dim3(1), dim3(256), 0, st>>>(la);
            filter_emit_kernel<<<dim3(seg_blocks), dim3(256), 0, st>>>(la);
            VDB_HIP(hipGetLastError());
            h->filter_has_list = true;
        } else {
            fb.seg.release();
            fb.list.release();
        }
    } catch (...) {                    // (a failed allocation: the handle keeps its rows and loses only the filter)
        (void)hipGetLastError();
        filter_drop(h);
        throw;
    }
    h->filter_kind = kind_of(h);
    h->filter_valid = true;
}

void filter_set_check(vdb_index_s *h, const char *what, const void *words, int64_t nbits) {
    filter_admit(h, what);
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (!words) throw Error(VDB_ERR_INVALID, "null pointer");
    if (nbits != h->N)
        throw Error(VDB_ERR_INVALID, std::string(what) + ": a filter has one bit per row: nbits must equal ntotal = " + std::to_string(h->N) +
                                         ", got " + std::to_string(nbits));
}

void filter_search_check(vdb_index_s *h, const char *what, const void *q, int64_t nq, int k, const void *D, const void *I) {
    filter_admit(h, what);
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    filter_require(h, what);
    if (nq <= 0) throw Error(VDB_ERR_INVALID, "the query count must be positive");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (!q || !D || !I) throw Error(VDB_ERR_INVALID, "null pointer");
}

template <int QB>
void launch_filter_rows(const FilterRowsArgs &a, int64_t units, hipStream_t st) {
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 3) / 4, 8192)));
    const int kpl = kpl_for(a.c.k);
    if (QB > 1) {                      // (k <= 128, filter_rows_blocked)
        if (kpl == 1) filter_rows_kernel<1, QB><<<grid, dim3(256), 0, st>>>(a);
        else filter_rows_kernel<2, QB><<<grid, dim3(256), 0, st>>>(a);
    } else {
        DISPATCH_KPL(kpl, (filter_rows_kernel<KPL, 1><<<grid, dim3(256), 0, st>>>(a)));
    }
    VDB_HIP(hipGetLastError());
}

// the sparse route: the listed rows alone, split over S waves per query (group), merged by merge_kernel
void filter_rows_search(vdb_index_s *h, const float *dq, int64_t nq, int k, float *D, int64_t *I, hipStream_t st) {
    Workspace &ws = h->ws;
    const float *qpad = dq;
    if (h->D4 != h->dim) {
        ws.qpad.reserve((size_t)nq * h->D4 * sizeof(float));
        pad_rows_kernel<<<dim3((unsigned)((nq * h->D4 + 255) / 256)), dim3(256), 0, st>>>(dq, nq, h->dim, h->D4, ws.qpad.as<float>());
        VDB_HIP(hipGetLastError());
        qpad = ws.qpad.as<float>();
    }
    const bool blocked = filter_rows_blocked(nq, k);
    FilterRowsArgs a{};
    a.c = flat_rows(h, qpad, k);
    a.list = h->filter.list.as<int32_t>();
    a.n = h->filter_count;
    a.nq = nq;
    a.S = filter_rows_splits(nq, k, a.n);
    a.per_split = filter_rows_per_split(a.n, a.S);
    const int64_t groups = blocked ? (nq + kFilterRowsQB - 1) / kFilterRowsQB : nq;
    const long tslot = timing_begin(h, st);
    timing_mark(h, tslot, 0, st);
    if (a.S == 1) {
        a.D = D;
        a.I = I;
    } else {
        ws.pkeys.reserve((size_t)nq * a.S * k * sizeof(double));
        ws.pids.reserve((size_t)nq * a.S * k * sizeof(int64_t));
        a.pkeys = ws.pkeys.as<double>();
        a.pids = ws.pids.as<int64_t>();
    }
    if (blocked) launch_filter_rows<kFilterRowsQB>(a, groups * a.S, st);
    else launch_filter_rows<1>(a, groups * a.S, st);
    timing_mark(h, tslot, 1, st);
    if (a.S > 1) {
        MergeArgs ma{};
        ma.pkeys = a.pkeys; ma.pids = a.pids;
        ma.part_stride = k; ma.slot_stride = (int64_t)a.S * k; ma.nparts = a.S;
        ma.k = k; ma.metric = h->metric;
        ma.count = nq;
        ma.D = D; ma.I = I;
        launch_merge(ma, nq, st);
    }
    timing_mark(h, tslot, 2, st);
    h->last.last_path = VDB_PATH_FILTER_ROWS;
    h->last.last_nq = nq;
    h->filter_cand = nq * h->filter_count;
}

void filtered_search_impl(vdb_index_s *h, const float *dq, int64_t nq, int k, float *D, int64_t *I, hipStream_t st) {
    if (h->filter_has_list && filter_route_sparse(nq, k, h->filter_count, h->opt.filter_sparse_pairs, h->opt.force_path))
        filter_rows_search(h, dq, nq, k, D, I, st);
    else
        search_device_impl(h, dq, nq, k, D, I, nullptr, nullptr, st, true);
}

}  // namespace

extern "C" {

int vdb_filter_set(vdb_handle hh, const uint32_t *words_host, int64_t nbits) {
    return guarded([&] {
        auto *h = check(hh);
        filter_set_check(h, "vdb_filter_set", words_host, nbits);
        set_device(h->device);
        hipStream_t st = nullptr;
        DevBuf up;                             // the caller's words (freed when the call returns: the install has synchronised)
        const size_t bytes = (size_t)filter_words_in(nbits) * sizeof(uint32_t);
        up.reserve_exact(bytes);
        VDB_HIP(hipMemcpyAsync(up.p, words_host, bytes, hipMemcpyHostToDevice, st));
        filter_install(h, up.as<uint32_t>(), st);
    });
}

int vdb_filter_set_device(vdb_handle hh, const uint32_t *words_dev, int64_t nbits, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        filter_set_check(h, "vdb_filter_set_device", words_dev, nbits);
        set_device(h->device);
        filter_install(h, words_dev, as_stream(stream));
    });
}

int vdb_filter_clear(vdb_handle hh) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_filter_clear", kAnyKind & ~kMulti);      // (a handle that changed kind since the install may still hold the buffers)
        filter_drop(h);
    });
}

int vdb_filter_count(vdb_handle hh, int64_t *n_allowed) {
    return guarded([&] {
        auto *h = check(hh);
        filter_admit(h, "vdb_filter_count");
        filter_require(h, "vdb_filter_count");
        if (!n_allowed) throw Error(VDB_ERR_INVALID, "null pointer");
        *n_allowed = h->filter_count;
    });
}

int vdb_search_filtered(vdb_handle hh, const float *q_host, int64_t nq, int k, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        filter_search_check(h, "vdb_search_filtered", q_host, nq, k, D, I);
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            filtered_search_impl(h, dq, nq, k, dD, dI, st);
        });
    });
}

int vdb_search_filtered_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        filter_search_check(h, "vdb_search_filtered_device", q_dev, nq, k, D_dev, I_dev);
        set_device(h->device);
        filtered_search_impl(h, q_dev, nq, k, D_dev, I_dev, as_stream(stream));
    });
}

}  // extern "C"

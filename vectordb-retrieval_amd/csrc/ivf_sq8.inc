// ivf_sq8.inc -- host side of IVF<nlist>,SQ8 (kernels: ivf_sq8.hpp).  Included by ivf.inc inside its anonymous namespace.
//
// An SQ8 handle (vdb_ivf_set_codec(h, 1) on an empty single-device handle) keeps NO float32 rows and no fp16 / int8 scan
// copies: the codes [N][D4] in list order, the list of every list-order row, the int64 ids, and the centroids and
// {vmin, vdiff} zero padded to D4, and (D <= 128) the panel-space bias and scales.  Every row is scored as its decoded x^
// (refine.hpp, sq8_key); D <= 128 batches take the list-major MFMA scan on fp16 panels converted from the codes per search
// (ivf_search_lists), D > 128 and small batches the exact list scan -- the result is the IVF-Flat result over x^ either way.

constexpr int64_t kSq8TrainRows = 100000;      // rows the range training reads at most (evenly spaced beyond that)

inline bool sq8(const vdb_index_s *h) { return h->ivf_codec == 1; }

Sq8Rows sq8_rows(const vdb_index_s *h) {
    return Sq8Rows{h->codes.sq8_codes.as<unsigned char>(), h->codes.sq8_list.as<int32_t>(), h->kept.sq8_cent.as<float>(),
                   h->kept.sq8_param.as<float>(), h->kept.sq8_param.as<float>() + h->D4};
}

// the installed centroids, zero padded to D4 (host)
std::vector<float> sq8_padded_centroids(const vdb_index_s *h) {
    std::vector<float> c((size_t)h->nlist * h->D4, 0.f);
    for (int l = 0; l < h->nlist; ++l)
        memcpy(&c[(size_t)l * h->D4], &h->ivf_centroids[(size_t)l * h->dim], (size_t)h->dim * sizeof(float));
    return c;
}

// centroids and {vmin, vdiff} of the handle on the device (before every encode)
void sq8_upload_params(vdb_index_s *h) {
    const int Dm = h->dim, D4 = h->D4;
    const std::vector<float> c = sq8_padded_centroids(h);
    std::vector<float> p((size_t)2 * D4, 0.f);
    memcpy(&p[0], h->sq8_vmin.data(), (size_t)Dm * sizeof(float));
    memcpy(&p[(size_t)D4], h->sq8_vdiff.data(), (size_t)Dm * sizeof(float));
    h->kept.sq8_cent.reserve(c.size() * sizeof(float));
    h->kept.sq8_param.reserve(p.size() * sizeof(float));
    VDB_HIP(hipMemcpy(h->kept.sq8_cent.p, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(h->kept.sq8_param.p, p.data(), p.size() * sizeof(float), hipMemcpyHostToDevice));
}

// the coarse quantizer's workspace of a build-time assignment pass (one k = 1 search of every row) is given back: an SQ8
// index is chosen for its footprint, and the next search sizes that workspace for its own batch
void sq8_release_coarse_ws(vdb_index_s *h) {
    group_release(h->coarse->ws);
    h->coarse->info_valid_nq = -1;
}

// vmin / vdiff from the residuals of x_host [n][dim] against the installed centroids: every row when n <= kSq8TrainRows,
// else the rows floor(i * n / kSq8TrainRows), i = 0 .. kSq8TrainRows - 1 (deterministic)
void sq8_train_ranges(vdb_index_s *h, const float *x_host, int64_t n) {
    const int Dm = h->dim, D4 = h->D4;
    const int64_t ns = std::min<int64_t>(n, kSq8TrainRows);
    std::vector<float> sample;
    const float *rows = x_host;
    if (ns < n) {
        sample.resize((size_t)ns * Dm);
        for (int64_t i = 0; i < ns; ++i)
            memcpy(&sample[(size_t)i * Dm], x_host + (size_t)((i * n) / ns) * Dm, (size_t)Dm * sizeof(float));
        rows = sample.data();
    }
    DevBuf dx, dassign, dcent, pmin, pmax;
    dx.reserve((size_t)ns * Dm * sizeof(float));
    VDB_HIP(hipMemcpy(dx.p, rows, (size_t)ns * Dm * sizeof(float), hipMemcpyHostToDevice));
    ivf_assign_rows(h, dx.as<float>(), ns, dassign);
    const std::vector<float> c = sq8_padded_centroids(h);
    dcent.reserve(c.size() * sizeof(float));
    VDB_HIP(hipMemcpy(dcent.p, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
    const int chunks = (int)std::min<int64_t>(kSq8RangeChunks, ns);
    pmin.reserve((size_t)chunks * Dm * sizeof(float));
    pmax.reserve((size_t)chunks * Dm * sizeof(float));
    sq8_range_kernel<<<dim3((unsigned)((Dm + 63) / 64), (unsigned)chunks), dim3(256), 0, nullptr>>>(
        dx.as<float>(), ns, Dm, D4, dcent.as<float>(), dassign.as<int64_t>(), pmin.as<float>(), pmax.as<float>());
    VDB_HIP(hipGetLastError());
    std::vector<float> lo((size_t)chunks * Dm), hi((size_t)chunks * Dm);
    VDB_HIP(hipMemcpy(lo.data(), pmin.p, lo.size() * sizeof(float), hipMemcpyDeviceToHost));
    VDB_HIP(hipMemcpy(hi.data(), pmax.p, hi.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> vmin((size_t)Dm), vdiff((size_t)Dm);
    for (int d = 0; d < Dm; ++d) {
        float a = lo[(size_t)d], b = hi[(size_t)d];
        for (int j = 1; j < chunks; ++j) {
            a = std::min(a, lo[(size_t)j * Dm + d]);
            b = std::max(b, hi[(size_t)j * Dm + d]);
        }
        ivf_require(std::isfinite(a) && std::isfinite(b), VDB_ERR_INVALID, "SQ8 ranges: the training rows are not finite");
        vmin[(size_t)d] = a;
        vdiff[(size_t)d] = b - a;
    }
    sq8_release_coarse_ws(h);
    h->sq8_vmin = vmin;
    h->sq8_vdiff = vdiff;
    h->sq8_ranges = true;
}

void ivf_build_panel_space(vdb_index_s *h);     // (ivf.inc)

// The panel space of an SQ8 index (D <= 128): spans, bias (||x^||^2), scale and fp16-exactness flag exactly as
// ivf_build_panel_space derives them for an IVF-Flat index over the float32 rows x^ -- from a decoded copy that lives only
// for this call, and is freed again together with the fp16 panels (a search converts those from the codes itself).
void sq8_build_panel_space(vdb_index_s *h) {
    h->ivf_mfma_ok = false;
    if (h->N == 0 || h->ksteps > kMaxKSteps) return;      // D > 128: the exact list scan serves every batch
    const size_t bytes = (size_t)h->N * h->D4 * sizeof(float);
    h->rows.x32.reserve_exact(bytes);
    try {
        VDB_HIP(hipMemset(h->rows.x32.p, 0, bytes));
        sq8_decode_rows_kernel<<<dim3((unsigned)std::min<int64_t>((h->N * h->dim + 255) / 256, 1 << 20)), dim3(256), 0, nullptr>>>(
            sq8_rows(h), h->N, h->dim, h->D4, h->D4, h->rows.x32.as<float>());
        VDB_HIP(hipGetLastError());
        ivf_build_panel_space(h);
        VDB_HIP(hipDeviceSynchronize());
    } catch (...) {
        h->rows.x32.release();
        h->scan.panels.release();
        h->ivf_mfma_ok = false;
        throw;
    }
    h->rows.x32.release();
    h->scan.panels.release();
    h->rows.xnorm2.release();                                  // (the norms only fed the bias)
}

// vdb_ivf_add(_assigned) on an SQ8 handle: the same lists as ivf_add_impl (ivf_add_lists), but the new rows are encoded as
// soon as they are on the device and only their codes are kept
void sq8_add(vdb_index_s *h, const float *x_host, int64_t n, int64_t id_base, const int32_t *given) {
    ivf_require(h->nlist > 0 && h->coarse, VDB_ERR_STATE, "no centroids: train or set them first");
    ivf_require(h->sq8_ranges, VDB_ERR_STATE, "no SQ8 ranges: train the index or set them first");
    ivf_require(n >= 0 && (n == 0 || x_host), VDB_ERR_INVALID, "bad corpus");
    int64_t N0, N1;
    if (!ivf_add_range(h, n, id_base, N0, N1)) return;
    ivf_check_given(h, given, n);
    set_device(h->device);
    const int Dm = h->dim, D4 = h->D4;
    VDB_HIP(hipDeviceSynchronize());
    h->ivf_built = false;
    h->built = false;
    sq8_upload_params(h);
    std::vector<int64_t> assign_new((size_t)n);
    if (N1 > 0) {
        DevBuf fresh, dnew, src_codes, src_ids, dperm, doff;
        src_codes.reserve((size_t)N1 * D4);
        if (N0) VDB_HIP(hipMemcpy(src_codes.p, h->codes.sq8_codes.p, (size_t)N0 * D4, hipMemcpyDeviceToDevice));
        if (n > 0) {
            // the new rows through the pinned staging blocks, then their lists, then their codes (the float32 rows live
            // only for the duration of this call)
            fresh.reserve((size_t)n * D4 * sizeof(float));
            if (D4 != Dm) VDB_HIP(hipMemset(fresh.p, 0, (size_t)n * D4 * sizeof(float)));
            upload_rows(h, fresh.as<float>(), D4, x_host, n, Dm, nullptr);
            dnew.reserve((size_t)n * sizeof(int64_t));
            if (given) {
                for (int64_t i = 0; i < n; ++i) assign_new[(size_t)i] = given[i];
                VDB_HIP(hipMemcpy(dnew.p, assign_new.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
            } else {
                ivf_add_assign(h, fresh.as<float>(), n, dnew, assign_new);
                sq8_release_coarse_ws(h);
            }
            sq8_encode_kernel<<<dim3((unsigned)std::min<int64_t>((n * D4 + 255) / 256, 1 << 20)), dim3(256), 0, nullptr>>>(
                fresh.as<float>(), n, D4, h->kept.sq8_cent.as<float>(), dnew.as<int64_t>(), h->kept.sq8_param.as<float>(),
                h->kept.sq8_param.as<float>() + D4, src_codes.as<unsigned char>() + (size_t)N0 * D4);
            VDB_HIP(hipGetLastError());
            VDB_HIP(hipDeviceSynchronize());
            fresh.release();
            dnew.release();
        }
        ivf_add_lists(h, assign_new, N0, src_ids, dperm, doff);
        h->codes.sq8_codes.reserve((size_t)N1 * D4);
        h->lists.ivf_ids.reserve((size_t)N1 * 8);
        const int64_t total = N1 * (D4 / 4);
        sq8_gather_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr>>>(
            src_codes.as<unsigned char>(), dperm.as<int32_t>(), N1, D4, id_base, N0 ? src_ids.as<int64_t>() : nullptr,
            h->codes.sq8_codes.as<unsigned char>(), h->lists.ivf_ids.as<int64_t>());
        VDB_HIP(hipGetLastError());
        std::vector<int32_t> list_of((size_t)N1);       // list of every list-order row (the accessor's centroid)
        for (int l = 0; l < h->nlist; ++l)
            std::fill(list_of.begin() + h->ivf_offsets_host[(size_t)l], list_of.begin() + h->ivf_offsets_host[(size_t)l + 1], l);
        h->codes.sq8_list.reserve((size_t)N1 * 4);
        VDB_HIP(hipMemcpy(h->codes.sq8_list.p, list_of.data(), (size_t)N1 * 4, hipMemcpyHostToDevice));
        VDB_HIP(hipDeviceSynchronize());
    }
    ivf_add_finish(h, assign_new, N0, id_base);
    sq8_build_panel_space(h);
    h->ivf_built = true;
}

// ivf_sq8.inc -- host side of IVF<nlist>,SQ8 (kernels: ivf_sq8.hpp).  Included by ivf.inc inside its anonymous namespace.
//
// An SQ8 handle (vdb_ivf_set_codec(h, 1) on an empty single-device handle) keeps NO float32 rows and no fp16 / int8 scan
// copies: the codes [N][D4] in list order, the list of every list-order row, the int64 ids, and the centroids and
// {vmin, vdiff} zero padded to D4, and (D <= 128) the panel-space bias and scales.  Every row is scored as its decoded x^
// (refine.hpp, sq8_key); D <= 128 batches take the list-major MFMA scan on fp16 panels converted from the codes per search
// (ivf_search_lists), D > 128 and small batches the exact list scan -- the result is the IVF-Flat result over x^ either way.
// Option "ivf_sq8_kloop": D > 128 keeps span tables and the panel-space bias too and scans the codes themselves (sq8k_build_space).

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
int64_t ivf_build_spans(vdb_index_s *h, int span_rows);

// What the direct scan (option "ivf_sq8_direct", ivf_sq8_scan.hpp) reads of the centroids and ranges, in float64 on the host: with
// g = vdiff / 255 and e = vmin + 128.5 g -- max g; max |c_l[d]| + max |e[d]| (the window of the slot term); the norm of the per-dimension
// rounding bound of sq8_decode, |c|max[d] + 2 |vmin[d]| + 4.2 vdiff[d]; max_l ||c_l + e||.  ok: all of it finite
void sq8d_constants(vdb_index_s *h) {
    const int Dm = h->dim;
    std::vector<double> cmax((size_t)Dm, 0.0), e((size_t)Dm);
    double gmax = 0.0, emax = 0.0, camax = 0.0, can2 = 0.0, dec2 = 0.0;
    for (int d = 0; d < Dm; ++d) {
        const double g = (double)h->sq8_vdiff[(size_t)d] / 255.0;
        e[(size_t)d] = (double)h->sq8_vmin[(size_t)d] + 128.5 * g;
        gmax = std::max(gmax, g);
        emax = std::max(emax, std::fabs(e[(size_t)d]));
    }
    for (int l = 0; l < h->nlist; ++l) {
        double n2 = 0.0;
        for (int d = 0; d < Dm; ++d) {
            const double c = (double)h->ivf_centroids[(size_t)l * Dm + d];
            cmax[(size_t)d] = std::max(cmax[(size_t)d], std::fabs(c));
            n2 += (c + e[(size_t)d]) * (c + e[(size_t)d]);
        }
        can2 = std::max(can2, n2);
    }
    for (int d = 0; d < Dm; ++d) {
        const double t = cmax[(size_t)d] + 2.0 * std::fabs((double)h->sq8_vmin[(size_t)d]) + 4.2 * (double)h->sq8_vdiff[(size_t)d];
        camax = std::max(camax, cmax[(size_t)d]);
        dec2 += t * t;
    }
    vdb_index_s::Sq8Direct k;
    k.gmax = gmax > 0.0 ? std::nextafter((float)gmax, INFINITY) : 0.f;      // (rounded up: the scale window must hold for every w)
    k.camax = std::nextafter((float)(camax + emax), INFINITY);
    k.dec_norm = std::sqrt(dec2) * 1.000001;
    k.can = std::sqrt(can2) * 1.000001;
    k.ok = std::isfinite(k.gmax) && std::isfinite(k.camax) && std::isfinite(k.dec_norm) && std::isfinite(k.can);
    h->sq8d = k;
}

// The panel space of an SQ8 index (D <= 128): spans, bias (||x^||^2), scale and fp16-exactness flag exactly as
// ivf_build_panel_space derives them for an IVF-Flat index over the float32 rows x^ -- from a decoded copy that lives only
// for this call, and is freed again together with the fp16 panels (a search converts those from the codes itself).
// D > 128, option "ivf_sq8_kloop": what the K-loop scan of the codes (ivf_sq8_kloop.hpp) needs of the panel space, without any panels --
// the span tables, the accumulator inits (||x^||^2 per list-padded row, kPadBias on padding rows: 4 bytes per padded row) and maxnorm2.
// The norms come from the codes in blocks of rows: a block is decoded into a scratch buffer and read by the norm pass of index_stats
// (corpus_stats_kernel: one float64 chain per row, rounded once), so the bias is the one an IVF-Flat index over x^ holds -- and the
// float32 rows of the whole index (38 GB at 12.5M x 768) never exist.
constexpr size_t kSq8kNormBlockBytes = (size_t)128 << 20;
void sq8k_build_space(vdb_index_s *h) {
    hipStream_t st = nullptr;
    const int64_t N = h->N;
    const int D4 = h->D4;
    h->ivf_tps = ivf_tps_of(h->opt, N, h->nlist);
    const int span_rows = h->ivf_tps * 16;
    const int64_t P = ivf_build_spans(h, span_rows);
    if (P == 0) return;
    DevBuf block;
    const int64_t block_rows = std::max<int64_t>(1024, (int64_t)(kSq8kNormBlockBytes / ((size_t)D4 * sizeof(float))));
    block.reserve((size_t)std::min(N, block_rows) * D4 * sizeof(float));
    h->rows.xnorm2.reserve((size_t)N * sizeof(float));
    h->kept.stats.reserve(sizeof(IndexStats));
    try {
        VDB_HIP(hipMemsetAsync(h->kept.stats.p, 0, sizeof(IndexStats), st));
        VDB_HIP(hipMemsetAsync(block.p, 0, (size_t)std::min(N, block_rows) * D4 * sizeof(float), st));     // (the padding columns stay 0)
        const Sq8Rows all = sq8_rows(h);
        for (int64_t r0 = 0; r0 < N; r0 += block_rows) {
            const int64_t nb = std::min(block_rows, N - r0);
            const Sq8Rows part{all.codes + (size_t)r0 * D4, all.list + r0, all.cent, all.vmin, all.vdiff};
            sq8_decode_rows_kernel<<<dim3((unsigned)std::min<int64_t>((nb * h->dim + 255) / 256, 1 << 20)), dim3(256), 0, st>>>(
                part, nb, h->dim, D4, D4, block.as<float>());
            corpus_stats_kernel<<<dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st>>>(block.as<float>(), nb, D4, h->rows.xnorm2.as<float>() + r0,
                                                                                         h->kept.stats.as<IndexStats>());
            VDB_HIP(hipGetLastError());
        }
        IndexStats hs;
        VDB_HIP(hipMemcpyAsync(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        memcpy(&h->absmax, &hs.absmax_bits, 4);
        memcpy(&h->maxnorm2, &hs.maxnorm2_bits, 4);
        h->nonfinite = hs.nonfinite != 0;
        if (!h->nonfinite) {
            h->scan.bias.reserve((size_t)P * span_rows * sizeof(float));
            ivf_build_bias_kernel<<<dim3((unsigned)((P * span_rows + 255) / 256)), dim3(256), 0, st>>>(
                h->rows.xnorm2.as<float>(), P, span_rows, h->metric, h->lists.ivf_span_row0.as<int32_t>(), h->lists.ivf_span_valid.as<int32_t>(),
                h->scan.bias.as<float>());
            VDB_HIP(hipGetLastError());
            VDB_HIP(hipStreamSynchronize(st));
        }
    } catch (...) {
        h->rows.xnorm2.release();
        h->scan.bias.release();
        throw;
    }
    h->rows.xnorm2.release();                                  // (the norms only fed the bias)
    h->sq8k_ok = !h->nonfinite;
    h->tile16 = h->sq8k_ok;                                    // (the plan's K-loop geometry: ivf_shape_of)
    h->ivf_mfma_ok = h->sq8k_ok;
}

void sq8_build_panel_space(vdb_index_s *h) {
    h->ivf_mfma_ok = false;
    if (h->sq8k_ok) {         // (the bookkeeping of the last add goes with its lists; the rule below decides anew)
        h->scan.bias.release();
        h->sq8k_ok = false;
        h->tile16 = false;
    }
    if (h->N == 0) return;
    if (h->ksteps > kMaxKSteps) {     // D > 128: the exact list scan serves every batch, unless option "ivf_sq8_kloop" is set
        if (ivf_sq8k_builds(h->opt.ivf_sq8_kloop, h->ivf_codec, h->ksteps, h->dim)) sq8k_build_space(h);
        return;
    }
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
    sq8d_constants(h);
    h->ivf_built = true;
}

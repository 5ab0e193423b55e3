// ivf_pq.inc -- host side of IVF<nlist>,PQ<M> (kernels: ivf_pq.hpp).  Included by ivf.inc inside its anonymous namespace.
//
// An IVF-PQ handle (vdb_ivf_set_codec(h, 2) on an empty single-device handle) keeps NO float32 rows and no fp16 / int8 scan
// copies: the codes [N][M] in list order, the list of every list-order row, the int64 ids, the centroids zero padded to D4,
// the codebooks of the residuals, and (D <= 128) the panel-space bias and scales.  Every row is scored as its decoded x^
// (refine.hpp, ivfpq_key); D <= 128 batches take the list-major MFMA scan on fp16 panels made from the codes per batch
// (ivf_search_lists), D > 128 and small batches the exact list scan -- the result is the IVF-Flat result over x^ either way.
// The buffers shared with the SQ8 codec (the list of every row, the padded centroids, the per-batch panels) are the same
// members: a handle has one codec for life.

inline bool ivfpq(const vdb_index_s *h) { return h->ivf_codec == 2; }

IvfPqRows ivfpq_rows(const vdb_index_s *h) {
    IvfPqRows p;
    p.pq.codes = h->codes.ivfpq_codes.as<unsigned char>();
    p.list = h->codes.sq8_list.as<int32_t>();
    p.cent = h->kept.sq8_cent.as<float>();
    p.pq.cb = h->kept.ivfpq_cb.as<float>();
    p.pq.M = h->ivfpq.M;
    p.pq.dsub = h->ivfpq.dsub;
    return p;
}

// pq_install_codebooks (pq.inc) on the codebooks of the residuals; refused ones leave the index as it was
void ivfpq_install_codebooks(vdb_index_s *h, int M, const float *cb_host) {
    VDB_HIP(hipDeviceSynchronize());
    pq_install_codebooks(h, h->ivfpq, h->kept.ivfpq_cb, M, cb_host);
    h->ivf_built = false;                      // (rows encoded under the old codebooks are dropped by the next add)
}

// the installed centroids, zero padded, on the device (before every add: vdb_ivf_set_centroids may have replaced them)
void ivfpq_upload_centroids(vdb_index_s *h) {
    const std::vector<float> c = sq8_padded_centroids(h);
    h->kept.sq8_cent.reserve(c.size() * sizeof(float));
    VDB_HIP(hipMemcpy(h->kept.sq8_cent.p, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
}

// x^ of the first n list-order rows: float32, `pitch` floats per row (zero beyond dim)
void ivfpq_decode_rows(vdb_index_s *h, int64_t n, int64_t pitch, float *out, hipStream_t st) {
    if (n <= 0) return;
    pq_decode_rows_kernel<true><<<dim3((unsigned)std::min<int64_t>((n * pitch + 255) / 256, 1 << 16)), dim3(256), 0, st>>>(
        ivfpq_rows(h), n, h->dim, h->D4, pitch, out);
    VDB_HIP(hipGetLastError());
}

// The panel space of an IVF-PQ index (D <= 128), as sq8_build_panel_space derives it: spans, bias (||x^||^2), scale and
// fp16-exactness flag of an IVF-Flat index over the float32 rows x^, from a decoded copy that lives only for this call.
void ivfpq_build_panel_space(vdb_index_s *h) {
    h->ivf_mfma_ok = false;
    if (h->N == 0 || h->ksteps > kMaxKSteps) return;      // D > 128: the exact list scan serves every batch
    h->rows.x32.reserve_exact((size_t)h->N * h->D4 * sizeof(float));
    try {
        ivfpq_decode_rows(h, h->N, h->D4, h->rows.x32.as<float>(), nullptr);
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

// vdb_ivf_add(_assigned) and vdb_ivfpq_add_codes on an IVF-PQ handle: the same lists as ivf_add_impl (ivf_add_lists); the new
// rows are encoded as soon as they are on the device (x_host), or arrive as codes (codes_host, with `given`), and only
// codes are kept.  Every argument is checked before the handle is touched: a refused add leaves the index as it was.
void ivfpq_add(vdb_index_s *h, const float *x_host, const uint8_t *codes_host, int64_t n, int64_t id_base, const int32_t *given) {
    ivf_require(h->nlist > 0 && h->coarse, VDB_ERR_STATE, "no centroids: train or set them first");
    ivf_require(h->ivfpq.M > 0, VDB_ERR_STATE, "no IVF-PQ codebooks: call vdb_ivfpq_train or vdb_ivfpq_set_codebooks first");
    ivf_require(n >= 0 && (n == 0 || x_host || codes_host), VDB_ERR_INVALID, "bad corpus");
    int64_t N0, N1;
    if (!ivf_add_range(h, n, id_base, N0, N1)) return;
    ivf_check_given(h, given, n);
    set_device(h->device);
    const int Dm = h->dim, D4 = h->D4, M = h->ivfpq.M;
    VDB_HIP(hipDeviceSynchronize());
    h->ivf_built = false;
    h->built = false;
    ivfpq_upload_centroids(h);
    std::vector<int64_t> assign_new((size_t)n);
    if (N1 > 0) {
        DevBuf fresh, dnew, src_codes, src_ids, dperm, doff;
        src_codes.reserve((size_t)N1 * M);
        if (N0) VDB_HIP(hipMemcpy(src_codes.p, h->codes.ivfpq_codes.p, (size_t)N0 * M, hipMemcpyDeviceToDevice));
        unsigned char *new_codes = src_codes.as<unsigned char>() + (size_t)N0 * M;
        if (n > 0 && codes_host) {
            for (int64_t i = 0; i < n; ++i) assign_new[(size_t)i] = given[i];
            VDB_HIP(hipMemcpy(new_codes, codes_host, (size_t)n * M, hipMemcpyHostToDevice));
        } else if (n > 0) {
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
                for (int64_t i = 0; i < n; ++i)      // (the kernel reads centroid assign[i]: no row without a list reaches it)
                    ivf_require(assign_new[(size_t)i] >= 0 && assign_new[(size_t)i] < h->nlist, VDB_ERR_INVALID, "row could not be assigned to a list");
            }
            pq_launch_encode(fresh.as<float>(), n, D4, h->kept.sq8_cent.as<float>(), dnew.as<int64_t>(), h->kept.ivfpq_cb.as<float>(), M,
                             h->ivfpq.dsub, new_codes, nullptr);
            VDB_HIP(hipDeviceSynchronize());
            fresh.release();
            dnew.release();
        }
        ivf_add_lists(h, assign_new, N0, src_ids, dperm, doff);
        // (exact sizes: the index is chosen for its footprint, and an append gathers into fresh arrays anyway)
        h->codes.ivfpq_codes.reserve_exact((size_t)N1 * M);
        h->lists.ivf_ids.reserve_exact((size_t)N1 * 8);
        ivfpq_gather_kernel<<<dim3((unsigned)std::min<int64_t>((N1 * M + 255) / 256, 1 << 16)), dim3(256), 0, nullptr>>>(
            src_codes.as<unsigned char>(), dperm.as<int32_t>(), N1, M, id_base, N0 ? src_ids.as<int64_t>() : nullptr,
            h->codes.ivfpq_codes.as<unsigned char>(), h->lists.ivf_ids.as<int64_t>());
        VDB_HIP(hipGetLastError());
        std::vector<int32_t> list_of((size_t)N1);       // list of every list-order row (the accessor's centroid)
        for (int l = 0; l < h->nlist; ++l)
            std::fill(list_of.begin() + h->ivf_offsets_host[(size_t)l], list_of.begin() + h->ivf_offsets_host[(size_t)l + 1], l);
        h->codes.sq8_list.reserve_exact((size_t)N1 * 4);
        VDB_HIP(hipMemcpy(h->codes.sq8_list.p, list_of.data(), (size_t)N1 * 4, hipMemcpyHostToDevice));
        VDB_HIP(hipDeviceSynchronize());
    }
    ivf_add_finish(h, assign_new, N0, id_base);
    ivfpq_build_panel_space(h);
    h->ivf_built = true;
}

// The fp16 panels of the whole panel space, made from the codes for this batch (workspace).  LDS of a workgroup: 4 waves x
// (the staged code rows of a tile + its centroid), then the float32 codebooks of one slice of k-steps -- within the 64 KiB a
// kernel gets without opting in, so two workgroups run per CU.  The k-steps are dealt to blockIdx.y in the largest equal
// slices whose sub-spaces fit (D = 128, PQ64: 4 slices of 32 dims, 32 KiB each); a table no slice of which fits (a sub-space
// of more than ~50 dims) is read through the cache.
constexpr int kIvfPqLdsBudget = 64 * 1024;
const half8 *ivf_pq_panels(vdb_index_s *h, hipStream_t st) {
    const int64_t ntiles = h->ivf_pspans * kIvfTilesPerSpan;
    h->ws.sq8_panels.reserve((size_t)ntiles * h->ksteps * 64 * sizeof(half8));
    IvfPqPanelArgs a{};
    a.rows = ivfpq_rows(h);
    a.span_row0 = h->lists.ivf_span_row0.as<int32_t>();
    a.span_valid = h->lists.ivf_span_valid.as<int32_t>();
    a.panels = h->ws.sq8_panels.as<half8>();
    a.ntiles = ntiles;
    a.sx = h->sx;
    a.D = h->dim; a.D4 = h->D4; a.ksteps = h->ksteps;
    const int dsub = h->ivfpq.dsub;
    a.code_pitch = pq_code_pitch(h->ivfpq.M);
    const int fixed = 4 * (((32 * a.code_pitch + 15) & ~15) + kIvfPqCentFloats * (int)sizeof(float));
    bool lds = false;
    a.slice_ks = h->ksteps;
    size_t table_bytes = 0;
    for (int s = h->ksteps; s >= 1 && !lds; s /= 2) {
        int64_t worst = 0;                       // floats of the sub-spaces the widest slice touches
        for (int ks_lo = 0; ks_lo < h->ksteps; ks_lo += s) {
            const int d_lo = std::min(ks_lo * 16, h->dim), d_hi = std::min(h->dim, (ks_lo + s) * 16);
            worst = std::max<int64_t>(worst, (int64_t)((d_hi + dsub - 1) / dsub - d_lo / dsub) * 256 * dsub);
        }
        if (fixed + worst * (int64_t)sizeof(float) <= kIvfPqLdsBudget) {
            lds = true;
            a.slice_ks = s;
            table_bytes = (size_t)worst * sizeof(float);
        }
    }
    const unsigned gy = (unsigned)((h->ksteps + a.slice_ks - 1) / a.slice_ks);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ntiles + 3) / 4, (int64_t)2 * h->n_cus));
    if (lds) ivf_pq_panels_kernel<true><<<dim3(gx, gy), dim3(256), (size_t)fixed + table_bytes, st>>>(a);
    else ivf_pq_panels_kernel<false><<<dim3(gx, gy), dim3(256), (size_t)fixed, st>>>(a);
    VDB_HIP(hipGetLastError());
    return a.panels;
}

// ivf_pq.inc -- host side of IVF<nlist>,PQ<M> (kernels: ivf_pq.hpp).  Included by ivf.inc inside its anonymous namespace.
//
// An IVF-PQ handle (vdb_ivf_set_codec(h, 2) on an empty single-device handle) keeps NO float32 rows and no fp16 / int8 scan
// copies: the codes [N][M] in list order, the list of every list-order row, the int64 ids, the centroids zero padded to D4,
// the codebooks of the residuals, and (D <= 128) the panel-space bias and scales.  Every row is scored as its decoded x^
// (refine.hpp, ivfpq_key); D <= 128 batches take the list-major MFMA scan on fp16 panels made from the codes per batch
// (ivf_search_lists), D > 128 and small batches the exact list scan, and with option "ivfpq_adc_max_batch" small batches of any D the
// lookup-table (ADC) scan of the probed lists (ivf_pq_adc.hpp, the end of this file) -- the result is the IVF-Flat result over x^ every way.
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
    h->codes.ivfpq_n2.release();               // (the norms of the ADC scan: ivfpq_adc_prepare)
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
    h->codes.ivfpq_n2.release();               // (the norms of the ADC scan: the next admitted batch makes them anew)
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

// ---- the ADC scan of the probed lists (ivf_pq_adc.hpp; option "ivfpq_adc_max_batch") -----------------------------------------------
// What the scan keeps per handle, made by the first batch that asks after an add (never without the option): the float32 norms of
// the decoded rows (codes.ivfpq_n2, 4 N bytes: held = valid -- an add, new centroids and new codebooks release it, vdb_reset frees
// it with the codes) and the three magnitudes of the bound.  Usable: Xn^2 and (Cn + Rn)^2 within [1e-30, 1e30].
void ivfpq_adc_drop(vdb_index_s *h) {
    h->codes.ivfpq_n2.release();
    h->ivfpq_adc_ok = false;
}

bool ivfpq_adc_prepare(vdb_index_s *h, hipStream_t st) {
    if (h->codes.ivfpq_n2.p) return h->ivfpq_adc_ok;
    h->ivfpq_adc_ok = false;
    if (h->N == 0) return false;
    const int Dm = h->dim, M = h->ivfpq.M, dsub = h->ivfpq.dsub;
    double cn2 = 0.0, rn2 = 0.0;
    for (int l = 0; l < h->nlist; ++l) {
        double s = 0.0;
        for (int d = 0; d < Dm; ++d) s += (double)h->ivf_centroids[(size_t)l * Dm + d] * (double)h->ivf_centroids[(size_t)l * Dm + d];
        cn2 = std::max(cn2, s);
    }
    for (int m = 0; m < M; ++m) {
        double best = 0.0;
        for (int c = 0; c < 256; ++c) {
            const float *v = &h->ivfpq.host[((size_t)m * 256 + c) * dsub];
            double s = 0.0;
            for (int j = 0; j < dsub; ++j) s += (double)v[j] * (double)v[j];
            best = std::max(best, s);
        }
        rn2 += best;
    }
    DevBuf top;
    top.reserve(sizeof(unsigned));
    h->codes.ivfpq_n2.reserve_exact((size_t)h->N * sizeof(float));
    try {
        VDB_HIP(hipMemsetAsync(top.p, 0, sizeof(unsigned), st));
        ivfpq_norms_kernel<<<dim3((unsigned)std::min<int64_t>((h->N + 255) / 256, 1 << 16)), dim3(256), 0, st>>>(
            ivfpq_rows(h), h->N, h->D4, h->codes.ivfpq_n2.as<float>(), top.as<unsigned>());
        VDB_HIP(hipGetLastError());
        float xn2 = 0.f;
        VDB_HIP(hipMemcpyAsync(&xn2, top.p, sizeof(float), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        h->ivfpq_adc_xn2 = (double)xn2;
    } catch (...) {
        ivfpq_adc_drop(h);
        throw;
    }
    h->ivfpq_adc_cr = std::sqrt(cn2) + std::sqrt(rn2);
    const double cr2 = h->ivfpq_adc_cr * h->ivfpq_adc_cr;
    h->ivfpq_adc_ok = h->ivfpq_adc_xn2 >= 1.0e-30 && h->ivfpq_adc_xn2 <= 1.0e30 && cr2 >= 1.0e-30 && cr2 <= 1.0e30;      // (false for NaN)
    return h->ivfpq_adc_ok;
}

int64_t ivfpq_longest_list(const vdb_index_s *h) {
    int64_t m = 0;
    for (int l = 0; l < h->nlist && (size_t)l + 1 < h->ivf_offsets_host.size(); ++l)
        m = std::max(m, h->ivf_offsets_host[(size_t)l + 1] - h->ivf_offsets_host[(size_t)l]);
    return m;
}

// the views into ws.adc_aux of a batch of nb queries x nprobe probes
struct IvfPqAdcAux {
    float *cs, *B;
    int32_t *flag;
    int64_t *pos0;
};
IvfPqAdcAux ivfpq_adc_aux(DevBuf &buf, int64_t nb, int nprobe) {
    const size_t o_flag = 16, o_pos = o_flag + (((size_t)nb * 4 + 15) & ~(size_t)15), o_b = o_pos + (size_t)nb * (nprobe + 1) * 8;
    buf.reserve(o_b + (size_t)nb * nprobe * 4);
    char *p = buf.as<char>();
    return {reinterpret_cast<float *>(p), reinterpret_cast<float *>(p + o_b), reinterpret_cast<int32_t *>(p + o_flag), reinterpret_cast<int64_t *>(p + o_pos)};
}

// prep, tables and scan of nb queries whose probes [nb][nprobe] are on the device: the three dispatches the search and the test hook share
void ivfpq_adc_score(vdb_index_s *h, const IvfAdcPlan &pl, const float *q, int64_t nb, int nprobe, const int64_t *probes, const IvfPqAdcAux &x,
                     float *tables, float *eps, float *scores, long tslot, hipStream_t st) {
    const int M = h->ivfpq.M;
    IvfPqAdcPrepArgs pa{};
    pa.Q = q; pa.cent = h->kept.sq8_cent.as<float>(); pa.probes = probes; pa.offsets = h->lists.ivf_offsets.as<int64_t>();
    pa.nq = nb; pa.D = h->dim; pa.D4 = h->D4; pa.M = M; pa.metric = h->metric; pa.nprobe = nprobe; pa.nlist = h->nlist;
    pa.Xn2 = h->ivfpq_adc_xn2; pa.CR = h->ivfpq_adc_cr;
    pa.cs = x.cs; pa.eps = eps; pa.flag = x.flag; pa.B = x.B; pa.pos0 = x.pos0;
    ivfpq_adc_prep_kernel<<<dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st>>>(pa);
    PqAdcTableArgs t{};
    t.Q = q; t.cb = h->kept.ivfpq_cb.as<float>(); t.tables = tables; t.nq = nb; t.D = h->dim; t.M = M; t.dsub = h->ivfpq.dsub; t.metric = h->metric;
    t.cs_dev = x.cs;
    pq_adc_tables_kernel<<<dim3((unsigned)M, (unsigned)((nb + kPqAdcQB - 1) / kPqAdcQB)), dim3(256), 0, st>>>(t);
    VDB_HIP(hipGetLastError());
    timing_mark(h, tslot, 0, st);
    IvfPqAdcScanArgs sa{};
    sa.codes = h->codes.ivfpq_codes.as<unsigned char>(); sa.n2 = h->codes.ivfpq_n2.as<float>(); sa.tables = tables; sa.cs = x.cs; sa.B = x.B;
    sa.pos0 = x.pos0; sa.probes = probes; sa.offsets = pa.offsets; sa.scores = scores; sa.stride = pl.stride; sa.N = h->N;
    sa.nprobe = nprobe; sa.nlist = h->nlist; sa.M = M; sa.metric = h->metric; sa.part_rows = pl.part_rows;
    if (pl.lds_bytes > 65536)         // (more than the default 64 KiB of dynamic LDS: opt in, on the current device, every time)
        VDB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_adc_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kIvfAdcLdsBudget));
    ivfpq_adc_scan_kernel<<<dim3(pl.parts, (unsigned)nprobe, (unsigned)nb), dim3(256), pl.lds_bytes, st>>>(sa);
    VDB_HIP(hipGetLastError());
    timing_mark(h, tslot, 1, st);
}

// one admitted batch (ivf_search_device_impl): scores, then the tail, then the exact list scan of the queries the tail flagged.
// (D, I) = final rows, or D == nullptr and (pk, pi) = partial rows.  The coarse result is in plan.ivf_probe_i; ws.small is zeroed
void ivfpq_search_adc(vdb_index_s *h, const IvfAdcPlan &pl, const float *q, const float *qpad, int64_t nb, int k, int nprobe, float *D, int64_t *I,
                      double *pk, int64_t *pi, long tslot, hipStream_t st) {
    Workspace &ws = h->ws;
    const int M = h->ivfpq.M;
    const int64_t *probes = h->plan.ivf_probe_i.as<int64_t>();
    const IvfPqAdcAux x = ivfpq_adc_aux(ws.adc_aux, nb, nprobe);
    ws.adc_tab.reserve((size_t)nb * M * 256 * sizeof(float));
    ws.adc_scores.reserve((size_t)nb * pl.stride * sizeof(float));
    ws.eps.reserve((size_t)nb * sizeof(float));
    ws.fallback.reserve((size_t)nb * sizeof(int32_t));
    ivfpq_adc_score(h, pl, q, nb, nprobe, probes, x, ws.adc_tab.as<float>(), ws.eps.as<float>(), ws.adc_scores.as<float>(), tslot, st);
    IvfPqAdcTailArgs ta{};
    ta.c = RefineCommon{nullptr, qpad, h->N, h->id_base, h->D4, h->metric, k, h->lists.ivf_ids.as<int64_t>()};
    ta.c.ivfpq = ivfpq_rows(h);
    ta.scores = ws.adc_scores.as<float>(); ta.eps = ws.eps.as<float>(); ta.flag = x.flag;
    ta.pos0 = x.pos0; ta.probes = probes; ta.offsets = h->lists.ivf_offsets.as<int64_t>();
    ta.stride = pl.stride; ta.nprobe = nprobe; ta.nlist = h->nlist; ta.cand_cap = pl.cand_cap;
    ta.fallback = ws.fallback.as<int32_t>();
    ta.stat_counters = reinterpret_cast<unsigned long long *>(ws.small.as<char>() + 64);
    ta.D = D; ta.I = I; ta.pk = pk; ta.pi = pi;
    const int kpl = kpl_for(k);
    switch (kpl) {        // (k <= 1024: no KPL = 32)
        case 1: ivfpq_adc_tail_kernel<1><<<dim3((unsigned)nb), dim3(256), 0, st>>>(ta); break;
        case 2: ivfpq_adc_tail_kernel<2><<<dim3((unsigned)nb), dim3(256), 0, st>>>(ta); break;
        case 4: ivfpq_adc_tail_kernel<4><<<dim3((unsigned)nb), dim3(256), 0, st>>>(ta); break;
        case 8: ivfpq_adc_tail_kernel<8><<<dim3((unsigned)nb), dim3(256), 0, st>>>(ta); break;
        case 16: ivfpq_adc_tail_kernel<16><<<dim3((unsigned)nb), dim3(256), 0, st>>>(ta); break;
        default: throw Error(VDB_ERR_STATE, "internal: the ADC tail serves k <= 1024");
    }
    VDB_HIP(hipGetLastError());
    IvfScanArgs a{};
    a.c = ta.c;
    a.offsets = ta.offsets; a.probes = probes; a.nq = nb; a.nprobe = nprobe; a.S = 1;
    a.only_flagged = ta.fallback;
    a.D = D; a.I = I; a.pkeys = pk; a.pids = pi;
    DISPATCH_KPL(kpl, (ivf_scan_kernel<KPL><<<dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st>>>(a)));
    VDB_HIP(hipGetLastError());
}

// vdb_debug_ivfpq_adc_scores: the scan's own three dispatches for nq queries that all probe list `l`, on buffers of the call's own
void ivfpq_adc_debug_scores(vdb_index_s *h, const float *q_host, int64_t nq, int l, int64_t row0, int64_t nrows, float *scores_host, float *eps_host,
                            double *cscale) {
    ivf_require(h->ivf_built && h->N > 0, VDB_ERR_STATE, "Index has not been built yet.");
    ivf_require(q_host && scores_host && eps_host, VDB_ERR_INVALID, "null pointer");
    ivf_require(l >= 0 && l < h->nlist && nq >= 1 && nq <= kIvfAdcMaxBatch, VDB_ERR_INVALID, "bad list or query count");
    const int64_t len = h->ivf_offsets_host[(size_t)l + 1] - h->ivf_offsets_host[(size_t)l];
    ivf_require(row0 >= 0 && nrows >= 1 && row0 + nrows <= len, VDB_ERR_INVALID, "bad range");
    set_device(h->device);
    hipStream_t st = nullptr;
    ivf_require(ivfpq_adc_prepare(h, st), VDB_ERR_STATE, "vdb_debug_ivfpq_adc_scores: the norms of this index are outside the range the ADC scan serves");
    Options opt = h->opt;
    opt.force_path = 0;
    opt.ivfpq_adc_max_batch = kIvfAdcMaxBatch;
    const IvfAdcPlan pl = ivf_adc_plan(opt, 2, h->ivfpq.M, true, len, len, nq, 1, 1);
    ivf_require(pl.ok, VDB_ERR_UNSUPPORTED, "vdb_debug_ivfpq_adc_scores: the ADC scan does not serve this M or this many scores");
    const int Dm = h->dim, M = h->ivfpq.M;
    DevBuf dq, probes, aux, tables, eps, out;
    dq.reserve((size_t)nq * Dm * 4);
    probes.reserve((size_t)nq * 8);
    tables.reserve((size_t)nq * M * 1024);
    eps.reserve((size_t)nq * 4);
    out.reserve((size_t)nq * pl.stride * 4);
    const IvfPqAdcAux x = ivfpq_adc_aux(aux, nq, 1);
    const std::vector<int64_t> pl_host((size_t)nq, (int64_t)l);
    VDB_HIP(hipMemcpyAsync(dq.p, q_host, (size_t)nq * Dm * 4, hipMemcpyHostToDevice, st));
    VDB_HIP(hipMemcpyAsync(probes.p, pl_host.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
    ivfpq_adc_score(h, pl, dq.as<float>(), nq, 1, probes.as<int64_t>(), x, tables.as<float>(), eps.as<float>(), out.as<float>(), -1, st);
    float cs = 0.f;
    VDB_HIP(hipMemcpy2DAsync(scores_host, (size_t)nrows * 4, out.as<float>() + row0, (size_t)pl.stride * 4, (size_t)nrows * 4, (size_t)nq,
                             hipMemcpyDeviceToHost, st));
    VDB_HIP(hipMemcpyAsync(eps_host, eps.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipMemcpyAsync(&cs, x.cs, 4, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
    if (cscale) *cscale = (double)cs;
}

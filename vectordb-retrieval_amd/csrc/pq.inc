// pq.inc -- host side of the product quantizer (kernels: pq.hpp).  First the core that the flat PQ<M> index and
// IVF<nlist>,PQ<M> (ivf_pq.inc, ivf.inc) share: the M rule, installing and reading codebooks, their training, the encode
// launch.  Then the flat index: encoding adds, the derived scan statistics, the per-slab panel pass of a search, the launchers of the
// lookup-table (ADC) scan of small batches (pq_adc.hpp) and its test hook.  Included by
// vdbhip.hip ahead of ivf.inc; a handle keeps one PqCodebooks for each of the two (vdb_index_s: pq, ivfpq).

namespace {

// ---- the core ---------------------------------------------------------------------------------------------------------------
void pq_check_M(const vdb_index_s *h, int M) {
    if (M < 1 || M > std::min(h->dim, 256)) throw Error(VDB_ERR_INVALID, "M must be in [1, min(dim, 256)]");
    if (h->dim % M) throw Error(VDB_ERR_INVALID, "dim must be a multiple of M");
}

// [M][256][dsub] finite floats become the codebooks `q` of the handle, with their device copy `dev`; refused ones leave both as
// they were.  The caller has synchronised the device, and drops what the old codebooks made (a captured graph, encoded rows).
void pq_install_codebooks(vdb_index_s *h, PqCodebooks &q, DevBuf &dev, int M, const float *cb_host) {
    const size_t total = (size_t)256 * h->dim;
    for (size_t i = 0; i < total; ++i)
        if (!std::isfinite(cb_host[i])) throw Error(VDB_ERR_INVALID, "codebook entries must be finite");
    dev.reserve_exact(total * sizeof(float));
    VDB_HIP(hipMemcpy(dev.p, cb_host, total * sizeof(float), hipMemcpyHostToDevice));
    q.host.assign(cb_host, cb_host + total);
    q.M = M;
    q.dsub = h->dim / M;
}

// vdb_*_get_codebooks: *M = q.M when the handle is of the kind that owns `q` (`mine`), else 0; the entries when asked for
void pq_get_codebooks(const PqCodebooks &q, bool mine, int *M, float *codebooks_host) {
    if (!M) throw Error(VDB_ERR_INVALID, "null pointer");
    *M = mine ? q.M : 0;
    if (codebooks_host && *M > 0) memcpy(codebooks_host, q.host.data(), q.host.size() * sizeof(float));
}

// the training arguments both trainers refuse (max_points_per_centroid <= 0: the default, 256)
void pq_check_train_args(const float *x_host, int64_t n, int niter, int &max_points_per_centroid) {
    if (!x_host || n <= 0) throw Error(VDB_ERR_INVALID, "no training vectors");
    if (n < 256) throw Error(VDB_ERR_INVALID, "need at least 256 training vectors (one per centroid of a sub-space)");
    if (niter < 0 || niter > 1000) throw Error(VDB_ERR_INVALID, "niter out of range");
    if (max_points_per_centroid <= 0) max_points_per_centroid = 256;
}

// one row sample [ns][D] for every sub-space, drawn with `seed` (vdb_ivf_train's draws)
std::vector<float> pq_training_sample(const float *x_host, int64_t n, int D, uint64_t seed, int max_points_per_centroid) {
    const int64_t ns = std::min<int64_t>(n, (int64_t)max_points_per_centroid * 256);
    const std::vector<int64_t> pick = sample_rows(n, ns, seed);
    std::vector<float> sample((size_t)ns * D);
    for (int64_t i = 0; i < ns; ++i) memcpy(&sample[(size_t)i * D], x_host + (size_t)pick[(size_t)i] * D, (size_t)D * sizeof(float));
    return sample;
}

// sampled rows [ns][D] (IVF-PQ: their residuals) -> codebooks [M][256][dsub].  Sub-space m: the library's k-means
// (vdb_ivf_train on a flat L2 handle of dsub dims) over the sample, seed + m
std::vector<float> pq_train_codebooks(int device, const std::vector<float> &sample, int D, int M, int niter, uint64_t seed,
                                      int max_points_per_centroid) {
    const int dsub = D / M;
    const int64_t ns = (int64_t)(sample.size() / (size_t)D);
    std::vector<float> cb((size_t)256 * D), sub((size_t)ns * dsub);
    for (int m = 0; m < M; ++m) {
        for (int64_t i = 0; i < ns; ++i) memcpy(&sub[(size_t)i * dsub], &sample[(size_t)i * D + (size_t)m * dsub], (size_t)dsub * sizeof(float));
        vdb_handle t = nullptr;
        int rc = vdb_create(dsub, VDB_METRIC_L2, device, &t);
        if (rc == VDB_OK) rc = vdb_ivf_train(t, 256, sub.data(), ns, niter, seed + (uint64_t)m, max_points_per_centroid);
        if (rc == VDB_OK) rc = vdb_ivf_get_centroids(t, &cb[(size_t)m * 256 * dsub]);
        const std::string msg = rc == VDB_OK ? std::string() : g_last_error;
        if (t) (void)vdb_destroy(t);
        if (rc != VDB_OK) throw Error(rc, "k-means of sub-space " + std::to_string(m) + ": " + msg);
    }
    return cb;
}

// codes of the n rows at `rows` (device, `pitch` floats each, zero padded), or of their residuals against cent[assign[i]]
// (both null for the flat index): pq_encode_kernel, the sub-space's codebook in LDS when its 256 dsub floats fit 48 KiB
void pq_launch_encode(const float *rows, int64_t n, int64_t pitch, const float *cent, const int64_t *assign, const float *cb, int M, int dsub,
                      unsigned char *codes, hipStream_t st) {
    const bool in_lds = (size_t)256 * dsub * sizeof(float) <= 49152;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048)), (unsigned)M);
    const size_t lds_bytes = in_lds ? (size_t)256 * dsub * sizeof(float) : 0;
    if (cent) pq_encode_kernel<true><<<grid, dim3(256), lds_bytes, st>>>(rows, n, pitch, cent, assign, cb, M, dsub, in_lds ? 256 * dsub : 0, codes);
    else pq_encode_kernel<false><<<grid, dim3(256), lds_bytes, st>>>(rows, n, pitch, nullptr, nullptr, cb, M, dsub, in_lds ? 256 * dsub : 0, codes);
    VDB_HIP(hipGetLastError());
}

// bytes per code row staged in LDS by the panel passes: M rounded up to a dword, an odd number of dwords (the rows a lane
// group reads fall on different banks)
inline int pq_code_pitch(int M) {
    const int pitch = (M + 3) & ~3;
    return (pitch / 4) % 2 == 0 ? pitch + 4 : pitch;
}

// ---- the flat index ---------------------------------------------------------------------------------------------------------
PqRows pq_rows(const vdb_index_s *h) {
    PqRows p;
    p.codes = h->codes.pq_codes.as<unsigned char>();
    p.cb = h->kept.pq_cb.as<float>();
    p.M = h->pq.M;
    p.dsub = h->pq.dsub;
    return p;
}

// What the PQ entry points admit.  A handle becomes a PQ index on one device, with no other row store or structure over float32
// rows (and no option a PQ index refuses: refuse_options_set).  The calls on the codes refuse the handles that never hold flat
// codebooks; every other kind has none yet, which is the state error of pq_need_codebooks.
constexpr unsigned kBecomesPq = kFlat | kPq, kPqCodeCalls = kAnyKind & ~(kMulti | kIvfPq | kIvfI8);
void pq_need_codebooks(const vdb_index_s *h, const char *what) {
    if (!pq_on(h)) throw Error(VDB_ERR_STATE, std::string(what) + ": no codebooks (call vdb_pq_train or vdb_pq_set_codebooks first)");
}

// x^ of the code rows [r0, r0 + n): float32, `pitch` floats per row (zero beyond dim)
void pq_decode_rows(vdb_index_s *h, int64_t r0, int64_t n, int64_t pitch, float *out, hipStream_t st) {
    if (n <= 0) return;
    const int64_t blocks = std::min<int64_t>((n * pitch + 255) / 256, 1 << 16);
    IvfPqRows p;
    p.pq = pq_rows(h);
    p.pq.codes += (size_t)r0 * p.pq.M;
    pq_decode_rows_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(p, n, h->dim, h->D4, pitch, out);
    VDB_HIP(hipGetLastError());
}

// Everything a search needs besides the codes, from the h->N code rows: the flat build's statistics (row norms -> bias, max
// norm, scale sx, fp16-exactness, integer flags) taken on a TRANSIENT float32 copy x^ -- bit for bit those of a flat index
// over x^ -- the span / tile geometry, and the scaled fp16 table of the panel pass.  The copy and the norms are freed again.
void pq_rebuild(vdb_index_s *h, hipStream_t st) {
    const int D = h->dim, D4 = h->D4;
    const int64_t n = h->N;
    h->built = false;
    h->scan_ok = false;
    h->int8_only = false;
    h->panels_streamed = false;
    h->i8_ok = false;
    h->tile16 = h->ksteps > kMaxKSteps;          // (D > 128: p16 panels; D <= 128: layout "x16" -- the slab is made per search either way)
    h->x16 = !h->tile16;
    const int64_t span_rows = h->tile16 ? kSpanRows16 : kSpanRows;
    h->Npad = (n + span_rows - 1) / span_rows * span_rows;
    if (n == 0) {
        h->built = true;
        return;
    }
    try {
        h->rows.x32.reserve_exact((size_t)n * D4 * sizeof(float));
        pq_decode_rows(h, 0, n, D4, h->rows.x32.as<float>(), st);
        index_stats(h, st);
        h->i8_ok = false;                        // (x^ is not kept in any integer form: the fp16 scan serves every batch)
        if (D <= 4096 && !h->nonfinite) {
            const int64_t total = n * D4;
            pq_fp16_flag_kernel<<<dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16)), dim3(256), 0, st>>>(
                h->rows.x32.as<float>(), total, h->sx, h->kept.stats.as<IndexStats>());
            const int64_t tab_n = (int64_t)256 * D;
            h->scan.pq_tab.reserve_exact((size_t)tab_n * sizeof(_Float16));
            pq_table_kernel<<<dim3((unsigned)((tab_n + 255) / 256)), dim3(256), 0, st>>>(h->kept.pq_cb.as<float>(), tab_n, h->sx,
                                                                                       h->scan.pq_tab.as<_Float16>());
            h->scan.bias.reserve((size_t)h->Npad * sizeof(float));
            build_bias_kernel<<<dim3((unsigned)((h->Npad + 255) / 256)), dim3(256), 0, st>>>(h->rows.xnorm2.as<float>(), n, h->Npad, h->metric,
                                                                                            h->scan.bias.as<float>());
            VDB_HIP(hipGetLastError());
            IndexStats hs;
            VDB_HIP(hipMemcpyAsync(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
            VDB_HIP(hipStreamSynchronize(st));
            h->corpus_fp16_exact = hs.not_fp16_exact == 0;
            h->scan_ok = true;
        }
    } catch (...) {
        h->rows.x32.release();
        h->rows.xnorm2.release();
        throw;
    }
    VDB_HIP(hipStreamSynchronize(st));
    h->rows.x32.release();
    h->rows.xnorm2.release();                    // (the norms only fed `bias`)
    h->built = true;
}

// the index holds N0 + n code rows afterwards, or (on failure) the N0 it held before
template <class F>
void pq_append(vdb_index_s *h, int64_t n, int64_t id_base, F &&fill) {
    if (n < 0) throw Error(VDB_ERR_INVALID, "negative row count");
    const int64_t N0 = h->N;
    if (N0 > 0) require_same_id_base(h, id_base);
    if (N0 + n > 2147483647ll - 1024) throw Error(VDB_ERR_UNSUPPORTED, "more than 2^31 rows per shard");
    graph_reset(h);
    VDB_HIP(hipDeviceSynchronize());             // (searches of the codes about to move may still run)
    if (N0 == 0) h->id_base = id_base;
    if (n == 0) {
        if (!h->built) pq_rebuild(h, nullptr);
        return;
    }
    const size_t M = (size_t)h->pq.M;
    h->codes.pq_codes.grow((size_t)(N0 + n) * M + 16, (size_t)N0 * M);      // (16 spare bytes: the 16-byte code loads of the panel pass)
    fill(h->codes.pq_codes.as<unsigned char>() + (size_t)N0 * M);
    h->N = N0 + n;
    try {
        pq_rebuild(h, nullptr);
    } catch (...) {
        (void)hipGetLastError();
        h->N = N0;
        try {
            pq_rebuild(h, nullptr);
        } catch (...) {                          // not even the old state fits any more: the index is emptied, loudly
            h->N = 0;
            h->built = false;
            h->scan_ok = false;
        }
        throw;
    }
}

// rows (host) -> codes (device), through a float32 block of at most ~256 MiB
void pq_encode_host_rows(vdb_index_s *h, const float *x_host, int64_t n, unsigned char *codes, hipStream_t st) {
    const int D = h->dim, D4 = h->D4, M = h->pq.M;
    const int64_t block_rows = std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)256 << 20) / ((int64_t)D4 * 4)));
    DevBuf blk;
    blk.reserve((size_t)block_rows * D4 * sizeof(float));
    for (int64_t r0 = 0; r0 < n; r0 += block_rows) {
        const int64_t nb = std::min<int64_t>(block_rows, n - r0);
        if (D4 != D) VDB_HIP(hipMemsetAsync(blk.p, 0, (size_t)nb * D4 * sizeof(float), st));
        upload_rows(h, blk.as<float>(), D4, x_host + (size_t)r0 * D, nb, D, st);
        pq_launch_encode(blk.as<float>(), nb, D4, nullptr, nullptr, h->kept.pq_cb.as<float>(), M, h->pq.dsub, codes + (size_t)r0 * M, st);
        VDB_HIP(hipStreamSynchronize(st));       // (the block is refilled by the next one)
    }
}

// The panel pass of one slab: tiles [tile0, tile0 + ntiles) of the scan layout -> fp16 panels at `panels`.
// LDS: 4 waves x the staged code rows of a tile, then the table slice.  A workgroup gets at most half a CU's 160 KiB, so
// two run per CU; at D = 128 the whole table (64 KiB) fits, above that the 32-dim k-steps are dealt to blockIdx.y in
// slices whose dims are whole sub-spaces.  A table no slice of which fits is read through the cache.
constexpr int kPqLdsBudget = 80 * 1024;
void launch_pq_panels(vdb_index_s *h, int64_t tile0, int64_t ntiles, half8 *panels, hipStream_t st) {
    if (ntiles <= 0) return;
    PqPanelArgs a{};
    a.codes = h->codes.pq_codes.as<unsigned char>();
    a.tab = h->scan.pq_tab.as<_Float16>();
    a.panels = panels;
    a.N = h->N;
    a.tile0 = tile0;
    a.ntiles = ntiles;
    a.D = h->dim;
    a.M = h->pq.M;
    a.dsub = h->pq.dsub;
    a.p16 = h->tile16 ? 1 : 0;
    a.ksteps = h->tile16 ? h->ksteps / 2 : h->ksteps;
    a.code_pitch = pq_code_pitch(a.M);
    const int R = a.p16 ? 16 : 32;
    const int stage = 4 * ((R * a.code_pitch + 15) & ~15);
    const int ks32_n = a.p16 ? a.ksteps : a.ksteps / 2;
    const int dsub = a.dsub;
    int unit = dsub;                             // k-steps per slice unit: lcm(32, dsub) / 32
    for (int gdiv = 32; gdiv >= 1; gdiv >>= 1)
        if (dsub % gdiv == 0) { unit = dsub / gdiv; break; }
    bool lds = false;
    a.slice_ks = ks32_n;
    const int64_t full = (int64_t)256 * a.D * 2;
    size_t lds_bytes = (size_t)stage;
    if (stage + full + (int64_t)a.M * kPqTabSkew * 2 <= kPqLdsBudget) {
        lds = true;
        lds_bytes += (size_t)full + (size_t)a.M * kPqTabSkew * 2;
    } else {
        const int64_t unit_bytes = (int64_t)unit * 32 * 512 + (int64_t)(unit * 32 / dsub) * kPqTabSkew * 2;      // (table + skew of its sub-spaces)
        const int64_t units = (kPqLdsBudget - stage) / unit_bytes;
        if (units >= 1 && a.p16) {
            lds = true;
            a.slice_ks = (int)(units * unit);
            lds_bytes += (size_t)(units * unit_bytes);
        }
    }
    const unsigned gy = (unsigned)((ks32_n + a.slice_ks - 1) / a.slice_ks);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ntiles + 3) / 4, (int64_t)2 * h->n_cus));
    const int W = dsub % 8 == 0 ? 8 : dsub % 4 == 0 ? 4 : dsub % 2 == 0 ? 2 : 1;
#define VDB_PQ_PANELS(W_) do { \
        if (lds) { \
            if (lds_bytes > 65536)       /* (more than the default 64 KiB of dynamic LDS: opt in, on the current device, every time) */ \
                VDB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_panels_kernel<W_, true>), \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, kPqLdsBudget)); \
            pq_panels_kernel<W_, true><<<dim3(gx, gy), dim3(256), lds_bytes, st>>>(a); \
        } else { \
            pq_panels_kernel<W_, false><<<dim3(gx, gy), dim3(256), (size_t)stage, st>>>(a); \
        } } while (0)
    if (W == 8) VDB_PQ_PANELS(8);
    else if (W == 4) VDB_PQ_PANELS(4);
    else if (W == 2) VDB_PQ_PANELS(2);
    else VDB_PQ_PANELS(1);
#undef VDB_PQ_PANELS
    VDB_HIP(hipGetLastError());
}

// ---- the ADC scan (pq_adc.hpp) ------------------------------------------------------------------------------------------------
// LDS of a scan workgroup: the query's table (M KiB), the reduction block, and -- when M is a multiple of 4 and it still fits --
// one bin of staged code rows.  The budget is a whole CU's LDS: M <= 127 stages, M = 128 (the table alone is 128 KiB) reads its
// codes from the index, M >= 160 does not fit and stays on the panel pass.
constexpr int kPqAdcLdsBudget = 160 * 1024;
bool pq_adc_fits(int M) { return (int64_t)M * 1024 + kPqAdcAuxBytes <= kPqAdcLdsBudget; }
inline bool pq_adc_staged(int M) {
    return M % 4 == 0 && 16 * M <= 256 * kPqAdcMaxPieces &&
           (int64_t)M * 1024 + kPqAdcAuxBytes + (int64_t)256 * pq_code_pitch(M) <= kPqAdcLdsBudget;
}

// the lookup tables [nq][M][256] and the ADC error bounds of a batch whose statistics `info` holds (or will, in stream order)
void launch_pq_adc_tables(vdb_index_s *h, const float *dq, int64_t nq, const QueryBatchInfo *info, float *tables, float *eps, hipStream_t st) {
    PqAdcTableArgs t{};
    t.Q = dq;
    t.cb = h->kept.pq_cb.as<float>();
    t.info = info;
    t.tables = tables;
    t.eps = eps;
    t.nq = nq;
    t.D = h->dim;
    t.M = h->pq.M;
    t.dsub = h->pq.dsub;
    t.metric = h->metric;
    t.xnorm_max = sqrtf(h->maxnorm2) * 1.0000002f;
    pq_adc_tables_kernel<<<dim3((unsigned)t.M, (unsigned)((nq + kPqAdcQB - 1) / kPqAdcQB)), dim3(256), 0, st>>>(t);
    VDB_HIP(hipGetLastError());
}

// what the scan and the test hook share of the arguments
PqAdcScanArgs pq_adc_args(vdb_index_s *h, const float *tables, const QueryBatchInfo *info) {
    PqAdcScanArgs a{};
    a.codes = h->codes.pq_codes.as<unsigned char>();
    a.bias = h->scan.bias.as<float>();
    a.tables = tables;
    a.info = info;
    a.N = h->N;
    a.M = h->pq.M;
    a.groups = h->tile16 ? 4 : 2;
    a.gshift = h->tile16 ? 2 : 3;                 // (quads on p16 spans, octs on layout "x16": f16_octs(shape, opt, 0) of scan_plan.hpp)
    a.code_pitch = pq_code_pitch(a.M);
    return a;
}

// one workgroup per (chunk, query) of the geometry in `a`
void launch_pq_adc_scan(vdb_index_s *h, PqAdcScanArgs &a, int64_t nq, hipStream_t st) {
    const bool staged = pq_adc_staged(a.M);
    const size_t lds = (size_t)a.M * 1024 + kPqAdcAuxBytes + (staged ? (size_t)256 * a.code_pitch : 0);
    if (lds > (size_t)kPqAdcLdsBudget) throw Error(VDB_ERR_STATE, "internal: the ADC table does not fit the LDS");
    const dim3 grid((unsigned)a.nchunks, (unsigned)nq);
    if (staged) {
        if (lds > 65536)         // (more than the default 64 KiB of dynamic LDS: opt in, on the current device, every time)
            VDB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_adc_scan_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kPqAdcLdsBudget));
        pq_adc_scan_kernel<true><<<grid, dim3(256), lds, st>>>(a);
    } else {
        if (lds > 65536)
            VDB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_adc_scan_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kPqAdcLdsBudget));
        pq_adc_scan_kernel<false><<<grid, dim3(256), lds, st>>>(a);
    }
    VDB_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int vdb_pq_set_codebooks(vdb_handle hh, int M, const float *codebooks_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_pq_set_codebooks", kBecomesPq);
        refuse_options_set(h, "vdb_pq_set_codebooks", kPq);
        pq_check_M(h, M);
        if (!codebooks_host) throw Error(VDB_ERR_INVALID, "null codebook pointer");
        if (h->N > 0) throw Error(VDB_ERR_STATE, "the codebooks are set before rows exist (vdb_reset first): the codes of the " +
                                                     std::to_string(h->N) + " rows held would lose their meaning");
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        graph_reset(h);
        pq_install_codebooks(h, h->pq, h->kept.pq_cb, M, codebooks_host);
    });
}

int vdb_pq_get_codebooks(vdb_handle hh, int *M, float *codebooks_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_pq_get_codebooks", kAnyKind);
        pq_get_codebooks(h->pq, true, M, codebooks_host);       // (pq.M is 0 on every other kind)
    });
}

int vdb_pq_train(vdb_handle hh, int M, const float *x_host, int64_t n, int niter, uint64_t seed, int max_points_per_centroid) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_pq_train", kBecomesPq);
        refuse_options_set(h, "vdb_pq_train", kPq);
        pq_check_M(h, M);
        pq_check_train_args(x_host, n, niter, max_points_per_centroid);
        if (h->N > 0) throw Error(VDB_ERR_STATE, "the codebooks are trained before rows exist (vdb_reset first)");
        const std::vector<float> cb = pq_train_codebooks(h->device, pq_training_sample(x_host, n, h->dim, seed, max_points_per_centroid), h->dim, M,
                                                         niter, seed, max_points_per_centroid);
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        graph_reset(h);
        pq_install_codebooks(h, h->pq, h->kept.pq_cb, M, cb.data());
    });
}

int vdb_pq_add(vdb_handle hh, const float *x_host, int64_t n, int64_t id_base) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_pq_add", kPqCodeCalls);
        pq_need_codebooks(h, "vdb_pq_add");
        if (n > 0 && !x_host) throw Error(VDB_ERR_INVALID, "null corpus pointer");
        set_device(h->device);
        pq_append(h, n, id_base, [&](unsigned char *codes) { pq_encode_host_rows(h, x_host, n, codes, nullptr); });
    });
}

int vdb_pq_add_codes(vdb_handle hh, const uint8_t *codes_host, int64_t n, int64_t id_base) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_pq_add_codes", kPqCodeCalls);
        pq_need_codebooks(h, "vdb_pq_add_codes");
        if (n > 0 && !codes_host) throw Error(VDB_ERR_INVALID, "null code pointer");
        set_device(h->device);
        pq_append(h, n, id_base, [&](unsigned char *codes) {
            VDB_HIP(hipMemcpy(codes, codes_host, (size_t)n * h->pq.M, hipMemcpyHostToDevice));
        });
    });
}

int vdb_pq_get_codes(vdb_handle hh, uint8_t *codes_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_pq_get_codes", kPqCodeCalls);
        pq_need_codebooks(h, "vdb_pq_get_codes");
        if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
        if (!codes_host) throw Error(VDB_ERR_INVALID, "null pointer");
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        VDB_HIP(hipMemcpy(codes_host, h->codes.pq_codes.p, (size_t)h->N * h->pq.M, hipMemcpyDeviceToHost));
    });
}

int vdb_debug_pq_adc_scores(vdb_handle hh, const float *q_host, int64_t nq, int64_t row0, int64_t nrows, float *scores_host,
                            float *eps_host, double *cscale) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_debug_pq_adc_scores", kPq);
        if (!h->built || h->N == 0 || !h->scan_ok) throw Error(VDB_ERR_STATE, "vdb_debug_pq_adc_scores: no scan statistics (no rows, or a corpus the scan does not serve)");
        if (!pq_adc_fits(h->pq.M)) throw Error(VDB_ERR_UNSUPPORTED, "vdb_debug_pq_adc_scores: the lookup table of M = " + std::to_string(h->pq.M) + " sub-spaces does not fit the LDS");
        if (!q_host || !scores_host || !eps_host) throw Error(VDB_ERR_INVALID, "null pointer");
        if (nq <= 0 || nq > 65535 || nrows <= 0 || row0 < 0 || row0 + nrows > h->N) throw Error(VDB_ERR_INVALID, "bad range");
        set_device(h->device);
        hipStream_t st = nullptr;
        const int Dm = h->dim, M = h->pq.M;
        DevBuf dq, info, tables, eps, out;
        dq.reserve((size_t)nq * Dm * 4);
        info.reserve(sizeof(QueryBatchInfo));
        tables.reserve((size_t)nq * M * 1024);
        eps.reserve((size_t)nq * 4);
        out.reserve((size_t)nq * nrows * 4);
        VDB_HIP(hipMemcpyAsync(dq.p, q_host, (size_t)nq * Dm * 4, hipMemcpyHostToDevice, st));
        VDB_HIP(hipMemsetAsync(info.p, 0, sizeof(QueryBatchInfo), st));
        const int64_t total = nq * Dm;
        query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, st>>>(dq.as<float>(), total, info.as<QueryBatchInfo>(),
            FinalizeArgs{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2, 0});
        launch_pq_adc_tables(h, dq.as<float>(), nq, info.as<QueryBatchInfo>(), tables.as<float>(), eps.as<float>(), st);
        const PqAdcScanArgs a = pq_adc_args(h, tables.as<float>(), info.as<QueryBatchInfo>());
        const size_t lds = (size_t)M * 1024;
        if (lds > 65536)
            VDB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_adc_scores_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPqAdcLdsBudget));
        pq_adc_scores_kernel<<<dim3((unsigned)((nrows + 255) / 256), (unsigned)nq), dim3(256), lds, st>>>(a, row0, nrows, out.as<float>());
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

// ivf_i8.inc -- host side of IVF-I8 (kernels: ivf_i8.hpp, rules: ivf_i8_plan.hpp).  Included by ivf.inc inside its anonymous namespace.
//
// An IVF-I8 handle (vdb_ivf_set_codec(h, 3) on an empty single-device handle, D <= 128) files a byte-valued corpus -- every value
// an integer in 0..255 or in -128..127, the test of the flat int8 copies -- LOSSLESSLY as int8 rows x - cx in list order, and keeps
// of an IVF-Flat index over the same rows only what is derived from those bytes: rows8, panels8, bias8, rowstat8, the fp16 scan's
// bias and statistics, the ids, the CSR and span tables and the centroids.  No float32 rows, no resident fp16 panels.  Integer
// batches inside the byte window take the int8 list scan and the integer refine as they do on IVF-Flat; every other batch of the
// list-major path scans fp16 panels converted from panels8 for that batch (ivf_i8_panels), and every exact stage scores the
// int8 rows through exact_key_i8 (refine.hpp) -- the float64 chain over x = byte + cx, the key of the float32 row.  Results are
// the IVF-Flat results, bit for bit (DESIGN 4.18).

inline bool ivf_i8(const vdb_index_s *h) { return h->ivf_codec == 3; }

int64_t ivf_build_spans(vdb_index_s *h, int span_rows);     // (ivf.inc)

// dst takes over what src holds (a buffer built as a temporary of the add becomes the handle's)
void i8_take(DevBuf &dst, DevBuf &src) {
    dst.release();
    dst.p = src.p; dst.cap = src.cap; dst.borrowed = src.borrowed;
    src.p = nullptr; src.cap = 0; src.borrowed = false;
}

// where the exact stages of a search find the rows of an IVF-I8 index (c.X stays nullptr: row_key falls through to exact_key_i8)
void i8_refine_rows(const vdb_index_s *h, RefineCommon &c) {
    c.X8 = h->scan.rows8.as<signed char>();
    c.x8_pitch = h->rows8_pitch; c.cx = h->i8_cx; c.D = h->dim;
}

// Everything derived from the N int8 rows in list order (h->scan.rows8, window h->i8_cx): span tables, panels8, bias8, rowstat8,
// the fp16 scan's bias, and the statistics ivf_build_panel_space takes from the float32 rows of an IVF-Flat index --
//   absmax       max(|min|, |max|) of the corpus: the same integer
//   maxnorm2     (float)max sum x^2: corpus_stats_kernel rounds the float64 sum of the same integers once, exact below 2^24
//   sx = 1, corpus_int_unscaled, corpus_fp16_exact: integers of magnitude <= 255 are stored unscaled and are exact in fp16
// so prep, eps and select see the numbers they see on IVF-Flat.
void i8_build_panel_space(vdb_index_s *h) {
    h->ivf_mfma_ok = false;
    h->scan_ok = false;
    h->tile16 = false;
    h->ivf_tps = 0;
    h->nonfinite = false;
    h->corpus_int_unscaled = true;
    h->corpus_fp16_exact = true;
    h->sx = 1.f;
    h->absmax = (float)std::max(std::abs(h->i8_min), std::abs(h->i8_max));
    h->maxnorm2 = 0.f;
    h->i8_ok = h->N > 0;
    DevBuf *old[] = {&h->scan.panels, &h->scan.panels8, &h->scan.bias8, &h->scan.rowstat8, &h->scan.bias};
    for (auto b : old) b->release();
    if (h->N == 0) return;
    const int64_t P = ivf_build_spans(h, kIvfSpanRows);
    if (P == 0) return;
    hipStream_t st = nullptr;
    const int64_t ntiles = P * kIvfTilesPerSpan, t8 = ntiles * h->i8_ks * 64, panel_rows = P * kIvfSpanRows;
    DevBuf maxn2;
    maxn2.reserve(4);
    VDB_HIP(hipMemsetAsync(maxn2.p, 0, 4, st));
    h->scan.panels8.reserve_exact((size_t)t8 * sizeof(int4v));
    h->scan.bias8.reserve_exact((size_t)2 * panel_rows * sizeof(int32_t));
    h->scan.rowstat8.reserve_exact((size_t)h->N * 2 * sizeof(int));
    h->scan.bias.reserve_exact((size_t)panel_rows * sizeof(float));
    ivf_i8_build_panels_kernel<<<dim3((unsigned)((t8 + 255) / 256)), dim3(256), 0, st>>>(
        h->scan.rows8.as<signed char>(), h->rows8_pitch, h->dim, h->i8_ks, ntiles, h->lists.ivf_span_row0.as<int32_t>(),
        h->lists.ivf_span_valid.as<int32_t>(), h->scan.panels8.as<int4v>());
    ivf_i8_build_bias_kernel<<<dim3((unsigned)((panel_rows + 255) / 256)), dim3(256), 0, st>>>(
        h->scan.rows8.as<signed char>(), h->rows8_pitch, h->i8_cx, P, h->dim, h->metric, h->lists.ivf_span_row0.as<int32_t>(),
        h->lists.ivf_span_valid.as<int32_t>(), h->scan.bias8.as<int32_t>(), h->scan.rowstat8.as<int>(), h->scan.bias.as<float>(),
        maxn2.as<int>());
    VDB_HIP(hipGetLastError());
    int n2 = 0;
    VDB_HIP(hipMemcpyAsync(&n2, maxn2.p, 4, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
    h->maxnorm2 = (float)n2;
    h->ivf_mfma_ok = true;
}

// vdb_ivf_add(_assigned) on an IVF-I8 handle.  The new rows pass through in blocks of option "int8_block_rows" (default 1M rows):
// byte test and extrema, coarse assignment, low bytes at the rows' insertion positions -- the float32 block is the only float32
// copy of corpus rows the device ever holds.  Then the window is fixed over the stored and the new rows, the bytes are put under
// it, one int8 gather files them in list order, and the panel space is rebuilt.  Everything is built in temporaries: an add
// that is refused (rows that are not byte-valued, no window for the union) leaves the handle as it was.
void i8_add(vdb_index_s *h, const float *x_host, int64_t n, int64_t id_base, const int32_t *given) {
    ivf_require(h->nlist > 0 && h->coarse, VDB_ERR_STATE, "no centroids: train or set them first");
    ivf_require(n >= 0 && (n == 0 || x_host), VDB_ERR_INVALID, "bad corpus");
    int64_t N0, N1;
    if (!ivf_add_range(h, n, id_base, N0, N1)) return;
    ivf_check_given(h, given, n);
    set_device(h->device);
    const int Dm = h->dim, D4 = h->D4;
    const int ks = ivf_i8_ksteps(Dm), pitch = ivf_i8_pitch(Dm), wpr = pitch / 4;
    VDB_HIP(hipDeviceSynchronize());
    hipStream_t st = nullptr;
    std::vector<int64_t> assign_new((size_t)n);
    DevBuf src8, rows8_new, ids_new, src_ids, dperm, doff;
    int cx = N0 ? h->i8_cx : 128, vmin = N0 ? h->i8_min : 1024, vmax = N0 ? h->i8_max : -1024;
    if (N1 > 0) {
        src8.reserve_exact((size_t)N1 * pitch);
        if (N0) VDB_HIP(hipMemcpy(src8.p, h->scan.rows8.p, (size_t)N0 * pitch, hipMemcpyDeviceToDevice));
    }
    if (n > 0) {
        const int64_t block_rows = std::min<int64_t>(n, h->opt.int8_block_rows > 0 ? h->opt.int8_block_rows : (int64_t)1 << 20);
        DevBuf blk, norms, dstat, dmm, dnew;
        blk.reserve((size_t)block_rows * D4 * sizeof(float));
        norms.reserve((size_t)block_rows * sizeof(float));
        dstat.reserve(sizeof(IndexStats));
        dmm.reserve(8);
        const int mm0[2] = {1024, -1024};
        VDB_HIP(hipMemsetAsync(dstat.p, 0, sizeof(IndexStats), st));
        VDB_HIP(hipMemcpy(dmm.p, mm0, 8, hipMemcpyHostToDevice));
        int64_t blocks = 0;
        std::vector<int64_t> assign_blk;
        for (int64_t r0 = 0; r0 < n; r0 += block_rows) {
            const int64_t nb = std::min<int64_t>(block_rows, n - r0);
            if (D4 != Dm) VDB_HIP(hipMemsetAsync(blk.p, 0, (size_t)nb * D4 * sizeof(float), st));
            upload_rows(h, blk.as<float>(), D4, x_host + (size_t)r0 * Dm, nb, Dm, st);
            blocks += h->last_upload_blocks;
            corpus_stats_kernel<<<dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st>>>(blk.as<float>(), nb, D4, norms.as<float>(),
                                                                                        dstat.as<IndexStats>());
            ivf_i8_ingest_kernel<<<dim3((unsigned)((nb * wpr + 255) / 256)), dim3(256), 0, st>>>(
                blk.as<float>(), nb, Dm, D4, pitch, reinterpret_cast<unsigned *>(src8.as<char>() + (size_t)(N0 + r0) * pitch), dmm.as<int>());
            VDB_HIP(hipGetLastError());
            if (given) {
                for (int64_t i = 0; i < nb; ++i) assign_new[(size_t)(r0 + i)] = given[r0 + i];
            } else {
                assign_blk.resize((size_t)nb);
                ivf_add_assign(h, blk.as<float>(), nb, dnew, assign_blk);
                std::copy(assign_blk.begin(), assign_blk.end(), assign_new.begin() + r0);
            }
            VDB_HIP(hipStreamSynchronize(st));      // (the block buffer is refilled by the next block)
        }
        h->last_upload_blocks = blocks;
        if (!given) sq8_release_coarse_ws(h);       // (the workspace of the assignment passes is given back, as on the coded kinds)
        IndexStats hs;
        int mm[2];
        VDB_HIP(hipMemcpy(&hs, dstat.p, sizeof(hs), hipMemcpyDeviceToHost));
        VDB_HIP(hipMemcpy(mm, dmm.p, 8, hipMemcpyDeviceToHost));
        const bool all_integer = !hs.nonfinite && !hs.not_integer;
        ivf_require(ivf_i8_window(mm[0], mm[1], all_integer) >= 0, VDB_ERR_INVALID,
                    "IVF-I8 files byte-valued rows only (every value an integer in 0..255 or in -128..127): these rows are not, nothing was added");
        vmin = std::min(vmin, mm[0]);
        vmax = std::max(vmax, mm[1]);
        cx = ivf_i8_window(vmin, vmax, true);
        ivf_require(cx >= 0, VDB_ERR_INVALID,
                    "IVF-I8: no byte window (0..255 or -128..127) holds the stored rows together with the new ones, nothing was added");
        // the bytes under the window: the stored ones change sides when the window does, the new low bytes when it is the u8 one
        if (N0 && cx != h->i8_cx)
            ivf_i8_flip_kernel<<<dim3((unsigned)((N0 * wpr + 255) / 256)), dim3(256), 0, st>>>(src8.as<unsigned>(), N0 * wpr);
        if (cx == 128)
            ivf_i8_flip_kernel<<<dim3((unsigned)((n * wpr + 255) / 256)), dim3(256), 0, st>>>(src8.as<unsigned>() + (size_t)N0 * wpr, n * wpr);
        VDB_HIP(hipGetLastError());
    }
    const std::vector<int64_t> offsets_before = h->ivf_offsets_host;
    try {
        if (N1 > 0) {
            ivf_add_lists(h, assign_new, N0, src_ids, dperm, doff);
            rows8_new.reserve_exact((size_t)N1 * pitch);
            ids_new.reserve_exact((size_t)N1 * 8);
            sq8_gather_kernel<<<dim3((unsigned)((N1 * wpr + 255) / 256)), dim3(256), 0, st>>>(
                src8.as<unsigned char>(), dperm.as<int32_t>(), N1, pitch, id_base, N0 ? src_ids.as<int64_t>() : nullptr,
                rows8_new.as<unsigned char>(), ids_new.as<int64_t>());
            VDB_HIP(hipGetLastError());
            VDB_HIP(hipDeviceSynchronize());
        }
    } catch (...) {
        h->ivf_offsets_host = offsets_before;
        throw;
    }
    // ---- commit ----
    h->ivf_built = false;
    h->built = false;
    i8_take(h->scan.rows8, rows8_new);
    i8_take(h->lists.ivf_ids, ids_new);
    h->rows8_pitch = pitch;
    h->i8_ks = ks;
    h->i8_cx = cx;
    h->i8_min = vmin;
    h->i8_max = vmax;
    ivf_add_finish(h, assign_new, N0, id_base);
    i8_build_panel_space(h);
    h->ivf_built = true;
}

// the fp16 panels of the whole panel space for this batch, converted from panels8 (workspace; the kernel returns at once when the
// int8 scan serves the batch)
const half8 *ivf_i8_panels(vdb_index_s *h, const QueryBatchInfo *info, hipStream_t st) {
    const int64_t ntiles = h->ivf_pspans * kIvfTilesPerSpan;
    h->ws.sq8_panels.reserve((size_t)ivf_i8_slab_bytes(h->ivf_pspans * kIvfSpanRows, h->dim));
    const int64_t threads = ntiles * h->ksteps * 64;
    ivf_panels_from_i8_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(
        h->scan.panels8.as<int4v>(), h->i8_ks, h->ksteps, h->i8_cx, h->sx, ntiles, h->dim, h->lists.ivf_span_valid.as<int32_t>(), info,
        h->ws.sq8_panels.as<half8>());
    VDB_HIP(hipGetLastError());
    return h->ws.sq8_panels.as<half8>();
}

// lsh.inc -- host side of the sign-LSH codes (kernels: lsh.hpp): projection, encoding adds, candidate scan, search; and the
// host driver of the counting select (lsh_select.hpp) that the hash-table LSH (lsh_tables.inc) shares.
// Included by vdbhip.hip; the handle's LSH state lives in vdb_index_s (lsh_*).

namespace {

inline bool lsh_on(const vdb_index_s *h) { return h->lsh_nbits > 0; }

// What the LSH entry points admit.  A projection goes onto a flat handle (resident float32 rows in insertion order on ONE
// device; no option that drops them: refuse_options_set).  The candidate / search calls refuse the kinds that keep no float32
// rows or stay another flat structure; an IVF-Flat or SQ8 handle is told "no projection" by lsh_require_ready, as a flat one is.
constexpr unsigned kBecomesLsh = kFlat | kLsh, kLshSearchCalls = kFlat | kLsh | kIvfFlat | kIvfSq8;
constexpr unsigned kLshGetCodes = kLshSearchCalls | kKnng;      // (a k-NN graph handle is told "no projection", not that it stays what it is)

// n rows of x (device, `pitch` floats apart) -> codes (n x lsh_wp words)
void lsh_encode(vdb_index_s *h, const float *x, int64_t n, int64_t pitch, uint32_t *codes, hipStream_t st) {
    if (n <= 0) return;
    VDB_HIP(hipMemsetAsync(codes, 0, (size_t)n * h->lsh_wp * sizeof(uint32_t), st));
    const int64_t items = (n + kLshEncRows - 1) / kLshEncRows * ((h->lsh_nbits + 63) / 64);
    lsh_encode_kernel<<<dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st>>>(x, n, h->dim, pitch, h->kept.lsh_rt.as<float>(), h->lsh_nbits,
                                                                             h->lsh_wp, codes);
    VDB_HIP(hipGetLastError());
}

// codes of the rows [r0, N) of h->rows.x32 (rows below r0 keep theirs): called behind every add, and by set_projection with r0 = 0
void lsh_encode_rows(vdb_index_s *h, int64_t r0, hipStream_t st) {
    if (!lsh_on(h)) return;
    if (r0 > h->lsh_rows || r0 > h->N) r0 = 0;
    h->lsh_rows = 0;
    if (h->N == 0 || !h->built) return;
    const size_t row_bytes = (size_t)h->lsh_wp * sizeof(uint32_t);
    if (r0 == 0) h->codes.lsh_codes.reserve((size_t)h->N * row_bytes);
    else h->codes.lsh_codes.grow((size_t)h->N * row_bytes, (size_t)r0 * row_bytes);
    lsh_encode(h, h->rows.x32.as<float>() + (size_t)r0 * h->D4, h->N - r0, h->D4, h->codes.lsh_codes.as<uint32_t>() + (size_t)r0 * h->lsh_wp, st);
    VDB_HIP(hipStreamSynchronize(st));
    h->lsh_rows = h->N;
}

void lsh_require_ready(vdb_index_s *h, const char *what) {
    if (!lsh_on(h)) throw Error(VDB_ERR_STATE, std::string(what) + ": no projection (call vdb_lsh_set_projection first)");
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + " is not available with option 'graph'");
    if (h->lsh_rows != h->N) throw Error(VDB_ERR_STATE, "the LSH codes do not cover the rows of this index (a failed add?): vdb_reset and add again");
}

// ---- the counting select (lsh_select.hpp), shared with lsh_tables.inc --------------------------------------------------------
// what tells the two kinds apart on the host
struct LshKind {
    int path;                        // VDB_PATH_LSH | VDB_PATH_LSHT
    const uint32_t *codes;           // [N][kw]
    int kw, T, wp, hb, qtile;        // LshSelArgs
    bool want_all;                   // a query wants min(ncand, N) candidates: every row has a score
    void (*encode)(vdb_index_s *, const float *, int64_t, int64_t, uint32_t *, hipStream_t);
    void (*sample)(const LshSelArgs &, dim3, hipStream_t);
    void (*scan0)(const LshSelArgs &, dim3, hipStream_t);
    void (*scan1)(const LshSelArgs &, dim3, hipStream_t);
    int row_tile;                    // rows per workgroup of the scans
};

#define LSH_DISPATCH(wp, ...)                                  \
    switch (wp) {                                              \
        case 1: { constexpr int WP = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int WP = 2; __VA_ARGS__; } break;  \
        case 4: { constexpr int WP = 4; __VA_ARGS__; } break;  \
        case 8: { constexpr int WP = 8; __VA_ARGS__; } break;  \
        case 16: { constexpr int WP = 16; __VA_ARGS__; } break; \
        default: { constexpr int WP = 32; __VA_ARGS__; } break; \
    }

template <int MODE>
void launch_lsh_scan(const LshSelArgs &a, dim3 grid, hipStream_t st) {
    LSH_DISPATCH(a.kw, (lsh_scan_kernel<MODE, WP><<<grid, dim3(256), 0, st>>>(a)));
}

void launch_lsh_sample(const LshSelArgs &a, dim3 grid, hipStream_t st) {
    LSH_DISPATCH(a.kw, (lsh_sample_kernel<WP><<<grid, dim3(256), 0, st>>>(a)));
}

LshKind lsh_kind(vdb_index_s *h) {
    return {VDB_PATH_LSH, h->codes.lsh_codes.as<uint32_t>(), h->lsh_wp, 0, h->lsh_wp, h->lsh_nbits + 1, kLshQTile, true,
            lsh_encode, launch_lsh_sample, launch_lsh_scan<0>, launch_lsh_scan<1>, kLshRowTile};
}

constexpr size_t kLshListBudget = (size_t)512 << 20;     // bytes of per-query lists per pass: larger batches go in query chunks
constexpr size_t kLshCandBudget = (size_t)256 << 20;     // bytes of candidate ids + scores between scan and re-rank

// candidates of nq queries (device) -> score / ids (device, (nq, ncand)); tslot / mark0: timing (events 0 and 1 around the scans);
// empty: [0] the count, [1 ..] the numbers of the queries without a candidate (null: not listed)
void lsh_candidates_core(vdb_index_s *h, const LshKind &kd, const float *dq, int64_t nq, int ncand, int32_t *score, int64_t *ids,
                         hipStream_t st, long tslot, bool mark0, int32_t *empty) {
    const int kw = kd.kw;
    const int c = (int)std::min<int64_t>(ncand, h->N);
    int cap = 1;
    while (cap < std::min<int64_t>(4 * (int64_t)c + 1024, h->N)) cap <<= 1;
    const int64_t nqc = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 1 << 20), (int64_t)(kLshListBudget / ((size_t)cap * 8))));
    h->lsh_ws.lsh_qcodes.reserve((size_t)nq * kw * sizeof(uint32_t));
    h->lsh_ws.lsh_hist.reserve((size_t)nqc * kd.hb * sizeof(int));
    h->lsh_ws.lsh_small.reserve((size_t)nqc * 7 * sizeof(int));
    h->lsh_ws.lsh_list.reserve((size_t)nqc * cap * sizeof(unsigned long long));
    kd.encode(h, dq, nq, h->dim, h->lsh_ws.lsh_qcodes.as<uint32_t>(), st);
    LshSelArgs a{};
    a.codes = kd.codes;
    a.n = h->N;
    a.kw = kw;
    a.T = kd.T;
    a.wp = kd.wp;
    a.hb = kd.hb;
    a.want = kd.want_all ? c : ncand;
    a.ncand = ncand;
    a.cap = cap;
    a.qtile = kd.qtile;
    a.sample_n = std::min<int64_t>(h->N, kLshSampleMax);                       // (N <= the sample: all rows, exact histogram)
    a.sample_stride = a.sample_n == h->N ? 256 : h->N / (kLshSampleMax / 256);  // first rows of consecutive 256-row runs
    a.force_fallback = h->opt.lsh_force_fallback;
    a.id_base = h->id_base;
    a.hist = h->lsh_ws.lsh_hist.as<int>();
    a.thi = h->lsh_ws.lsh_small.as<int>();
    a.tq = a.thi + nqc;
    a.cnt = a.tq + nqc;
    a.flag = a.cnt + nqc;
    a.tsel = a.flag + nqc;
    a.msel = a.tsel + nqc;
    a.csel = a.msel + nqc;
    a.scanned0 = a.sample_n != a.n;
    a.list = h->lsh_ws.lsh_list.as<unsigned long long>();
    a.stat = h->lsh_ws.lsh_stat.as<unsigned long long>();
    a.empty_count = empty;
    a.empty_list = empty ? empty + 1 : nullptr;
    for (int64_t q0 = 0; q0 < nq; q0 += nqc) {
        a.nq = std::min<int64_t>(nqc, nq - q0);
        a.q_base = q0;
        a.qcodes = h->lsh_ws.lsh_qcodes.as<uint32_t>() + (size_t)q0 * kw;
        a.out_score = score + (size_t)q0 * ncand;
        a.out_ids = ids + (size_t)q0 * ncand;
        const dim3 scan_grid((unsigned)((a.n + kd.row_tile - 1) / kd.row_tile), (unsigned)((a.nq + a.qtile - 1) / a.qtile));
        kd.sample(a, dim3((unsigned)((a.nq + kLshSampleQ - 1) / kLshSampleQ)), st);
        VDB_HIP(hipGetLastError());
        if (mark0 && q0 == 0) timing_mark(h, tslot, 0, st);
        if (a.scanned0) {
            kd.scan0(a, scan_grid, st);
            VDB_HIP(hipGetLastError());
        }
        lsh_threshold_kernel<<<dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, st>>>(a);
        VDB_HIP(hipGetLastError());
        kd.scan1(a, scan_grid, st);
        VDB_HIP(hipGetLastError());
        timing_mark(h, tslot, 1, st);
        if (a.T) lsh_select_kernel<true><<<dim3((unsigned)a.nq), dim3(256), 0, st>>>(a);
        else lsh_select_kernel<false><<<dim3((unsigned)a.nq), dim3(256), 0, st>>>(a);
        VDB_HIP(hipGetLastError());
    }
}

void lsh_check_args(const void *q, int64_t nq, int ncand, const void *o1, const void *o2) {
    if (ncand < 1 || ncand > kLshMaxCand) throw Error(VDB_ERR_INVALID, "ncand must be in [1, 65536]");
    if (nq < 0) throw Error(VDB_ERR_INVALID, "negative query count");
    if (nq > 0 && (!q || !o1 || !o2)) throw Error(VDB_ERR_INVALID, "null pointer");
}

void lsh_begin_call(vdb_index_s *h, int path, int64_t nq, hipStream_t st) {
    h->lsh_ws.lsh_stat.reserve((size_t)kStatShards * kStatStride * sizeof(unsigned long long));
    VDB_HIP(hipMemsetAsync(h->lsh_ws.lsh_stat.p, 0, (size_t)kStatShards * kStatStride * sizeof(unsigned long long), st));
    h->last.last_nq = nq;
    h->last.last_path = path;
}

void lsh_candidates_impl(vdb_index_s *h, const LshKind &kd, const float *dq, int64_t nq, int ncand, int32_t *score, int64_t *ids,
                         hipStream_t st) {
    lsh_begin_call(h, kd.path, nq, st);
    const long tslot = timing_begin(h, st);
    lsh_candidates_core(h, kd, dq, nq, ncand, score, ids, st, tslot, true, nullptr);
    timing_mark(h, tslot, 2, st);
}

// the same from and to host memory
void lsh_candidates_staged(vdb_index_s *h, const LshKind &kd, const float *q_host, int64_t nq, int ncand, int32_t *score, int64_t *ids) {
    DevBuf ds, di;
    h->ws.stage_q.reserve((size_t)nq * h->dim * sizeof(float));
    ds.reserve((size_t)nq * ncand * sizeof(int32_t));
    di.reserve((size_t)nq * ncand * sizeof(int64_t));
    hipStream_t st = nullptr;
    VDB_HIP(hipMemcpyAsync(h->ws.stage_q.p, q_host, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
    lsh_candidates_impl(h, kd, h->ws.stage_q.as<float>(), nq, ncand, ds.as<int32_t>(), di.as<int64_t>(), st);
    VDB_HIP(hipMemcpyAsync(score, ds.p, (size_t)nq * ncand * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    VDB_HIP(hipMemcpyAsync(ids, di.p, (size_t)nq * ncand * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
}

// query -> code -> top-ncand of the select -> exact top-k (rerank_kernel), in query chunks that bound the candidate buffers;
// fallback: the queries of a chunk without a candidate then take the exhaustive exact scan, from the device-side list the
// select wrote
void lsh_search_impl(vdb_index_s *h, const LshKind &kd, const float *dq, int64_t nq, int k, int ncand, int fallback, float *D, int64_t *I,
                     hipStream_t st) {
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    const int64_t nqs = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(kLshCandBudget / ((size_t)ncand * 12))));
    h->lsh_ws.lsh_cand_i.reserve((size_t)nqs * ncand * sizeof(int64_t));
    h->lsh_ws.lsh_cand_h.reserve((size_t)nqs * ncand * sizeof(int32_t));
    if (fallback) h->lsh_ws.lsht_empty.reserve((size_t)(nqs + 1) * sizeof(int32_t));
    lsh_begin_call(h, kd.path, nq, st);
    const long tslot = timing_begin(h, st);
    for (int64_t q0 = 0; q0 < nq; q0 += nqs) {
        const int64_t n = std::min<int64_t>(nqs, nq - q0);
        const float *qs = dq + (size_t)q0 * h->dim;
        int32_t *empty = fallback ? h->lsh_ws.lsht_empty.as<int32_t>() : nullptr;
        if (empty) VDB_HIP(hipMemsetAsync(empty, 0, sizeof(int32_t), st));
        lsh_candidates_core(h, kd, qs, n, ncand, h->lsh_ws.lsh_cand_h.as<int32_t>(), h->lsh_ws.lsh_cand_i.as<int64_t>(), st, tslot, q0 == 0, empty);
        rerank_device_impl(h, qs, n, h->lsh_ws.lsh_cand_i.as<int64_t>(), ncand, k, D + (size_t)q0 * k, I + (size_t)q0 * k, st);
        if (empty) {
            // (rerank_device_impl left the chunk's queries padded to D4 in ws.qpad when D4 != dim)
            RefineFullArgs fa{};
            fa.c = flat_rows(h, h->D4 != h->dim ? h->ws.qpad.as<float>() : qs, k);
            fa.qlist = empty + 1;
            fa.count_ptr = empty;
            fa.S = 1;
            fa.rows_per_split = h->N;
            fa.D = D + (size_t)q0 * k;
            fa.I = I + (size_t)q0 * k;
            launch_refine_full(fa, n, st);
        }
    }
    timing_mark(h, tslot, 2, st);
}

}  // namespace

extern "C" {

int vdb_lsh_set_projection(vdb_handle hh, int nbits, const float *proj_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_set_projection", kBecomesLsh);
        refuse_options_set(h, "vdb_lsh_set_projection", kLsh);
        if (nbits < 32 || nbits > kLshMaxBits || nbits % 32) throw Error(VDB_ERR_INVALID, "nbits must be a multiple of 32 in [32, 1024]");
        if (!proj_host) throw Error(VDB_ERR_INVALID, "null projection pointer");
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        graph_reset(h);
        const int D = h->dim;
        h->lsh_proj.assign(proj_host, proj_host + (size_t)nbits * D);
        std::vector<float> rt((size_t)D * nbits);
        for (int j = 0; j < nbits; ++j)
            for (int d = 0; d < D; ++d) rt[(size_t)d * nbits + j] = proj_host[(size_t)j * D + d];
        h->lsh_nbits = nbits;
        h->lsh_wp = 1;
        while (h->lsh_wp < nbits / 32) h->lsh_wp <<= 1;
        h->lsh_rows = 0;
        h->codes.lsh_codes.release();
        h->kept.lsh_rt.reserve_exact(rt.size() * sizeof(float));
        VDB_HIP(hipMemcpy(h->kept.lsh_rt.p, rt.data(), rt.size() * sizeof(float), hipMemcpyHostToDevice));
        lsh_encode_rows(h, 0, nullptr);
    });
}

int vdb_lsh_get_projection(vdb_handle hh, int *nbits, float *proj_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_get_projection", kAnyKind);
        if (!nbits) throw Error(VDB_ERR_INVALID, "null pointer");
        *nbits = h->lsh_nbits;                     // (0 on every other kind)
        if (proj_host && *nbits > 0) memcpy(proj_host, h->lsh_proj.data(), h->lsh_proj.size() * sizeof(float));
    });
}

int vdb_lsh_get_codes(vdb_handle hh, uint32_t *codes_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_get_codes", kLshGetCodes);
        if (!lsh_on(h)) throw Error(VDB_ERR_STATE, "vdb_lsh_get_codes: no projection (call vdb_lsh_set_projection first)");
        if (!h->built || h->N == 0 || h->lsh_rows != h->N) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
        if (!codes_host) throw Error(VDB_ERR_INVALID, "null pointer");
        set_device(h->device);
        const int w = h->lsh_nbits / 32, wp = h->lsh_wp;
        if (w == wp) {
            VDB_HIP(hipMemcpy(codes_host, h->codes.lsh_codes.p, (size_t)h->N * w * sizeof(uint32_t), hipMemcpyDeviceToHost));
            return;
        }
        std::vector<uint32_t> tmp((size_t)h->N * wp);
        VDB_HIP(hipMemcpy(tmp.data(), h->codes.lsh_codes.p, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < h->N; ++r) memcpy(codes_host + (size_t)r * w, tmp.data() + (size_t)r * wp, (size_t)w * sizeof(uint32_t));
    });
}

int vdb_lsh_candidates_device(vdb_handle hh, const float *q_dev, int64_t nq, int ncand, int32_t *ham_dev, int64_t *ids_dev,
                              void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_candidates_device", kLshSearchCalls);
        lsh_require_ready(h, "vdb_lsh_candidates_device");
        lsh_check_args(q_dev, nq, ncand, ham_dev, ids_dev);
        if (nq == 0) return;
        set_device(h->device);
        lsh_candidates_impl(h, lsh_kind(h), q_dev, nq, ncand, ham_dev, ids_dev, as_stream(stream));
    });
}

int vdb_lsh_candidates(vdb_handle hh, const float *q_host, int64_t nq, int ncand, int32_t *ham, int64_t *ids) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_candidates", kLshSearchCalls);
        lsh_require_ready(h, "vdb_lsh_candidates");
        lsh_check_args(q_host, nq, ncand, ham, ids);
        if (nq == 0) return;
        set_device(h->device);
        lsh_candidates_staged(h, lsh_kind(h), q_host, nq, ncand, ham, ids);
    });
}

int vdb_lsh_search_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, int ncand, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_search_device", kLshSearchCalls);
        lsh_require_ready(h, "vdb_lsh_search_device");
        lsh_check_args(q_dev, nq, ncand, D_dev, I_dev);
        if (nq == 0) return;
        set_device(h->device);
        lsh_search_impl(h, lsh_kind(h), q_dev, nq, k, ncand, 0, D_dev, I_dev, as_stream(stream));
    });
}

int vdb_lsh_search(vdb_handle hh, const float *q_host, int64_t nq, int k, int ncand, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsh_search", kLshSearchCalls);
        lsh_require_ready(h, "vdb_lsh_search");
        lsh_check_args(q_host, nq, ncand, D, I);
        if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
        if (nq == 0) return;
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            lsh_search_impl(h, lsh_kind(h), dq, nq, k, ncand, 0, dD, dI, st);
        });
    });
}

}  // extern "C"

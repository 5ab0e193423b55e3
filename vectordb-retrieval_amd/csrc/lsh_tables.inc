// lsh_tables.inc -- host side of the hash-table LSH (kernels: lsh_tables.hpp): tables, keying adds, candidate scan, search.
// Included by vdbhip.hip; the handle's state lives in vdb_index_s (lsht_*), the per-search buffers are those of the sign-LSH
// calls (lsh_ws: a handle is never both kinds).

namespace {

inline bool lsht_on(const vdb_index_s *h) { return h->lsht_T > 0; }

// Tables go onto a flat handle, as a projection does (lsh.inc); every other kind refuses the calls outright.
constexpr unsigned kLshtCalls = kFlat | kLsht;

// stored words per table: the contract's words rounded up to a width the scan is compiled for
int lsht_stored_words(int W) {
    for (int wp : {1, 2, 3, 4, 6, 8, 12, 16})
        if (W <= wp) return wp;
    return 16;
}

// WP = stored words per table, TMAX = the most tables T * W <= kLshtMaxWords allows at the narrowest W stored as WP
#define LSHT_DISPATCH(wp, ...)                                      \
    switch (wp) {                                                   \
        case 1: { constexpr int WP = 1, TMAX = 32; __VA_ARGS__; } break;   \
        case 2: { constexpr int WP = 2, TMAX = 32; __VA_ARGS__; } break;   \
        case 3: { constexpr int WP = 3, TMAX = 32; __VA_ARGS__; } break;   \
        case 4: { constexpr int WP = 4, TMAX = 32; __VA_ARGS__; } break;   \
        case 6: { constexpr int WP = 6, TMAX = 25; __VA_ARGS__; } break;   \
        case 8: { constexpr int WP = 8, TMAX = 18; __VA_ARGS__; } break;   \
        case 12: { constexpr int WP = 12, TMAX = 14; __VA_ARGS__; } break; \
        default: { constexpr int WP = 16, TMAX = 9; __VA_ARGS__; } break;  \
    }

// n rows of x (device, `pitch` floats apart) -> keys (n x lsht_kw words)
void lsht_key(vdb_index_s *h, const float *x, int64_t n, int64_t pitch, uint32_t *keys, hipStream_t st) {
    if (n <= 0) return;
    VDB_HIP(hipMemsetAsync(keys, 0, (size_t)n * h->lsht_kw * sizeof(uint32_t), st));
    LshtKeyArgs a{};
    a.x = x;
    a.n = n;
    a.pitch = pitch;
    a.dim = h->dim;
    a.pt = h->kept.lsht_pt.as<float>();
    a.off = h->kept.lsht_off.as<float>();
    a.T = h->lsht_T;
    a.H = h->lsht_H;
    a.mode = h->lsht_mode;
    a.wp = h->lsht_wp;
    a.kw = h->lsht_kw;
    a.w = (double)h->lsht_width;
    a.keys = keys;
    const int chunks = a.mode == 0 ? a.T : (a.T * a.H + 63) / 64;
    const int64_t items = (n + kLshEncRows - 1) / kLshEncRows * chunks;
    lsht_key_kernel<<<dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st>>>(a);
    VDB_HIP(hipGetLastError());
}

// keys of the rows [r0, N) of h->rows.x32 (rows below r0 keep theirs): called behind every add, and by set_tables with r0 = 0
void lsht_key_rows(vdb_index_s *h, int64_t r0, hipStream_t st) {
    if (!lsht_on(h)) return;
    if (r0 > h->lsht_rows || r0 > h->N) r0 = 0;
    h->lsht_rows = 0;
    if (h->N == 0 || !h->built) return;
    const size_t row_bytes = (size_t)h->lsht_kw * sizeof(uint32_t);
    if (r0 == 0) h->codes.lsht_keys.reserve((size_t)h->N * row_bytes);
    else h->codes.lsht_keys.grow((size_t)h->N * row_bytes, (size_t)r0 * row_bytes);
    lsht_key(h, h->rows.x32.as<float>() + (size_t)r0 * h->D4, h->N - r0, h->D4, h->codes.lsht_keys.as<uint32_t>() + (size_t)r0 * h->lsht_kw, st);
    VDB_HIP(hipStreamSynchronize(st));
    h->lsht_rows = h->N;
}

void lsht_require_ready(vdb_index_s *h, const char *what, bool search_call) {
    if (!lsht_on(h)) throw Error(VDB_ERR_STATE, std::string(what) + ": no hash tables (call vdb_lsht_set_tables first)");
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (search_call && h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + " is not available with option 'graph'");
    if (h->lsht_rows != h->N) throw Error(VDB_ERR_STATE, "the LSH table keys do not cover the rows of this index (a failed add?): vdb_reset and add again");
}

template <int MODE>
void launch_lsht_scan(const LshSelArgs &a, dim3 grid, hipStream_t st) {
    LSHT_DISPATCH(a.wp, (lsht_scan_kernel<MODE, WP, TMAX><<<grid, dim3(256), 0, st>>>(a)));
}

void launch_lsht_sample(const LshSelArgs &a, dim3 grid, hipStream_t st) {
    LSHT_DISPATCH(a.wp, (lsht_sample_kernel<WP, TMAX><<<grid, dim3(256), 0, st>>>(a)));
}

// the select of lsh.inc over the classes of the table keys
LshKind lsht_kind(vdb_index_s *h) {
    return {VDB_PATH_LSHT, h->codes.lsht_keys.as<uint32_t>(), h->lsht_kw, h->lsht_T, h->lsht_wp, h->lsht_T * h->lsht_T,
            std::min(256, kLshtLdsWords / h->lsht_kw), false,
            lsht_key, launch_lsht_sample, launch_lsht_scan<0>, launch_lsht_scan<1>, kLshtRowTile};
}

}  // namespace

extern "C" {

int vdb_lsht_set_tables(vdb_handle hh, int num_tables, int hash_size, int mode, const float *proj_host, const float *offsets_host,
                        float bucket_width) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_set_tables", kLshtCalls);
        refuse_options_set(h, "vdb_lsht_set_tables", kLsht);
        const int T = num_tables, H = hash_size;
        if (mode != 0 && mode != 1) throw Error(VDB_ERR_INVALID, "mode must be 0 (sign keys) or 1 (E2 bucket keys)");
        if (T < 1 || T > kLshtMaxTables) throw Error(VDB_ERR_INVALID, "num_tables must be in [1, 32]");
        if (H < 1 || H > (mode == 0 ? 64 : 16)) throw Error(VDB_ERR_INVALID, mode == 0 ? "hash_size must be in [1, 64] for sign keys" : "hash_size must be in [1, 16] for E2 keys");
        const int W = mode == 0 ? (H + 31) / 32 : H;
        if (T * W > kLshtMaxWords) throw Error(VDB_ERR_INVALID, "num_tables * words per table key must be at most 128");
        if (!proj_host) throw Error(VDB_ERR_INVALID, "null projection pointer");
        if (mode == 1 && !offsets_host) throw Error(VDB_ERR_INVALID, "null offsets pointer");
        if (mode == 1 && (!(bucket_width > 0.f) || isinf(bucket_width))) throw Error(VDB_ERR_INVALID, "bucket_width must be positive");
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        graph_reset(h);
        const int D = h->dim, TH = T * H;
        h->lsht_proj.assign(proj_host, proj_host + (size_t)TH * D);
        if (mode == 1) h->lsht_off.assign(offsets_host, offsets_host + TH);
        else h->lsht_off.assign((size_t)TH, 0.f);
        std::vector<float> pt((size_t)D * TH);
        for (int j = 0; j < TH; ++j)
            for (int d = 0; d < D; ++d) pt[(size_t)d * TH + j] = proj_host[(size_t)j * D + d];
        h->lsht_T = T;
        h->lsht_H = H;
        h->lsht_mode = mode;
        h->lsht_W = W;
        h->lsht_wp = lsht_stored_words(W);
        h->lsht_kw = T * h->lsht_wp;
        h->lsht_width = mode == 1 ? bucket_width : 0.f;
        h->lsht_rows = 0;
        h->codes.lsht_keys.release();
        h->kept.lsht_pt.reserve_exact(pt.size() * sizeof(float));
        h->kept.lsht_off.reserve_exact((size_t)TH * sizeof(float));
        VDB_HIP(hipMemcpy(h->kept.lsht_pt.p, pt.data(), pt.size() * sizeof(float), hipMemcpyHostToDevice));
        VDB_HIP(hipMemcpy(h->kept.lsht_off.p, h->lsht_off.data(), (size_t)TH * sizeof(float), hipMemcpyHostToDevice));
        lsht_key_rows(h, 0, nullptr);
    });
}

int vdb_lsht_get_tables(vdb_handle hh, int *num_tables, int *hash_size, int *mode, float *proj_host, float *offsets_host,
                        float *bucket_width) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_get_tables", kAnyKind);
        if (!num_tables) throw Error(VDB_ERR_INVALID, "null pointer");
        *num_tables = h->lsht_T;                   // (0 on every other kind)
        if (hash_size) *hash_size = h->lsht_H;
        if (mode) *mode = h->lsht_mode;
        if (bucket_width) *bucket_width = h->lsht_width;
        if (h->lsht_T == 0) return;
        if (proj_host) memcpy(proj_host, h->lsht_proj.data(), h->lsht_proj.size() * sizeof(float));
        if (offsets_host && h->lsht_mode == 1) memcpy(offsets_host, h->lsht_off.data(), h->lsht_off.size() * sizeof(float));
    });
}

int vdb_lsht_get_keys(vdb_handle hh, uint32_t *keys_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_get_keys", kLshtCalls);
        lsht_require_ready(h, "vdb_lsht_get_keys", false);
        if (!keys_host) throw Error(VDB_ERR_INVALID, "null pointer");
        set_device(h->device);
        const int T = h->lsht_T, W = h->lsht_W, wp = h->lsht_wp;
        if (W == wp) {
            VDB_HIP(hipMemcpy(keys_host, h->codes.lsht_keys.p, (size_t)h->N * T * W * sizeof(uint32_t), hipMemcpyDeviceToHost));
            return;
        }
        std::vector<uint32_t> tmp((size_t)h->N * h->lsht_kw);
        VDB_HIP(hipMemcpy(tmp.data(), h->codes.lsht_keys.p, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < h->N; ++r)
            for (int t = 0; t < T; ++t)
                memcpy(keys_host + ((size_t)r * T + t) * W, tmp.data() + ((size_t)r * T + t) * wp, (size_t)W * sizeof(uint32_t));
    });
}

int vdb_lsht_candidates_device(vdb_handle hh, const float *q_dev, int64_t nq, int ncand, int32_t *votes_dev, int64_t *ids_dev,
                               void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_candidates_device", kLshtCalls);
        lsht_require_ready(h, "vdb_lsht_candidates_device", true);
        lsh_check_args(q_dev, nq, ncand, votes_dev, ids_dev);
        if (nq == 0) return;
        set_device(h->device);
        lsh_candidates_impl(h, lsht_kind(h), q_dev, nq, ncand, votes_dev, ids_dev, as_stream(stream));
    });
}

int vdb_lsht_candidates(vdb_handle hh, const float *q_host, int64_t nq, int ncand, int32_t *votes, int64_t *ids) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_candidates", kLshtCalls);
        lsht_require_ready(h, "vdb_lsht_candidates", true);
        lsh_check_args(q_host, nq, ncand, votes, ids);
        if (nq == 0) return;
        set_device(h->device);
        lsh_candidates_staged(h, lsht_kind(h), q_host, nq, ncand, votes, ids);
    });
}

int vdb_lsht_search_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, int ncand, int fallback, float *D_dev, int64_t *I_dev,
                           void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_search_device", kLshtCalls);
        lsht_require_ready(h, "vdb_lsht_search_device", true);
        lsh_check_args(q_dev, nq, ncand, D_dev, I_dev);
        if (fallback != 0 && fallback != 1) throw Error(VDB_ERR_INVALID, "fallback must be 0 or 1");
        if (nq == 0) return;
        set_device(h->device);
        lsh_search_impl(h, lsht_kind(h), q_dev, nq, k, ncand, fallback, D_dev, I_dev, as_stream(stream));
    });
}

int vdb_lsht_search(vdb_handle hh, const float *q_host, int64_t nq, int k, int ncand, int fallback, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_lsht_search", kLshtCalls);
        lsht_require_ready(h, "vdb_lsht_search", true);
        lsh_check_args(q_host, nq, ncand, D, I);
        if (fallback != 0 && fallback != 1) throw Error(VDB_ERR_INVALID, "fallback must be 0 or 1");
        if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
        if (nq == 0) return;
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            lsh_search_impl(h, lsht_kind(h), dq, nq, k, ncand, fallback, dD, dI, st);
        });
    });
}

}  // extern "C"

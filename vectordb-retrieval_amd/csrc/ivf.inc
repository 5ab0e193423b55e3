// ivf.inc -- host side of IVF-Flat (included at the end of vdbhip.hip).
//
// Replaces what the reference delegates to faiss.index_factory(d, "IVF<nlist>,Flat", metric):
//   train  -> Lloyd k-means on <= max_points_per_centroid*nlist sampled rows      (modular.py:281-282)
//   add    -> assign every row to its nearest centroid, build CSR lists            (modular.py:283)
//   nprobe -> runtime parameter                                                     (modular.py:269-275, 437-441)
//   search -> coarse top-nprobe over the centroids, exact scan of the probed lists  (modular.py:544)
// Conventions: as vdb_search (squared L2 ascending / raw IP descending, -1 / +-FLT_MAX padding).
// All distance arithmetic is the canonical float64 of refine.hpp, so results equal a brute-force search
// restricted to the probed lists, bit for bit (tests/test_gpu_ivf.py vs oracle/ivf_oracle.c).

#include <numeric>
#include <random>

namespace {

void ivf_require(bool cond, int code, const char *msg) {
    if (!cond) throw Error(code, msg);
}

// What the IVF entry points admit (Kind, vdbhip.hip).  Every one of them refuses a flat PQ handle; on any other handle without
// centroids they answer VDB_ERR_STATE themselves (a sign-LSH or k-NN graph handle too: recorded behaviour, nobody chose it --
// DESIGN.md 4.11).  The calls that make a handle an IVF index also refuse the kinds that stay flat.  The calls of one codec
// refuse the handles that can never carry it, and are a state error on the rest.
constexpr unsigned kIvfCalls = kAnyKind & ~kPq, kBecomesIvf = kFlat | kIvf | kMulti;
inline void admit_sq8(const vdb_index_s *h, const char *what) {
    admit(h, what, kAnyKind & ~(kPq | kMulti | kIvfPq | kIvfI8));
    admit(h, what, kIvfSq8, VDB_ERR_STATE, ": not an SQ8 index (vdb_ivf_set_codec(h, 1) on an empty handle)");
}
inline void admit_ivf_i8(const vdb_index_s *h, const char *what) {      // (as admit_sq8: S where vdb_ivf_get_codes answers S, U where it answers U)
    admit(h, what, kAnyKind & ~(kPq | kMulti | kIvfPq));
    admit(h, what, kIvfI8, VDB_ERR_STATE, ": not an IVF-I8 index (vdb_ivf_set_codec(h, 3) on an empty handle)");
}
inline void admit_ivfpq(const vdb_index_s *h, const char *what) {
    admit(h, what, kAnyKind & ~(kPq | kMulti | kIvfI8));
    admit(h, what, kIvfPq, VDB_ERR_STATE, ": not an IVF-PQ index (vdb_ivf_set_codec(h, 2) on an empty handle)");
}

// (re)build the flat index over the current centroids
void ivf_install_centroids(vdb_index_s *h, const float *c_host, int nlist) {
    h->ivf_centroids.assign(c_host, c_host + (size_t)nlist * h->dim);
    h->nlist = nlist;
    h->codes.ivfpq_n2.release();             // (IVF-PQ: the norms of the ADC scan belong to the old centroids)
    if (!h->coarse) {
        h->coarse = new vdb_index_s();
        h->coarse->device = h->device;
        h->coarse->n_cus = h->n_cus;
        h->coarse->dim = h->dim;
        h->coarse->D4 = h->D4;
        h->coarse->ksteps = h->ksteps;
        h->coarse->metric = h->metric;
        h->coarse->set_only = true;      // only WHICH lists are nearest matters (assignment: k = 1; search: the probed set)
    }
    build_index(h->coarse, h->ivf_centroids.data(), false, nlist, 0, nullptr);
}

// nearest centroid of n device-resident rows (row stride = dim): int64 list ids, left on the device in dI
void ivf_assign_rows(vdb_index_s *h, const float *x_dev, int64_t n, DevBuf &dI) {
    DevBuf dD;
    dD.reserve((size_t)n * sizeof(float));
    dI.reserve((size_t)n * sizeof(int64_t));
    search_device_impl(h->coarse, x_dev, n, 1, dD.as<float>(), dI.as<int64_t>(), nullptr, nullptr, nullptr);
}

// stable counting sort of rows by list on the host (fallback for nlist > kCsrMaxLists): perm (rows grouped by list,
// ascending row inside a list), offsets
void ivf_csr(const std::vector<int64_t> &assign, int nlist, std::vector<int32_t> &perm, std::vector<int64_t> &offsets) {
    const size_t n = assign.size();
    offsets.assign((size_t)nlist + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t l = assign[i];
        if (l < 0 || l >= nlist) throw Error(VDB_ERR_INVALID, "row could not be assigned to a list");
        ++offsets[(size_t)l + 1];
    }
    for (int l = 0; l < nlist; ++l) offsets[(size_t)l + 1] += offsets[l];
    std::vector<int64_t> cursor(offsets.begin(), offsets.end() - 1);
    perm.resize(n);
    for (size_t i = 0; i < n; ++i) perm[(size_t)cursor[(size_t)assign[i]]++] = (int32_t)i;
}

// CSR of the device-resident assignment dI: dperm (int32 [n]) and doff (int64 [nlist+1]) on the device, offsets also on
// the host.  Device kernels (ivf.hpp) when the per-list counters fit in LDS, else the host loop.
void ivf_csr_build(vdb_index_s *h, const DevBuf &dI, int64_t n, int nlist, DevBuf &dperm, DevBuf &doff,
                   std::vector<int64_t> &offsets_host) {
    dperm.reserve((size_t)std::max<int64_t>(n, 1) * 4);
    doff.reserve(((size_t)nlist + 1) * 8);
    offsets_host.assign((size_t)nlist + 1, 0);
    int chunk_rows = 4096;
    while ((double)((n + chunk_rows - 1) / chunk_rows) * nlist > 1.0e8 && chunk_rows < (1 << 20)) chunk_rows *= 2;
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    if (nlist <= kCsrMaxLists && (double)nchunks * nlist <= 1.0e8 && n > 0) {
        DevBuf hist, total, bad;
        hist.reserve((size_t)nchunks * nlist * 4);
        total.reserve((size_t)nlist * 4);
        bad.reserve(4);
        VDB_HIP(hipMemsetAsync(bad.p, 0, 4, nullptr));
        const size_t lds = (size_t)nlist * 4;
        csr_hist_kernel<<<dim3((unsigned)nchunks), dim3(256), lds, nullptr>>>(dI.as<int64_t>(), n, nlist, chunk_rows,
                                                                          hist.as<int32_t>(), bad.as<int32_t>());
        csr_colscan_kernel<<<dim3((unsigned)((nlist + 255) / 256)), dim3(256), 0, nullptr>>>(hist.as<int32_t>(), (int)nchunks,
                                                                                          nlist, total.as<int32_t>());
        csr_offsets_kernel<<<dim3(1), dim3(1024), 0, nullptr>>>(total.as<int32_t>(), nlist, doff.as<int64_t>());
        csr_scatter_kernel<<<dim3((unsigned)nchunks), dim3(64), lds, nullptr>>>(dI.as<int64_t>(), n, nlist, chunk_rows,
                                                                             hist.as<int32_t>(), doff.as<int64_t>(),
                                                                             dperm.as<int32_t>());
        VDB_HIP(hipGetLastError());
        int32_t hbad = 0;
        VDB_HIP(hipMemcpy(&hbad, bad.p, 4, hipMemcpyDeviceToHost));
        if (hbad) throw Error(VDB_ERR_INVALID, "row could not be assigned to a list");
        VDB_HIP(hipMemcpy(offsets_host.data(), doff.p, ((size_t)nlist + 1) * 8, hipMemcpyDeviceToHost));
        return;
    }
    std::vector<int64_t> assign((size_t)n);
    std::vector<int32_t> perm;
    if (n > 0) VDB_HIP(hipMemcpy(assign.data(), dI.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    ivf_csr(assign, nlist, perm, offsets_host);
    if (n > 0) VDB_HIP(hipMemcpy(dperm.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(doff.p, offsets_host.data(), ((size_t)nlist + 1) * 8, hipMemcpyHostToDevice));
}

// ---- the bookkeeping of vdb_ivf_add(_assigned) that both codecs share (ivf_add_impl: float32 rows; sq8_add: codes) ----
// APPEND to a built, non-empty index (same id base), else build anew: N0 rows stay, N1 rows after the add; false = empty append
bool ivf_add_range(const vdb_index_s *h, int64_t n, int64_t id_base, int64_t &N0, int64_t &N1) {
    const bool append = h->ivf_built && h->N > 0;
    if (append) require_same_id_base(h, id_base);
    if (append && n == 0) return false;
    N0 = append ? h->N : 0;
    N1 = N0 + n;
    ivf_require(N1 <= 2147483647ll - 1024, VDB_ERR_UNSUPPORTED, "more than 2^31 rows per shard");
    return true;
}

// The lists are rebuilt from (stored rows in list order ++ new rows) with a stable sort by list, so inside a list the rows stay
// in insertion order and the index is the one a single add of the concatenated corpus builds.  dperm = source row of every
// list-order row; src_ids (N0 > 0 only) = ids of the source rows; the offsets land in h->ivf_offsets_host
void ivf_add_lists(vdb_index_s *h, const std::vector<int64_t> &assign_new, int64_t N0, DevBuf &src_ids, DevBuf &dperm, DevBuf &doff) {
    const int64_t n = (int64_t)assign_new.size(), N1 = N0 + n;
    // list of every source row: the stored rows are in list order (offsets), the new ones follow
    std::vector<int64_t> assign_all((size_t)N1);
    if (N0)
        for (int l = 0; l < h->nlist; ++l)
            std::fill(assign_all.begin() + h->ivf_offsets_host[(size_t)l], assign_all.begin() + h->ivf_offsets_host[(size_t)l + 1], (int64_t)l);
    std::copy(assign_new.begin(), assign_new.end(), assign_all.begin() + N0);
    DevBuf dassign;
    dassign.reserve((size_t)N1 * 8);
    VDB_HIP(hipMemcpy(dassign.p, assign_all.data(), (size_t)N1 * 8, hipMemcpyHostToDevice));
    if (N0) {           // ids of the source rows: the stored ones keep theirs (an append has n > 0)
        std::vector<int64_t> ids_new((size_t)n);
        for (int64_t i = 0; i < n; ++i) ids_new[(size_t)i] = h->id_base + N0 + i;
        src_ids.reserve((size_t)N1 * 8);
        VDB_HIP(hipMemcpy(src_ids.p, h->lists.ivf_ids.p, (size_t)N0 * 8, hipMemcpyDeviceToDevice));
        VDB_HIP(hipMemcpy(src_ids.as<int64_t>() + N0, ids_new.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
    ivf_csr_build(h, dassign, N1, h->nlist, dperm, doff, h->ivf_offsets_host);
}

// the list of each of n new rows on the device (`fresh`, row stride D4): the nearest centroid, read from an unpadded copy;
// left on the device in dnew and copied to assign_new
void ivf_add_assign(vdb_index_s *h, const float *fresh, int64_t n, DevBuf &dnew, std::vector<int64_t> &assign_new) {
    const int Dm = h->dim, D4 = h->D4;
    DevBuf raw;
    if (D4 != Dm) {
        raw.reserve((size_t)n * Dm * 4);
        VDB_HIP(hipMemcpy2D(raw.p, (size_t)Dm * 4, fresh, (size_t)D4 * 4, (size_t)Dm * 4, (size_t)n, hipMemcpyDeviceToDevice));
    }
    ivf_assign_rows(h, D4 != Dm ? raw.as<float>() : fresh, n, dnew);
    VDB_HIP(hipMemcpy(assign_new.data(), dnew.p, (size_t)n * 8, hipMemcpyDeviceToHost));
}

// once the rows are in list order: the counts, the offsets on the device, the list of every row in insertion order
void ivf_add_finish(vdb_index_s *h, const std::vector<int64_t> &assign_new, int64_t N0, int64_t id_base) {
    const int64_t n = (int64_t)assign_new.size();
    if (N0 + n == 0) h->ivf_offsets_host.assign((size_t)h->nlist + 1, 0);      // (no rows, no CSR build)
    h->N = N0 + n;
    h->id_base = id_base;
    h->lists.ivf_offsets.reserve((size_t)(h->nlist + 1) * 8);
    VDB_HIP(hipMemcpy(h->lists.ivf_offsets.p, h->ivf_offsets_host.data(), (size_t)(h->nlist + 1) * 8, hipMemcpyHostToDevice));
    h->ivf_list_of_row.resize((size_t)h->N);            // (the stored part stays)
    for (int64_t i = 0; i < n; ++i) h->ivf_list_of_row[(size_t)(N0 + i)] = (int32_t)assign_new[(size_t)i];
}

// vdb_ivf_add_assigned: every given list id names a list -- checked before the add touches the handle (both codecs), so a
// refused add leaves the index as it was
void ivf_check_given(const vdb_index_s *h, const int32_t *given, int64_t n) {
    if (!given) return;
    for (int64_t i = 0; i < n; ++i)
        ivf_require(given[i] >= 0 && given[i] < h->nlist, VDB_ERR_INVALID, "row could not be assigned to a list");
}

#include "ivf_sq8.inc"      // IVF<nlist>,SQ8: range training, encoding add, the codes' accessor
#include "ivf_pq.inc"       // IVF<nlist>,PQ<M>: residual product codes, encoding add, the per-batch panel pass
#include "ivf_i8.inc"       // IVF<nlist>,I8: lossless int8 rows of a byte-valued corpus, streaming add, the per-batch panel pass

// vdb_ivf_get_codes / vdb_ivfpq_get_codes: the code rows of a built coded index (`codes`: list order, `pitch` bytes apart, the
// first `width` of each are the row's code), scattered from list order to insertion order (id - id_base)
void ivf_get_codes(vdb_index_s *h, const DevBuf &codes, size_t pitch, size_t width, uint8_t *codes_host) {
    ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
    ivf_require(codes_host != nullptr || h->N == 0, VDB_ERR_INVALID, "null pointer");
    if (h->N == 0) return;
    set_device(h->device);
    std::vector<unsigned char> c((size_t)h->N * pitch);
    std::vector<int64_t> ids((size_t)h->N);
    VDB_HIP(hipDeviceSynchronize());
    VDB_HIP(hipMemcpy(c.data(), codes.p, c.size(), hipMemcpyDeviceToHost));
    VDB_HIP(hipMemcpy(ids.data(), h->lists.ivf_ids.p, ids.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < h->N; ++r) memcpy(codes_host + (size_t)(ids[(size_t)r] - h->id_base) * width, &c[(size_t)r * pitch], width);
}

// the panel space of the filed rows: every list padded to whole spans of `span_rows` rows.  Fills the span tables (list_pspan0,
// span_row0, span_valid; host counts ivf_pspans, ivf_max_pspans, ivf_span_rows) and returns the number of spans
int64_t ivf_build_spans(vdb_index_s *h, int span_rows) {
    const int nlist = h->nlist;
    h->ivf_span_rows = span_rows;
    std::vector<int32_t> pspan0((size_t)nlist + 1, 0), row0, valid;
    int maxp = 0;
    for (int l = 0; l < nlist; ++l) {
        const int64_t lo = h->ivf_offsets_host[(size_t)l], hi = h->ivf_offsets_host[(size_t)l + 1];
        const int spans = (int)((hi - lo + span_rows - 1) / span_rows);
        pspan0[(size_t)l + 1] = pspan0[(size_t)l] + spans;
        maxp = std::max(maxp, spans);
        for (int j = 0; j < spans; ++j) {
            row0.push_back((int32_t)(lo + (int64_t)j * span_rows));
            valid.push_back((int32_t)std::min<int64_t>(span_rows, hi - lo - (int64_t)j * span_rows));
        }
    }
    const int64_t P = pspan0[(size_t)nlist];
    h->ivf_pspans = P;
    h->ivf_max_pspans = maxp;
    if (P == 0) return 0;
    h->lists.ivf_list_pspan0.reserve(((size_t)nlist + 1) * 4);
    h->lists.ivf_span_row0.reserve((size_t)P * 4);
    h->lists.ivf_span_valid.reserve((size_t)P * 4);
    VDB_HIP(hipMemcpy(h->lists.ivf_list_pspan0.p, pspan0.data(), ((size_t)nlist + 1) * 4, hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(h->lists.ivf_span_row0.p, row0.data(), (size_t)P * 4, hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(h->lists.ivf_span_valid.p, valid.data(), (size_t)P * 4, hipMemcpyHostToDevice));
    return P;
}

// fp16 panels of the permuted rows, every list padded to whole spans (list-major MFMA scan).  D <= 128: 32-row tiles,
// 256-row spans (kIvfSpanRows; scan_kernel / scan_i8_kernel in ITEMS mode).  D > 128: p16 tiles (ivf_kloop.hpp), spans of 256 rows
// (four 64-row bins) or, for lists of thousands of rows, 1024 rows (four 256-row bins).
void ivf_build_panel_space(vdb_index_s *h) {
    h->ivf_mfma_ok = false;
    h->scan_ok = false;
    h->tile16 = h->ksteps > kMaxKSteps;
    if (h->N == 0 || h->dim > 4096) return;
    hipStream_t st = nullptr;
    index_stats(h, st);
    if (h->nonfinite) return;
    h->ivf_tps = h->tile16 ? ivf_tps_of(h->opt, h->N, h->nlist) : 0;
    const int span_rows = h->tile16 ? h->ivf_tps * 16 : kIvfSpanRows;
    const int64_t P = ivf_build_spans(h, span_rows);
    if (P == 0) return;
    const int64_t ntiles = h->tile16 ? P * h->ivf_tps : P * kIvfTilesPerSpan;
    const int ksl = h->tile16 ? h->ksteps / 2 : h->ksteps;           // k-steps of the layout (32 or 16 dims)
    h->scan.panels.reserve((size_t)ntiles * ksl * 64 * sizeof(half8));
    const int64_t threads = ntiles * ksl * 64;
    if (h->tile16)
        ivf_build_panels16_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(
            h->rows.x32.as<float>(), h->dim, h->D4, ksl, h->ivf_tps, ntiles, h->sx, h->lists.ivf_span_row0.as<int32_t>(),
            h->lists.ivf_span_valid.as<int32_t>(), h->scan.panels.as<half8>(), h->kept.stats.as<IndexStats>());
    else
        ivf_build_panels_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(
            h->rows.x32.as<float>(), h->dim, h->D4, h->ksteps, ntiles, h->sx, h->lists.ivf_span_row0.as<int32_t>(),
            h->lists.ivf_span_valid.as<int32_t>(), h->scan.panels.as<half8>(), h->kept.stats.as<IndexStats>());
    VDB_HIP(hipGetLastError());
    h->scan.bias.reserve((size_t)P * span_rows * sizeof(float));
    ivf_build_bias_kernel<<<dim3((unsigned)((P * span_rows + 255) / 256)), dim3(256), 0, st>>>(
        h->rows.xnorm2.as<float>(), P, span_rows, h->metric, h->lists.ivf_span_row0.as<int32_t>(), h->lists.ivf_span_valid.as<int32_t>(),
        h->scan.bias.as<float>());
    VDB_HIP(hipGetLastError());
    IndexStats hs;
    VDB_HIP(hipMemcpy(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost));
    h->corpus_fp16_exact = hs.not_fp16_exact == 0;
    h->i8_ok = h->i8_ok && !h->tile16 && h->ivf_codec == 0;   // (an SQ8 / IVF-PQ index keeps no int8 copies)
    if (h->i8_ok) {      // byte-valued rows: int8 copy of the same panel space (scan_i8.hpp)
        h->i8_ks = h->dim <= 64 ? 2 : 4;
        h->scan.panels8.reserve((size_t)ntiles * h->i8_ks * 64 * sizeof(int4v));
        const int64_t t8 = ntiles * h->i8_ks * 64;
        ivf_build_panels_i8_kernel<<<dim3((unsigned)((t8 + 255) / 256)), dim3(256), 0, st>>>(
            h->rows.x32.as<float>(), h->dim, h->D4, h->i8_ks, ntiles, h->i8_cx, h->lists.ivf_span_row0.as<int32_t>(),
            h->lists.ivf_span_valid.as<int32_t>(), h->scan.panels8.as<int4v>());
        h->scan.bias8.reserve((size_t)2 * P * kIvfSpanRows * sizeof(int32_t));
        h->scan.rowstat8.reserve((size_t)h->N * 2 * sizeof(int));
        ivf_build_bias_i8_kernel<<<dim3((unsigned)((P * kIvfSpanRows + 255) / 256)), dim3(256), 0, st>>>(
            h->rows.x32.as<float>(), P, h->dim, h->D4, h->metric, h->lists.ivf_span_row0.as<int32_t>(),
            h->lists.ivf_span_valid.as<int32_t>(), h->scan.bias8.as<int32_t>(), h->scan.rowstat8.as<int>());
        build_rows_i8(h, st);
        VDB_HIP(hipGetLastError());
        VDB_HIP(hipStreamSynchronize(st));
    }
    h->ivf_mfma_ok = true;
}

constexpr size_t kZeroSmall = (kSmallBytes + 127) / 128 * 128;     // stride of the two ws.small views inside ivf_zero

// ---- path, geometry, capacities and launch shapes of a batch: ivf_plan.hpp decides, this file reserves, fills arguments and launches ----
// what the rules of ivf_plan.hpp read of a handle
IvfIndexShape ivf_shape_of(const vdb_index_s *h) {
    IvfIndexShape s;
    s.mfma_ok = h->ivf_mfma_ok; s.tile16 = h->tile16; s.nlist = h->nlist; s.N = h->N;
    s.pspans = h->ivf_pspans; s.max_pspans = h->ivf_max_pspans; s.span_rows = h->ivf_span_rows; s.tps = h->ivf_tps;
    s.ksteps = h->ksteps; s.i8_ks = h->i8_ks;
    s.has_i8 = h->i8_ok && h->scan.panels8.p != nullptr;
    return s;
}

// one row per instantiation of a family (the lists of ivf_plan.hpp): its key and its kernel
#define VDB_ROW_IVF_SCAN(...) {ScanKey{{__VA_ARGS__}}, &scan_kernel<__VA_ARGS__>},
#define VDB_ROW_IVF_SCAN_I8(...) {ScanKey{{__VA_ARGS__}}, &scan_i8_kernel<__VA_ARGS__>},
#define VDB_ROW_IVF_KLOOP(...) {ScanKey{{__VA_ARGS__}}, &ivf_kloop_scan_kernel<__VA_ARGS__>},
constexpr ScanRow<ScanArgs> kRowsIvfScan[] = {VDB_KERNELS_IVF_SCAN(VDB_ROW_IVF_SCAN)};
constexpr ScanRow<ScanI8Args> kRowsIvfScanI8[] = {VDB_KERNELS_IVF_SCAN_I8(VDB_ROW_IVF_SCAN_I8)};
constexpr ScanRow<IvfKloopArgs> kRowsIvfKloop[] = {VDB_KERNELS_IVF_KLOOP(VDB_ROW_IVF_KLOOP)};
#undef VDB_ROW_IVF_SCAN
#undef VDB_ROW_IVF_SCAN_I8
#undef VDB_ROW_IVF_KLOOP

// the one <<<>>> of the plan's family, with the arguments of that family
void ivf_launch(const IvfLaunch &p, const ScanArgs *sa, const ScanI8Args *s8, const IvfKloopArgs *ka, hipStream_t st) {
    const dim3 grid(p.grid_x, p.grid_y), block(p.block);
    switch (p.family) {
        case ScanFamily::scan: scan_kernel_of(kRowsIvfScan, p)<<<grid, block, 0, st>>>(*sa); break;
        case ScanFamily::scan_i8: scan_kernel_of(kRowsIvfScanI8, p)<<<grid, block, 0, st>>>(*s8); break;
        case ScanFamily::ivf_kloop: scan_kernel_of(kRowsIvfKloop, p)<<<grid, block, 0, st>>>(*ka); break;
        default: throw Error(VDB_ERR_INVALID, "internal: no list scan kernel for an empty plan");
    }
    VDB_HIP(hipGetLastError());
}

// one batch of an IVF search, as ivf_search_device_impl hands it to its path.  The coarse result (nb x nprobe list ids) is
// already on the device (plan.ivf_probe_i).  (D, I) = final rows, or D == nullptr and (pk, pi) = per-shard partial rows
// (float64 order keys + ids): all four at this batch's offset
struct IvfBatch {
    vdb_index_s *h;
    const float *q, *qpad;
    int64_t nb;
    int k, nprobe;
    float *D; int64_t *I; double *pk; int64_t *pi;
    long tslot;
    hipStream_t st;
    IvfIndexShape shape;    // ivf_shape_of(h)
    IvfGeom g;              // list-major path only: the geometry, and the zeroed counter block of this batch (ivf_zero)
    int32_t *d_cnt;
    bool filtered;          // a vdb_ivf_search_filtered call (ivf_filter.inc): the scans read the masked copies of the handle's filter,
                            // the exact stages test its list-order allow words
};

// what the steps of ivf_search_lists share: capacities, the plan's launch shape, views into the counter block and the plan
struct IvfLists {
    IvfCaps c;
    int32_t *d_cursor, *d_slot_query, *d_fb_done;
    const int64_t *probes;
    IvfPlan *plan;
    QueryBatchInfo *info;
};

IvfLists ivf_lists_reserve(const IvfBatch &b) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    const int nlist = h->nlist;
    const int64_t nb = b.nb;
    IvfLists L{};
    L.c = ivf_caps(b.shape, h->opt, b.g, b.k);
    ws.eps.reserve((size_t)nb * sizeof(float));
    ws.qpanels.reserve((size_t)nb * h->ksteps * 16 * sizeof(_Float16));   // scaled fp16 query rows
    if (L.c.use_i8) ws.qpanels8.reserve((size_t)nb * h->i8_ks * 32);      // int8 query rows
    ws.bin_m1.reserve(b.g.bin_bytes);
    ws.bin_m2.reserve(b.g.bin_bytes);
    ws.bin_m3.reserve(b.g.bin_bytes);
    if (b.g.kloop) {
        ws.bin_m4.reserve(b.g.bin_bytes);
        ws.bin_m5.reserve(b.g.bin_bytes);
    }
    ws.cand.reserve((size_t)nb * L.c.cand_cap * sizeof(int32_t));
    ws.rescan.reserve((size_t)nb * L.c.rescan_cap * 2 * sizeof(int32_t));
    ws.counts.reserve((size_t)nb * 2 * sizeof(int32_t));
    ws.fallback.reserve((size_t)nb * sizeof(int32_t));
    L.d_cursor = b.d_cnt + nlist;
    L.d_slot_query = L.d_cursor + nlist;
    L.d_fb_done = L.d_slot_query + b.g.max_slots;
    ws.fb_list.reserve((size_t)nb * sizeof(int32_t));
    h->plan.ivf_slot_off.reserve(((size_t)nlist + 1) * 4);
    h->plan.ivf_list_item0.reserve(((size_t)nlist + 1) * 4);
    h->plan.ivf_item_list.reserve((size_t)b.g.max_items * 4);
    h->plan.ivf_item_slot0.reserve((size_t)b.g.max_items * 4);
    h->plan.ivf_item_bin0.reserve((size_t)b.g.max_items * 4);
    h->plan.ivf_plan.reserve(sizeof(IvfPlan));
    h->plan.ivf_slot_of.reserve((size_t)b.g.pairs * 4);
    L.probes = h->plan.ivf_probe_i.as<int64_t>();
    L.plan = h->plan.ivf_plan.as<IvfPlan>();
    L.info = batch_info(ws);      // (cleared by the dispatcher with the rest of ivf_zero)
    return L;
}

// query statistics (unless the coarse search of this batch took them), then scales + error bounds + query rows of either
// form + the per-list pair counts: one dispatch
void ivf_lists_prep(const IvfBatch &b, const IvfLists &L) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    const int Dm = h->dim;
    const int64_t nb = b.nb, total = nb * Dm;
    const FinalizeArgs fin{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2,
                           L.c.use_i8 ? (1 | (h->opt.ivf_i8_group == 8 ? 4 : 0)) : 0};   // (quads or octs, see plan_ivf_i8)
    const bool from_coarse = h->coarse->info_valid_nq == nb;   // the coarse search of this batch already took the statistics of these queries
    if (!from_coarse) query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, b.st>>>(b.q, total, L.info, fin);
    IvfPrepArgs pa{};
    pa.eps = EpsArgs{b.q, nb, Dm, h->ksteps * 16, h->metric, sqrtf(h->maxnorm2) * 1.0000002f,
                     h->corpus_fp16_exact ? 1 : 0, h->corpus_int_unscaled ? 1 : 0, h->sx, L.info, ws.eps.as<float>()};
    pa.Q = b.q; pa.nq = nb; pa.D = Dm; pa.Dpad = h->ksteps * 16;      // (= i8_ks * 32: both query-row forms have the same pitch)
    pa.qrows = reinterpret_cast<_Float16 *>(ws.qpanels.p);
    pa.q8 = L.c.use_i8 ? reinterpret_cast<signed char *>(ws.qpanels8.p) : nullptr;
    pa.info = L.info; pa.src = from_coarse ? batch_info(h->coarse->ws) : nullptr; pa.fin = fin;
    pa.n_eps_blocks = (unsigned)((nb * 16 + 255) / 256);
    pa.n_row_blocks = (unsigned)((nb * pa.Dpad / 8 + 255) / 256);     // (8 dims per thread)
    pa.probes = L.probes; pa.npairs = b.g.pairs; pa.nlist = h->nlist; pa.ppb = L.c.ppb; pa.cnt = b.d_cnt;
    ivf_prep_kernel<<<dim3(pa.n_eps_blocks + pa.n_row_blocks + L.c.pblocks), dim3(256), L.c.hist_bytes, b.st>>>(pa);
}

// work items of every probed list and the slot of every (query, probe) pair.  nlist <= kIvfLdsLists: plan + scatter in one
// dispatch (every workgroup recomputes the slot prefix in LDS), else a kernel each
void ivf_lists_plan(const IvfBatch &b, const IvfLists &L) {
    vdb_index_s *h = b.h;
    const int nlist = h->nlist;
    const auto plan_scatter = L.c.small_ppb ? ivf_plan_scatter_kernel<kIvfPairsPerBlock / 4> : ivf_plan_scatter_kernel<kIvfPairsPerBlock>;
    const auto scatter = L.c.small_ppb ? ivf_scatter_kernel<kIvfPairsPerBlock / 4> : ivf_scatter_kernel<kIvfPairsPerBlock>;
    if (L.c.hist_bytes) {
        plan_scatter<<<dim3(L.c.pblocks), dim3(256), 2 * L.c.hist_bytes, b.st>>>(
            L.probes, b.nb, b.nprobe, nlist, b.d_cnt, h->lists.ivf_list_pspan0.as<int32_t>(), b.g.group, b.g.bins_per_span, b.g.run_groups,
            (int)b.g.max_items, (int)b.g.max_slots, (int)b.g.max_bins, h->lists.ivf_offsets.as<int64_t>(), h->plan.ivf_slot_off.as<int32_t>(),
            h->plan.ivf_list_item0.as<int32_t>(), h->plan.ivf_item_list.as<int32_t>(), h->plan.ivf_item_slot0.as<int32_t>(),
            h->plan.ivf_item_bin0.as<int32_t>(), L.plan, L.d_cursor, L.d_slot_query, h->plan.ivf_slot_of.as<int32_t>());
    } else {
        ivf_plan_kernel<<<dim3(1), dim3(1024), 0, b.st>>>(
            b.d_cnt, h->lists.ivf_list_pspan0.as<int32_t>(), nlist, b.g.group, b.g.bins_per_span, b.g.run_groups, (int)b.g.max_items,
            (int)b.g.max_slots, (int)b.g.max_bins, h->plan.ivf_slot_off.as<int32_t>(), h->plan.ivf_list_item0.as<int32_t>(),
            h->plan.ivf_item_list.as<int32_t>(), h->plan.ivf_item_slot0.as<int32_t>(), h->plan.ivf_item_bin0.as<int32_t>(), L.plan,
            h->lists.ivf_offsets.as<int64_t>());
        scatter<<<dim3(L.c.pblocks), dim3(256), L.c.hist_bytes, b.st>>>(
            L.probes, b.nb, b.nprobe, nlist, h->plan.ivf_slot_off.as<int32_t>(), h->lists.ivf_list_pspan0.as<int32_t>(), L.d_cursor, L.plan,
            L.d_slot_query, h->plan.ivf_slot_of.as<int32_t>());
    }
    VDB_HIP(hipGetLastError());
}

// SQ8: the fp16 panels of the whole panel space, converted from the codes for this batch (workspace)
const half8 *ivf_sq8_panels(const IvfBatch &b) {
    vdb_index_s *h = b.h;
    const int64_t ntiles = h->ivf_pspans * kIvfTilesPerSpan;
    h->ws.sq8_panels.reserve((size_t)ntiles * h->ksteps * 64 * sizeof(half8));
    const int64_t threads = ntiles * h->ksteps * 64;
    ivf_sq8_panels_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, b.st>>>(
        sq8_rows(h), h->dim, h->D4, h->ksteps, ntiles, h->sx, h->lists.ivf_span_row0.as<int32_t>(), h->lists.ivf_span_valid.as<int32_t>(),
        h->ws.sq8_panels.as<half8>());
    VDB_HIP(hipGetLastError());
    return h->ws.sq8_panels.as<half8>();
}

// D > 128: the K-loop scan on p16 panels (ivf_kloop.hpp)
void ivf_scan_kloop(const IvfBatch &b, int kgroup, const ScanArgs &sa) {
    vdb_index_s *h = b.h;
    const IvfLaunch p = plan_ivf_kloop(b.shape, h->opt, b.g, kgroup);
    IvfKloopArgs ka{};
    ka.panels = sa.panels; ka.bias = sa.bias; ka.qrows = sa.qrows; ka.info = sa.info;
    ka.bin_m[0] = sa.bin_m1; ka.bin_m[1] = sa.bin_m2; ka.bin_m[2] = sa.bin_m3;
    ka.bin_m[3] = h->ws.bin_m4.as<float>(); ka.bin_m[4] = h->ws.bin_m5.as<float>();
    ka.item_list = sa.item_list; ka.item_slot0 = sa.item_slot0; ka.item_bin0 = sa.item_bin0;
    ka.n_items = sa.n_items; ka.list_pspan0 = sa.list_pspan0; ka.slot_query = sa.slot_query;
    ka.ksteps = h->ksteps;
    ka.part_spans = p.part_spans;
    ivf_launch(p, nullptr, nullptr, &ka, b.st);
}

// D <= 128: scan_kernel in ITEMS mode on 32-row tiles.  Sets sa.part_spans (the int8 scan takes the same, and the same grid)
void ivf_scan_fp16(const IvfBatch &b, ScanArgs &sa) {
    const IvfLaunch p = plan_ivf_f16(b.shape, b.h->opt, b.g);
    sa.part_spans = p.part_spans;
    ivf_launch(p, &sa, nullptr, nullptr, b.st);
}

// the int8 form of the same scan; whichever the finalize kernel did not choose returns at once
void ivf_scan_i8(const IvfBatch &b, const ScanArgs &sa) {
    vdb_index_s *h = b.h;
    ScanI8Args s8{};
    s8.panels = h->scan.panels8.as<int4v>();
    s8.bias8 = b.filtered ? h->ivf_filter.bias8_f.as<int32_t>() : h->scan.bias8.as<int32_t>();
    s8.info = sa.info;
    s8.bin_m1 = sa.bin_m1; s8.bin_m2 = sa.bin_m2; s8.bin_m3 = sa.bin_m3;
    s8.Npad = h->ivf_pspans * kIvfSpanRows;
    s8.item_list = sa.item_list; s8.item_slot0 = sa.item_slot0; s8.item_bin0 = sa.item_bin0;
    s8.n_items = sa.n_items; s8.list_pspan0 = sa.list_pspan0; s8.slot_query = sa.slot_query;
    s8.qrows = reinterpret_cast<const signed char *>(h->ws.qpanels8.p);
    s8.part_spans = sa.part_spans;
    ivf_launch(plan_ivf_i8(b.shape, h->opt, b.g), nullptr, &s8, nullptr, b.st);
}

IvfSelectArgs ivf_lists_select(const IvfBatch &b, const IvfLists &L, const ScanArgs &sa) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    const int k = b.k, nprobe = b.nprobe;
    const IvfSelectCaps sc = ivf_select_caps(b.shape, b.g, L.c, k, nprobe);
    IvfSelectArgs se{};
    se.bin_m[0] = sa.bin_m1; se.bin_m[1] = sa.bin_m2; se.bin_m[2] = sa.bin_m3;
    se.bin_m[3] = b.g.kloop ? ws.bin_m4.as<float>() : nullptr;
    se.bin_m[4] = b.g.kloop ? ws.bin_m5.as<float>() : nullptr;
    se.nm = sc.nm;
    se.eps = ws.eps.as<float>();
    se.info = L.info; se.plan = L.plan; se.probes = L.probes;
    se.slot_of = h->plan.ivf_slot_of.as<int32_t>(); se.slot_off = h->plan.ivf_slot_off.as<int32_t>();
    se.list_item0 = h->plan.ivf_list_item0.as<int32_t>(); se.item_bin0 = h->plan.ivf_item_bin0.as<int32_t>();
    se.list_pspan0 = h->lists.ivf_list_pspan0.as<int32_t>();
    se.span_row0 = h->lists.ivf_span_row0.as<int32_t>(); se.span_valid = h->lists.ivf_span_valid.as<int32_t>();
    se.nq = b.nb; se.nprobe = nprobe; se.group = b.g.group; se.k = k;
    se.cand_cap = L.c.cand_cap; se.rescan_cap = L.c.rescan_cap;
    se.max_entries = sc.max_entries; se.probe_cap = sc.probe_cap; se.vals_entries = sc.vals_entries; se.act_cap = sc.act_cap;
    se.group_rows = b.g.kloop ? L.c.kgroup : 0;
    se.bins_per_span = b.g.bins_per_span; se.bin_rows = b.g.bin_rows; se.run_groups = b.g.run_groups;
    se.cand_rows = ws.cand.as<int32_t>(); se.rescan_rows = ws.rescan.as<int32_t>();
    se.counts = ws.counts.as<int32_t>(); se.fallback = ws.fallback.as<int32_t>(); se.fb_list = ws.fb_list.as<int32_t>();
    se.fb_count = ws.small.as<int32_t>();            // (zeroed with the batch info: the first 64 bytes of ws.small)
    se.stat_counters = reinterpret_cast<unsigned long long *>(ws.small.as<char>() + 64);
    ivf_select_kernel<<<dim3((unsigned)((b.nb + 1) / 2)), dim3(128),
                        (size_t)2 * ivf_select_lds_words(se.vals_entries, se.probe_cap, se.act_cap, se.nm) * 4, b.st>>>(se);
    VDB_HIP(hipGetLastError());
    return se;
}

// the refine of the selected candidates and, in the same launch, the flagged queries (work list overflow, unusable scales,
// plan overflow): exact list scan, split on the device
void ivf_lists_tail(const IvfBatch &b, const IvfLists &L, const IvfSelectArgs &se) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    const int k = b.k;
    const int64_t nb = b.nb;
    RefineCommon rc{h->rows.x32.as<float>(), b.qpad, h->N, h->id_base, h->D4, h->metric, k, h->lists.ivf_ids.as<int64_t>()};
    rc.info = L.info;
    if (b.filtered) rc.allow = h->ivf_filter.words.as<uint32_t>();
    if (sq8(h)) rc.sq8 = sq8_rows(h);      // (the refine and the flagged-query pass decode the candidates' codes)
    if (ivfpq(h)) rc.ivfpq = ivfpq_rows(h);
    if (ivf_i8(h)) i8_refine_rows(h, rc);  // (IVF-I8: rc.X is nullptr, every exact stage scores the int8 rows)
    if (L.c.use_i8 && h->scan.rows8.p) {
        rc.X8 = h->scan.rows8.as<signed char>(); rc.rowstat = h->scan.rowstat8.as<int>();
        rc.Q8 = reinterpret_cast<const signed char *>(ws.qpanels8.p);      // the int8 query rows the scan gathers from
        rc.x8_pitch = h->rows8_pitch; rc.cx = h->i8_cx; rc.D = h->dim;
    }
    RefineListArgs la{};
    la.c = rc;
    la.nq = nb;
    la.cand_rows = se.cand_rows; la.rescan_rows = se.rescan_rows; la.counts = se.counts; la.fallback = se.fallback;
    la.cand_cap = L.c.cand_cap; la.rescan_cap = L.c.rescan_cap;
    la.D = b.D; la.I = b.I; la.pkeys = b.pk; la.pids = b.pi;
    if (b.g.kloop) la.group_shift = L.c.kgroup == 1 ? 0 : L.c.kgroup == 2 ? 1 : 2;
    IvfFallbackArgs a{};
    a.c = rc;
    a.offsets = h->lists.ivf_offsets.as<int64_t>();
    a.probes = L.probes; a.nprobe = b.nprobe;
    a.fb_list = se.fb_list; a.fb_count = se.fb_count;
    a.max_split = std::min(b.nprobe, 64);
    a.cap_units = std::max<int64_t>(nb, 4096);
    ws.pkeys.reserve((size_t)a.cap_units * k * sizeof(double));
    ws.pids.reserve((size_t)a.cap_units * k * sizeof(int64_t));
    a.pkeys = ws.pkeys.as<double>(); a.pids = ws.pids.as<int64_t>();
    a.done = L.d_fb_done;
    a.D = b.D; a.I = b.I; a.okeys = b.pk; a.oids = b.pi;
    const int kpl = kpl_for(k);
    const dim3 grid(512 + (unsigned)((nb + 3) / 4));
    if (b.filtered) {
        DISPATCH_KPL(kpl, (ivf_tail_kernel<KPL, true><<<grid, dim3(256), 0, b.st>>>(la, a, 512u)));
    } else {
        DISPATCH_KPL(kpl, (ivf_tail_kernel<KPL><<<grid, dim3(256), 0, b.st>>>(la, a, 512u)));
    }
    VDB_HIP(hipGetLastError());
}

// the list-major MFMA path: the steps in the order they are enqueued
void ivf_search_lists(const IvfBatch &b) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    const IvfLists L = ivf_lists_reserve(b);
    ivf_lists_prep(b, L);
    ivf_lists_plan(b, L);
    ScanArgs sa{};
    // IVF-I8 under "ivf_i8_scratch" = 0 holds no fp16 panels at all: the fp16 scan is not launched, and a batch the int8 scan
    // does not serve is flagged as a whole for the tail's exact list scan (ivf_i8_flag_kernel)
    const bool i8_no_slab = ivf_i8(h) && !h->opt.ivf_i8_scratch;
    sa.panels = i8_no_slab ? nullptr : ivf_i8(h) ? ivf_i8_panels(h, L.info, b.st) : sq8(h) ? ivf_sq8_panels(b) : ivfpq(h) ? ivf_pq_panels(h, b.st) : h->scan.panels.as<half8>();
    sa.bias = b.filtered ? h->ivf_filter.bias_f.as<float>() : h->scan.bias.as<float>();
    sa.qpanels = nullptr;
    sa.qrows = reinterpret_cast<const _Float16 *>(ws.qpanels.p);
    sa.slot_query = L.d_slot_query;
    sa.info = L.info;
    sa.bin_m1 = ws.bin_m1.as<float>(); sa.bin_m2 = ws.bin_m2.as<float>(); sa.bin_m3 = ws.bin_m3.as<float>();
    sa.item_list = h->plan.ivf_item_list.as<int32_t>(); sa.item_slot0 = h->plan.ivf_item_slot0.as<int32_t>();
    sa.item_bin0 = h->plan.ivf_item_bin0.as<int32_t>();
    sa.n_items = &L.plan->n_items;
    sa.list_pspan0 = h->lists.ivf_list_pspan0.as<int32_t>();
    timing_mark(h, b.tslot, 0, b.st);
    if (b.g.kloop) {
        ivf_scan_kloop(b, L.c.kgroup, sa);
    } else {
        if (i8_no_slab) {
            ivf_i8_flag_kernel<<<dim3(1), dim3(64), 0, b.st>>>(L.info);
            sa.part_spans = plan_ivf_f16(b.shape, h->opt, b.g).part_spans;      // (the int8 scan takes the fp16 plan's parts)
        } else {
            ivf_scan_fp16(b, sa);
        }
        if (L.c.use_i8) ivf_scan_i8(b, sa);
    }
    timing_mark(h, b.tslot, 1, b.st);
    const IvfSelectArgs se = ivf_lists_select(b, L, sa);
    ivf_lists_tail(b, L, se);
}

// (re)size ivf_zero and point both ws.small at it: [coarse small | own small | counter block of `cnt_words` ints]
int32_t *ivf_bind_zero(vdb_index_s *h, size_t cnt_words) {
    const size_t need = 2 * kZeroSmall + cnt_words * 4;
    if (need > h->plan.ivf_zero.cap || h->ws.small.p != (char *)h->plan.ivf_zero.p + kZeroSmall) {
        // (dropping the views first: reserve() may free the memory they point into)
        h->ws.small.release();
        if (h->coarse) h->coarse->ws.small.release();
        h->plan.ivf_zero.reserve(need);
        h->ws.small.borrow((char *)h->plan.ivf_zero.p + kZeroSmall, kSmallBytes);
    }
    if (h->coarse && h->coarse->ws.small.p != h->plan.ivf_zero.p) h->coarse->ws.small.borrow(h->plan.ivf_zero.p, kSmallBytes);
    return reinterpret_cast<int32_t *>((char *)h->plan.ivf_zero.p + 2 * kZeroSmall);
}

// the exact list scan: every query's probed lists in S splits (one wave each), merged when S > 1
void ivf_search_exact(const IvfBatch &b) {
    vdb_index_s *h = b.h;
    Workspace &ws = h->ws;
    const int64_t nb = b.nb;
    const int k = b.k, nprobe = b.nprobe;
    hipStream_t st = b.st;
    const int64_t S = ivf_exact_splits(h->N, h->nlist, nprobe, nb, k);
    IvfScanArgs a{};
    a.c = RefineCommon{h->rows.x32.as<float>(), b.qpad, h->N, h->id_base, h->D4, h->metric, k, h->lists.ivf_ids.as<int64_t>()};
    if (sq8(h)) a.c.sq8 = sq8_rows(h);      // (SQ8: no float32 rows -- the rows are decoded from their codes)
    if (ivfpq(h)) a.c.ivfpq = ivfpq_rows(h);  // (IVF-PQ: likewise, centroid + codebook entry)
    if (ivf_i8(h)) i8_refine_rows(h, a.c);    // (IVF-I8: the int8 rows, x = byte + cx)
    if (b.filtered) a.c.allow = h->ivf_filter.words.as<uint32_t>();
    a.offsets = h->lists.ivf_offsets.as<int64_t>();
    a.probes = h->plan.ivf_probe_i.as<int64_t>();
    a.nq = nb; a.nprobe = nprobe; a.S = (int)S;
    if (S == 1) {
        a.D = b.D; a.I = b.I; a.pkeys = b.pk; a.pids = b.pi;
    } else {
        ws.pkeys.reserve((size_t)nb * S * k * sizeof(double));
        ws.pids.reserve((size_t)nb * S * k * sizeof(int64_t));
        a.pkeys = ws.pkeys.as<double>(); a.pids = ws.pids.as<int64_t>();
    }
    timing_mark(h, b.tslot, 0, st);
    const int kpl = kpl_for(k);
    const unsigned grid = (unsigned)((nb * S + 3) / 4);
    if (b.filtered) {
        DISPATCH_KPL(kpl, (ivf_scan_kernel<KPL, true><<<dim3(grid), dim3(256), 0, st>>>(a)));
    } else {
        DISPATCH_KPL(kpl, (ivf_scan_kernel<KPL><<<dim3(grid), dim3(256), 0, st>>>(a)));
    }
    VDB_HIP(hipGetLastError());
    timing_mark(h, b.tslot, 1, st);
    if (S > 1) {
        MergeArgs ma{};
        ma.pkeys = a.pkeys; ma.pids = a.pids;
        ma.part_stride = k; ma.slot_stride = S * k; ma.nparts = (int)S;
        ma.k = k; ma.metric = h->metric; ma.count = nb;
        ma.D = b.D; ma.I = b.I; ma.okeys = b.pk; ma.oids = b.pi;
        launch_merge(ma, nb, st);
    }
}

// what both paths share -- the clearing of ivf_zero, timing_begin, the coarse search, padded queries -- then the path, per batch
// (filtered: a vdb_ivf_search_filtered call, ivf_filter.inc -- the same batches with IvfBatch::filtered set; the coarse search never
//  looks at the filter, the routing rule reads the admitted count)
void ivf_search_device_impl(vdb_index_s *h, const float *dq, int64_t nq, int k, float *D, int64_t *I, double *PK,
                            int64_t *PI, hipStream_t st, bool filtered = false) {
    ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
    const bool partial = D == nullptr;
    ivf_require(k >= 1 && k <= 2048, VDB_ERR_INVALID, "k must be in [1, 2048]");
    ivf_require(nq >= 0, VDB_ERR_INVALID, "negative query count");
    h->last.last_nq = nq;
    h->last.last_path = VDB_PATH_IVF;
    if (nq == 0) return;
    ivf_require(dq && (partial ? (PK && PI) : (D && I)), VDB_ERR_INVALID, "null pointer");
    const int nprobe = std::max(1, std::min(h->nprobe, h->nlist));
    const int Dm = h->dim, D4 = h->D4;
    const int64_t kBatch = 16384;
    Workspace &ws = h->ws;
    bool any_mfma = false, any_adc = false;
    const IvfIndexShape shape = ivf_shape_of(h);
    // IVF-PQ, option "ivfpq_adc_max_batch": batches ivf_adc_plan admits take the lookup-table scan of the probed lists (ivf_pq.inc).
    // The first call that may admit one makes the handle's norms (one pass over the codes, one stream synchronisation)
    const bool adc_on = ivfpq(h) && h->opt.ivfpq_adc_max_batch > 0 && h->opt.force_path == 0 && k <= kIvfAdcMaxK &&
                        std::min<int64_t>(kBatch, nq) <= h->opt.ivfpq_adc_max_batch && h->N > 0;
    const bool adc_ranges = adc_on && ivfpq_adc_prepare(h, st);
    const int64_t adc_longest = adc_ranges ? ivfpq_longest_list(h) : 0;
    const size_t ev_mark = h->ev_used;
    try {
    for (int64_t b0 = 0; b0 < nq; b0 += kBatch) {
        IvfBatch b{};
        b.h = h; b.k = k; b.nprobe = nprobe; b.st = st;
        b.nb = std::min<int64_t>(kBatch, nq - b0);
        b.q = dq + (size_t)b0 * Dm;
        // everything this batch needs zeroed sits in ivf_zero: ONE memset (first batch of a call: both ws.small whole and
        // the counter block; later batches keep this handle's statistics counters, which accumulate over the call)
        b.shape = shape;
        b.filtered = filtered;
        const IvfAdcPlan adc = ivf_adc_plan(h->opt, h->ivf_codec, h->ivfpq.M, adc_ranges, h->N, adc_longest, b.nb, k, b.nprobe);
        if (!adc.ok) b.g = filtered ? ivf_filter_geometry(shape, h->opt, b.nb, k, b.nprobe, h->ivf_filter_count) : ivf_geometry(shape, h->opt, b.nb, k, b.nprobe);
        b.d_cnt = ivf_bind_zero(h, b.g.ok ? b.g.cnt_words : 0);
        if (b0 == 0) {
            VDB_HIP(hipMemsetAsync(h->plan.ivf_zero.p, 0, 2 * kZeroSmall + (b.g.ok ? b.g.cnt_words * 4 : 0), st));
        } else {
            VDB_HIP(hipMemsetAsync(h->plan.ivf_zero.p, 0, kZeroSmall + 64, st));
            if (b.g.ok) VDB_HIP(hipMemsetAsync(b.d_cnt, 0, b.g.cnt_words * 4, st));
        }
        h->coarse->small_preset = true;
        b.tslot = timing_begin(h, st);
        h->plan.ivf_probe_d.reserve((size_t)b.nb * b.nprobe * sizeof(float));
        h->plan.ivf_probe_i.reserve((size_t)b.nb * b.nprobe * sizeof(int64_t));
        search_device_impl(h->coarse, b.q, b.nb, b.nprobe, h->plan.ivf_probe_d.as<float>(), h->plan.ivf_probe_i.as<int64_t>(), nullptr,
                           nullptr, st);
        b.qpad = b.q;
        if (D4 != Dm) {
            ws.qpad.reserve((size_t)b.nb * D4 * sizeof(float));
            pad_rows_kernel<<<dim3((unsigned)((b.nb * D4 + 255) / 256)), dim3(256), 0, st>>>(b.q, b.nb, Dm, D4, ws.qpad.as<float>());
            b.qpad = ws.qpad.as<float>();
        }
        b.D = partial ? nullptr : D + (size_t)b0 * k; b.I = partial ? nullptr : I + (size_t)b0 * k;
        b.pk = partial ? PK + (size_t)b0 * k : nullptr; b.pi = partial ? PI + (size_t)b0 * k : nullptr;
        if (adc.ok) ivfpq_search_adc(h, adc, b.q, b.qpad, b.nb, k, b.nprobe, b.D, b.I, b.pk, b.pi, b.tslot, st);
        else if (b.g.ok) ivf_search_lists(b);
        else ivf_search_exact(b);
        any_adc = any_adc || adc.ok;
        timing_mark(h, b.tslot, 2, st);
        any_mfma = any_mfma || b.g.ok;
    }
    } catch (...) {
        h->ev_used = ev_mark;
        if (h->coarse) h->coarse->small_preset = false;
        throw;
    }
    h->ivf_last_mfma = any_mfma;
    if (any_adc) h->last.last_path = VDB_PATH_IVFPQ_ADC;
}

}  // namespace

extern "C" {

int vdb_ivf_set_centroids(vdb_handle hh, const float *centroids_host, int nlist) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivf_set_centroids", kBecomesIvf);
        ivf_require(centroids_host != nullptr, VDB_ERR_INVALID, "null centroid pointer");
        ivf_require(nlist >= 1 && nlist <= (1 << 22), VDB_ERR_INVALID, "nlist out of range");
        if (h->multi) return multi_set_centroids(h, centroids_host, nlist);
        set_device(h->device);
        graph_reset(h);
        filter_drop(h);                        // (an installed filter describes the lists of the old centroids)
        h->range_valid = false;                // (... and so does the last range result)
        ivf_install_centroids(h, centroids_host, nlist);
        h->ivf_built = false;
    });
}

int vdb_ivf_get_centroids(vdb_handle hh, float *centroids_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivf_get_centroids", kIvfCalls);
        ivf_require(h->nlist > 0, VDB_ERR_STATE, "no centroids: train or set them first");
        ivf_require(centroids_host != nullptr, VDB_ERR_INVALID, "null pointer");
        if (h->multi) h = multi_first_shard(h);
        memcpy(centroids_host, h->ivf_centroids.data(), h->ivf_centroids.size() * sizeof(float));
    });
}

int vdb_ivf_train(vdb_handle hh, int nlist, const float *x_host, int64_t n, int niter, uint64_t seed,
                  int max_points_per_centroid) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivf_train", kBecomesIvf);
        ivf_require(x_host != nullptr && n > 0, VDB_ERR_INVALID, "no training vectors");
        ivf_require(nlist >= 1 && nlist <= (1 << 22), VDB_ERR_INVALID, "nlist out of range");
        ivf_require(n >= nlist, VDB_ERR_INVALID, "need at least nlist training vectors");
        ivf_require(niter >= 0 && niter <= 1000, VDB_ERR_INVALID, "niter out of range");
        if (max_points_per_centroid <= 0) max_points_per_centroid = 256;
        if (h->multi) return multi_train(h, nlist, x_host, n, niter, seed, max_points_per_centroid);
        graph_reset(h);
        set_device(h->device);
        filter_drop(h);
        h->range_valid = false;
        const int Dm = h->dim, D4 = h->D4;
        // ---- sample (seeded partial Fisher-Yates), in draw order -----------------------------------
        const int64_t ns = std::min<int64_t>(n, (int64_t)max_points_per_centroid * nlist);
        const std::vector<int64_t> pick = sample_rows(n, ns, seed);
        std::vector<float> sample((size_t)ns * Dm);
        for (int64_t i = 0; i < ns; ++i)
            memcpy(&sample[(size_t)i * Dm], x_host + (size_t)pick[(size_t)i] * Dm, (size_t)Dm * sizeof(float));
        DevBuf raw, padded, dperm, doff, dcent;
        raw.reserve((size_t)ns * Dm * 4);
        padded.reserve((size_t)ns * D4 * 4);
        VDB_HIP(hipMemcpy(raw.p, sample.data(), (size_t)ns * Dm * 4, hipMemcpyHostToDevice));
        VDB_HIP(hipMemset(padded.p, 0, (size_t)ns * D4 * 4));
        VDB_HIP(hipMemcpy2D(padded.p, (size_t)D4 * 4, sample.data(), (size_t)Dm * 4, (size_t)Dm * 4, (size_t)ns,
                            hipMemcpyHostToDevice));
        dcent.reserve((size_t)nlist * Dm * 4);
        std::vector<float> cent(sample.begin(), sample.begin() + (size_t)nlist * Dm);  // init: first nlist draws
        const int spherical = h->metric == VDB_METRIC_IP ? 1 : 0;
        std::vector<int64_t> offsets;
        DevBuf dassign;
        for (int it = 0; it < niter; ++it) {
            ivf_install_centroids(h, cent.data(), nlist);
            ivf_assign_rows(h, raw.as<float>(), ns, dassign);
            ivf_csr_build(h, dassign, ns, nlist, dperm, doff, offsets);
            VDB_HIP(hipMemcpy(dcent.p, cent.data(), (size_t)nlist * Dm * 4, hipMemcpyHostToDevice));
            centroid_update_kernel<<<dim3((unsigned)((nlist + 3) / 4)), dim3(256), 0, nullptr>>>(
                padded.as<float>(), dperm.as<int32_t>(), doff.as<int64_t>(), nlist, Dm, D4, spherical, dcent.as<float>());
            VDB_HIP(hipGetLastError());
            VDB_HIP(hipMemcpy(cent.data(), dcent.p, (size_t)nlist * Dm * 4, hipMemcpyDeviceToHost));
            // empty clusters: split the currently largest one (symmetric +-1/1024 perturbation, as FAISS does)
            std::vector<int64_t> cnt((size_t)nlist);
            for (int l = 0; l < nlist; ++l) cnt[(size_t)l] = offsets[(size_t)l + 1] - offsets[(size_t)l];
            for (int l = 0; l < nlist; ++l) {
                if (cnt[(size_t)l] != 0) continue;
                int big = 0;
                for (int j = 1; j < nlist; ++j)
                    if (cnt[(size_t)j] > cnt[(size_t)big]) big = j;
                for (int d = 0; d < Dm; ++d) {
                    const float c = cent[(size_t)big * Dm + d];
                    const float e = (d & 1) ? 1.f / 1024.f : -1.f / 1024.f;
                    cent[(size_t)l * Dm + d] = c * (1.f + e);
                    cent[(size_t)big * Dm + d] = c * (1.f - e);
                }
                cnt[(size_t)l] = cnt[(size_t)big] / 2;
                cnt[(size_t)big] -= cnt[(size_t)l];
            }
        }
        ivf_install_centroids(h, cent.data(), nlist);
        h->ivf_built = false;
        if (sq8(h)) sq8_train_ranges(h, x_host, n);      // SQ8: then the residual ranges, against these centroids
    });
}

int vdb_ivf_set_codec(vdb_handle hh, int codec) {
    return guarded([&] {
        auto *h = check(hh);
        // codec 0 is what every handle has: admitted as the other IVF calls are (a no-op on a multi-device handle)
        const bool coded = codec >= 1 && codec <= 3;
        admit(h, codec == 1 ? "the SQ8 codec" : codec == 2 ? "the IVF-PQ codec" : codec == 3 ? "the IVF-I8 codec" : "vdb_ivf_set_codec", coded ? kFlat | kIvf : kIvfCalls);
        ivf_require(codec >= 0 && codec <= 3, VDB_ERR_INVALID, "codec must be 0 (Flat), 1 (SQ8), 2 (PQ) or 3 (I8)");
        if (h->multi) return;
        ivf_require(h->nlist == 0 && h->N == 0, VDB_ERR_STATE, "the codec is chosen before centroids or rows exist");
        ivf_require(codec != 3 || h->dim <= 128, VDB_ERR_UNSUPPORTED, "the IVF-I8 codec serves dim <= 128 (the int8 list scan and the int8 row pitch)");
        if (coded) refuse_options_set(h, "vdb_ivf_set_codec", codec == 1 ? kIvfSq8 : codec == 2 ? kIvfPq : kIvfI8);
        if (codec != 2) {                       // (codebooks belong to codec 2)
            h->ivfpq = PqCodebooks{};
            h->kept.ivfpq_cb.release();
        }
        h->ivf_codec = codec;
    });
}

int vdb_ivf_sq8_train_ranges(vdb_handle hh, const float *x_host, int64_t n) {
    return guarded([&] {
        auto *h = check(hh);
        admit_sq8(h, "vdb_ivf_sq8_train_ranges");
        ivf_require(h->nlist > 0 && h->coarse, VDB_ERR_STATE, "no centroids: train or set them first");
        ivf_require(x_host != nullptr && n > 0, VDB_ERR_INVALID, "no training vectors");
        set_device(h->device);
        sq8_train_ranges(h, x_host, n);
        h->ivf_built = false;                           // (rows encoded under the old ranges are dropped by the next add)
    });
}

int vdb_ivf_sq8_set_ranges(vdb_handle hh, const float *vmin_host, const float *vdiff_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit_sq8(h, "vdb_ivf_sq8_set_ranges");
        ivf_require(vmin_host && vdiff_host, VDB_ERR_INVALID, "null pointer");
        for (int d = 0; d < h->dim; ++d)
            ivf_require(std::isfinite(vmin_host[d]) && std::isfinite(vdiff_host[d]) && vdiff_host[d] >= 0.f, VDB_ERR_INVALID,
                        "SQ8 ranges must be finite with vdiff >= 0");
        h->sq8_vmin.assign(vmin_host, vmin_host + h->dim);
        h->sq8_vdiff.assign(vdiff_host, vdiff_host + h->dim);
        h->sq8_ranges = true;
        h->ivf_built = false;
    });
}

int vdb_ivf_sq8_get_ranges(vdb_handle hh, float *vmin_host, float *vdiff_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit_sq8(h, "vdb_ivf_sq8_get_ranges");
        ivf_require(h->sq8_ranges, VDB_ERR_STATE, "no SQ8 ranges: train the index or set them first");
        ivf_require(vmin_host && vdiff_host, VDB_ERR_INVALID, "null pointer");
        memcpy(vmin_host, h->sq8_vmin.data(), (size_t)h->dim * sizeof(float));
        memcpy(vdiff_host, h->sq8_vdiff.data(), (size_t)h->dim * sizeof(float));
    });
}

int vdb_ivf_get_codes(vdb_handle hh, uint8_t *codes_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit_sq8(h, "vdb_ivf_get_codes");
        ivf_get_codes(h, h->codes.sq8_codes, (size_t)h->D4, (size_t)h->dim, codes_host);
    });
}

int vdb_ivf_i8_get_rows(vdb_handle hh, int8_t *rows_host, int *cx) {
    return guarded([&] {
        auto *h = check(hh);
        admit_ivf_i8(h, "vdb_ivf_i8_get_rows");
        ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
        ivf_require(cx != nullptr, VDB_ERR_INVALID, "null pointer");
        *cx = h->i8_cx;
        if (rows_host) ivf_get_codes(h, h->scan.rows8, (size_t)h->rows8_pitch, (size_t)h->dim, reinterpret_cast<uint8_t *>(rows_host));
    });
}

int vdb_ivfpq_set_codebooks(vdb_handle hh, int M, const float *codebooks_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit_ivfpq(h, "vdb_ivfpq_set_codebooks");
        pq_check_M(h, M);
        ivf_require(codebooks_host != nullptr, VDB_ERR_INVALID, "null codebook pointer");
        set_device(h->device);
        ivfpq_install_codebooks(h, M, codebooks_host);
    });
}

int vdb_ivfpq_get_codebooks(vdb_handle hh, int *M, float *codebooks_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivfpq_get_codebooks", kAnyKind);
        pq_get_codebooks(h->ivfpq, kind_of(h) == kIvfPq, M, codebooks_host);
    });
}

int vdb_ivfpq_train(vdb_handle hh, int M, const float *x_host, int64_t n, int niter, uint64_t seed, int max_points_per_centroid) {
    return guarded([&] {
        auto *h = check(hh);
        admit_ivfpq(h, "vdb_ivfpq_train");
        pq_check_M(h, M);
        ivf_require(h->nlist > 0 && h->coarse, VDB_ERR_STATE, "no centroids: train or set them first");
        pq_check_train_args(x_host, n, niter, max_points_per_centroid);
        set_device(h->device);
        // the row sample of vdb_pq_train, then its residuals against the installed centroids: r = x - c_l, one float32
        // subtraction per dimension
        const int D = h->dim;
        std::vector<float> res = pq_training_sample(x_host, n, D, seed, max_points_per_centroid);
        const int64_t ns = (int64_t)(res.size() / (size_t)D);
        {
            DevBuf dx, dassign;
            dx.reserve((size_t)ns * D * sizeof(float));
            VDB_HIP(hipMemcpy(dx.p, res.data(), (size_t)ns * D * sizeof(float), hipMemcpyHostToDevice));
            ivf_assign_rows(h, dx.as<float>(), ns, dassign);
            std::vector<int64_t> assign((size_t)ns);
            VDB_HIP(hipMemcpy(assign.data(), dassign.p, (size_t)ns * sizeof(int64_t), hipMemcpyDeviceToHost));
            sq8_release_coarse_ws(h);
            for (int64_t i = 0; i < ns; ++i) {
                ivf_require(assign[(size_t)i] >= 0 && assign[(size_t)i] < h->nlist, VDB_ERR_INVALID, "row could not be assigned to a list");
                const float *c = &h->ivf_centroids[(size_t)assign[(size_t)i] * D];
                float *r = &res[(size_t)i * D];
                for (int d = 0; d < D; ++d) r[d] = r[d] - c[d];
            }
        }
        const std::vector<float> cb = pq_train_codebooks(h->device, res, D, M, niter, seed, max_points_per_centroid);
        ivfpq_install_codebooks(h, M, cb.data());
    });
}

int vdb_ivfpq_add_codes(vdb_handle hh, const uint8_t *codes_host, int64_t n, int64_t id_base, const int32_t *list_of_row_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit_ivfpq(h, "vdb_ivfpq_add_codes");
        ivf_require(n >= 0 && (n == 0 || (codes_host && list_of_row_host)), VDB_ERR_INVALID, "null code or assignment pointer");
        ivfpq_add(h, nullptr, codes_host, n, id_base, list_of_row_host);
    });
}

int vdb_ivfpq_get_codes(vdb_handle hh, uint8_t *codes_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit_ivfpq(h, "vdb_ivfpq_get_codes");
        ivf_get_codes(h, h->codes.ivfpq_codes, (size_t)h->ivfpq.M, (size_t)h->ivfpq.M, codes_host);
    });
}

int vdb_debug_ivfpq_adc_scores(vdb_handle hh, const float *q_host, int64_t nq, int probe_list, int64_t row0, int64_t nrows, float *scores_host,
                               float *eps_host, double *cscale) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_debug_ivfpq_adc_scores", kIvfPq);
        ivfpq_adc_debug_scores(h, q_host, nq, probe_list, row0, nrows, scores_host, eps_host, cscale);
    });
}

}  // extern "C"

namespace {
// vdb_ivf_add / vdb_ivf_add_assigned: APPEND to the inverted lists, as faiss.IndexIVF.add does (ivf_add_lists).  `given`
// (optional, host, int32 [n]) = the list of every row, as stored by a persisted index; without it the rows are assigned to
// their nearest centroid here.
int ivf_add_impl(vdb_handle hh, const float *x_host, int64_t n, int64_t id_base, const int32_t *given) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, given ? "vdb_ivf_add_assigned" : "vdb_ivf_add", kIvfCalls);      // (a sign-LSH or k-NN graph handle is told "no centroids" below, not that it stays flat)
        if (h->multi) {
            if (h->nlist > 0 && n > 0) ivf_check_given(h, given, n);      // (a shard that refused its block would empty the whole index)
            return multi_add(h, x_host, false, n, id_base, nullptr, true, given);
        }
        if (sq8(h)) return sq8_add(h, x_host, n, id_base, given);
        if (ivfpq(h)) return ivfpq_add(h, x_host, nullptr, n, id_base, given);
        if (ivf_i8(h)) return i8_add(h, x_host, n, id_base, given);
        ivf_require(h->nlist > 0 && h->coarse, VDB_ERR_STATE, "no centroids: train or set them first");
        ivf_require(n >= 0 && (n == 0 || x_host), VDB_ERR_INVALID, "bad corpus");
        int64_t N0, N1;
        const bool rows_change = ivf_add_range(h, n, id_base, N0, N1);
        ivf_check_given(h, given, n);
        // an installed filter (ivf_filter.inc) has one bit per row, and the rows change place: every add that passed its checks drops
        // it, an empty append too; a refused add leaves it with the index.  (The coded indexes above never hold one.)
        filter_drop(h);
        h->range_valid = false;                // (the last range result, ivf_range.inc, goes the same way)
        if (!rows_change) return;
        set_device(h->device);
        const int Dm = h->dim, D4 = h->D4;
        graph_reset(h);
        VDB_HIP(hipDeviceSynchronize());
        h->ivf_built = false;
        h->built = false;
        std::vector<int64_t> assign_new((size_t)n);
        if (N1 > 0) {
            DevBuf src, src_ids, dperm, doff;
            // ONE pass over the host rows (row blocks through the pinned staging buffers); the unpadded copy the coarse
            // assignment reads is made on the device
            src.reserve((size_t)N1 * D4 * 4);
            if (N0) VDB_HIP(hipMemcpy(src.p, h->rows.x32.p, (size_t)N0 * D4 * 4, hipMemcpyDeviceToDevice));
            float *fresh = src.as<float>() + (size_t)N0 * D4;
            if (D4 != Dm) VDB_HIP(hipMemset(fresh, 0, (size_t)n * D4 * 4));
            upload_rows(h, fresh, D4, x_host, n, Dm, nullptr);
            if (given) {        // stored assignment: no coarse search at all
                for (int64_t i = 0; i < n; ++i) assign_new[(size_t)i] = given[i];
            } else if (n > 0) {
                DevBuf dnew;
                ivf_add_assign(h, fresh, n, dnew, assign_new);
            }
            ivf_add_lists(h, assign_new, N0, src_ids, dperm, doff);
            h->rows.x32.reserve((size_t)N1 * D4 * 4);
            h->lists.ivf_ids.reserve((size_t)N1 * 8);
            const int64_t total = N1 * (D4 / 4);
            gather_rows_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr>>>(
                src.as<float>(), dperm.as<int32_t>(), N1, D4, id_base, N0 ? src_ids.as<int64_t>() : nullptr,
                h->rows.x32.as<float>(), h->lists.ivf_ids.as<int64_t>());
            VDB_HIP(hipGetLastError());
            VDB_HIP(hipDeviceSynchronize());
        }
        ivf_add_finish(h, assign_new, N0, id_base);
        ivf_build_panel_space(h);
        h->ivf_built = true;
    });
}
// vdb_ivf_search_device (graph key kind 3: final rows D, I) and vdb_ivf_search_partial_device (kind 4: partial rows pk, pi)
int ivf_search_device_entry(vdb_handle hh, const float *q_dev, int64_t nq, int k, int kind, float *D, int64_t *I, double *pk,
                            int64_t *pi, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, kind == 3 ? "vdb_ivf_search_device" : "vdb_ivf_search_partial_device", kIvfCalls);
        if (h->multi) return multi_search(h, q_dev, true, nq, k, D, I, pk, pi, as_stream(stream), true);
        set_device(h->device);
        vdb_index_s::GraphKey key;
        key.q = q_dev; key.o1 = D ? (const void *)D : pk; key.o2 = D ? I : pi; key.nq = nq; key.k = k; key.kind = kind; key.nprobe = h->nprobe; key.st = as_stream(stream);
        graph_or_run(h, key, [&] { ivf_search_device_impl(h, q_dev, nq, k, D, I, pk, pi, as_stream(stream)); });
    });
}
}  // namespace

extern "C" {

int vdb_ivf_add(vdb_handle hh, const float *x_host, int64_t n, int64_t id_base) {
    return ivf_add_impl(hh, x_host, n, id_base, nullptr);
}

int vdb_ivf_add_assigned(vdb_handle hh, const float *x_host, int64_t n, int64_t id_base, const int32_t *list_of_row_host) {
    if (n > 0 && !list_of_row_host) {
        g_last_error = "null assignment pointer";
        return VDB_ERR_INVALID;
    }
    return ivf_add_impl(hh, x_host, n, id_base, list_of_row_host);
}

int vdb_ivf_set_nprobe(vdb_handle hh, int nprobe) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivf_set_nprobe", kIvfCalls);
        ivf_require(nprobe >= 1, VDB_ERR_INVALID, "nprobe must be >= 1");
        h->nprobe = std::min(nprobe, 2048);
        if (h->multi) {
            multi_for_each_shard(h, [&](vdb_index_s *c) { c->nprobe = h->nprobe; });
            return;
        }
        graph_reset(h);
    });
}

int vdb_ivf_get_assignment(vdb_handle hh, int32_t *list_of_row_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivf_get_assignment", kIvfCalls);
        ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
        ivf_require(list_of_row_host != nullptr || h->N == 0, VDB_ERR_INVALID, "null pointer");
        if (h->multi) return multi_get_assignment(h, list_of_row_host);
        if (h->N) memcpy(list_of_row_host, h->ivf_list_of_row.data(), (size_t)h->N * sizeof(int32_t));
    });
}

int vdb_ivf_search_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                          void *stream) {
    return ivf_search_device_entry(hh, q_dev, nq, k, 3, D_dev, I_dev, nullptr, nullptr, stream);
}

int vdb_ivf_search_partial_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, double *keys_dev,
                                  int64_t *ids_dev, void *stream) {
    return ivf_search_device_entry(hh, q_dev, nq, k, 4, nullptr, nullptr, keys_dev, ids_dev, stream);
}

// vdb_reserve: size the workspace of an nq-query, top-k search NOW (index build time) instead of inside the first search:
// one untimed search of nq queries taken from the corpus rows themselves (typical candidate counts, no degenerate ties),
// through the host-API staging buffers.  The reference harness times its very first batch_search, allocation included
// (experiment_runner.py:431-437, no warm-up): FAISS' GPU resources reserve their scratch memory at construction too.
int vdb_reserve(vdb_handle hh, int64_t nq, int k) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_reserve", kAnyKind);
        if (h->multi) return multi_reserve(h, nq, k);
        ivf_require(h->built || h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
        ivf_require(k >= 1 && k <= 2048, VDB_ERR_INVALID, "k must be in [1, 2048]");
        ivf_require(nq >= 0 && nq <= (1ll << 24), VDB_ERR_INVALID, "query count out of range");
        if (nq == 0 || h->N == 0) return;
        set_device(h->device);
        // the host-API transfers of that batch once, from / to a scratch host buffer: the runtime sets up its staging for
        // pageable copies of this size on first use
        const size_t row = (size_t)h->dim * sizeof(float);
        std::vector<char> host(std::max((size_t)nq * row, (size_t)nq * k * (sizeof(int64_t) + sizeof(float))));
        int64_t *I = reinterpret_cast<int64_t *>(host.data());
        float *D = reinterpret_cast<float *>(host.data() + (size_t)nq * k * sizeof(int64_t));
        run_staged(h, reinterpret_cast<const float *>(host.data()), nq, k, D, I, [&](float *dq, float *dD, int64_t *dI, hipStream_t st) {
            for (int64_t q0 = 0; q0 < nq; q0 += h->N) {      // queries = corpus rows (wrapping around a corpus smaller than the batch)
                const int64_t m = std::min<int64_t>(h->N, nq - q0);
                if (h->int8_only || ivf_i8(h))     // (no float32 rows: the int8 rows, converted)
                    rows_i8_to_float_kernel<<<dim3((unsigned)((m * h->dim + 255) / 256)), dim3(256), 0, st>>>(
                        h->scan.rows8.as<signed char>(), h->rows8_pitch, h->i8_cx, m, h->dim, dq + (size_t)q0 * h->dim);
                else if (pq_on(h))    // (product codes: the looked-up rows x^)
                    pq_decode_rows(h, 0, m, h->dim, dq + (size_t)q0 * h->dim, st);
                else if (ivfpq(h))    // (residual product codes: the decoded rows x^)
                    ivfpq_decode_rows(h, m, h->dim, dq + (size_t)q0 * h->dim, st);
                else if (sq8(h))      // (codes: the decoded rows x^)
                    sq8_decode_rows_kernel<<<dim3((unsigned)std::min<int64_t>((m * h->dim + 255) / 256, 1 << 20)), dim3(256), 0, st>>>(
                        sq8_rows(h), m, h->dim, h->D4, h->dim, dq + (size_t)q0 * h->dim);
                else
                    VDB_HIP(hipMemcpy2DAsync(reinterpret_cast<char *>(dq) + (size_t)q0 * row, row, h->rows.x32.p, (size_t)h->D4 * sizeof(float), row,
                                             (size_t)m, hipMemcpyDeviceToDevice, st));
            }
            if (h->ivf_built) ivf_search_device_impl(h, dq, nq, k, dD, dI, nullptr, nullptr, st);
            else search_device_impl(h, dq, nq, k, dD, dI, nullptr, nullptr, st);
        });
    });
}

int vdb_ivf_search(vdb_handle hh, const float *q_host, int64_t nq, int k, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_ivf_search", kIvfCalls);
        ivf_require(h->ivf_built, VDB_ERR_STATE, "Index has not been built yet.");
        ivf_require(k >= 1 && k <= 2048, VDB_ERR_INVALID, "k must be in [1, 2048]");
        if (nq <= 0) {
            ivf_require(nq == 0, VDB_ERR_INVALID, "negative query count");
            return;
        }
        ivf_require(q_host && D && I, VDB_ERR_INVALID, "null pointer");
        if (h->multi) return multi_search(h, q_host, false, nq, k, D, I, nullptr, nullptr, nullptr, true);
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            ivf_search_device_impl(h, dq, nq, k, dD, dI, nullptr, nullptr, st);
        });
    });
}

}  // extern "C"

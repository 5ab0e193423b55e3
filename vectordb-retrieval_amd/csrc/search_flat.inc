// search_flat.inc -- the flat (brute-force) search path of vdbhip.hip: the table of scan kernels and `launch` (which scan, and in
// which shape, is decided in scan_plan.hpp), one query batch (search_batch), hipGraph replay, the per-call driver
// (search_device_impl).  Included inside vdbhip.hip's anonymous namespace; not a translation unit of its own.

// ---- path and launch shape of the scans: scan_plan.hpp decides, this file fills arguments and launches ------------------------
// what the rules of scan_plan.hpp read of a handle
ScanIndexShape scan_shape_of(const vdb_index_s *h) {
    ScanIndexShape s;
    s.ksteps = h->ksteps; s.i8_ks = h->i8_ks; s.Npad = h->Npad; s.n_cus = h->n_cus;
    s.tile16 = h->tile16; s.x16 = h->x16;
    s.int8_only = h->int8_only; s.panels_streamed = h->panels_streamed; s.pq = h->pq.M > 0;
    s.i8_ok = h->i8_ok;
    return s;
}

// one row per instantiation of a family (the lists of scan_plan.hpp): its key and its kernel
template <class... Args>
struct ScanRow {
    ScanKey key;
    void (*kernel)(Args...);
};
#define VDB_ROW_SCAN(...) {ScanKey{{__VA_ARGS__}}, &scan_kernel<__VA_ARGS__>},
#define VDB_ROW_SCAN16_KLOOP(...) {ScanKey{{__VA_ARGS__}}, &scan16_kloop_kernel<__VA_ARGS__>},
#define VDB_ROW_SCAN_X16(...) {ScanKey{{__VA_ARGS__}}, &scan_x16_kernel<__VA_ARGS__>},
#define VDB_ROW_SCAN_I8(...) {ScanKey{{__VA_ARGS__}}, &scan_i8_kernel<__VA_ARGS__>},
#define VDB_ROW_SCAN_I8X16(...) {ScanKey{{__VA_ARGS__}}, &scan_i8x16_kernel<__VA_ARGS__>},
#define VDB_ROW_SCAN_PAIR_X16(...) {ScanKey{{__VA_ARGS__}}, &scan_pair_x16_kernel<__VA_ARGS__>},
constexpr ScanRow<ScanArgs> kRowsScan[] = {VDB_KERNELS_SCAN(VDB_ROW_SCAN)};
constexpr ScanRow<ScanArgs, ScanKloopExtra> kRowsScan16Kloop[] = {VDB_KERNELS_SCAN16_KLOOP(VDB_ROW_SCAN16_KLOOP)};
constexpr ScanRow<ScanArgs> kRowsScanX16[] = {VDB_KERNELS_SCAN_X16(VDB_ROW_SCAN_X16)};
constexpr ScanRow<ScanI8Args> kRowsScanI8[] = {VDB_KERNELS_SCAN_I8(VDB_ROW_SCAN_I8)};
constexpr ScanRow<ScanI8Args> kRowsScanI8x16[] = {VDB_KERNELS_SCAN_I8X16(VDB_ROW_SCAN_I8X16)};
constexpr ScanRow<ScanArgs, ScanI8Args> kRowsScanPairX16[] = {VDB_KERNELS_SCAN_PAIR_X16(VDB_ROW_SCAN_PAIR_X16)};
#undef VDB_ROW_SCAN
#undef VDB_ROW_SCAN16_KLOOP
#undef VDB_ROW_SCAN_X16
#undef VDB_ROW_SCAN_I8
#undef VDB_ROW_SCAN_I8X16
#undef VDB_ROW_SCAN_PAIR_X16

template <class Row, size_t N, class Launch>     // Launch: ScanLaunch, or IvfLaunch (ivf.inc)
auto scan_kernel_of(const Row (&rows)[N], const Launch &p) {
    for (const Row &r : rows)
        if (r.key == p.key) return r.kernel;
    std::string what = kScanFamilyNames[(int)p.family];
    for (int i = 0; i < kScanFamilyArgs[(int)p.family]; ++i) what += (i ? ", " : "<") + std::to_string(p.key.t[i]);
    throw Error(VDB_ERR_INVALID, "internal: no scan kernel for " + what + ">");
}

// the one <<<>>> of the plan's family; sa: the fp16 scan's arguments, s8: the int8 scan's (the pair takes both)
void launch(const ScanLaunch &p, const vdb_index_s *h, const ScanArgs *sa, const ScanI8Args *s8, hipStream_t st) {
    const dim3 grid(p.grid), block(p.block);
    ScanArgs a{};
    ScanI8Args a8{};
    if (sa) { a = *sa; a.nqtiles = p.nqtiles; }
    if (s8) { a8 = *s8; a8.nqtiles = p.family == ScanFamily::scan_pair_x16 ? p.nqtiles8 : p.nqtiles; }
    switch (p.family) {
        case ScanFamily::scan: scan_kernel_of(kRowsScan, p)<<<grid, block, 0, st>>>(a); break;
        case ScanFamily::scan16_kloop: scan_kernel_of(kRowsScan16Kloop, p)<<<grid, block, 0, st>>>(a, ScanKloopExtra{h->ksteps, p.qgroup}); break;
        case ScanFamily::scan_x16: scan_kernel_of(kRowsScanX16, p)<<<grid, block, 0, st>>>(a); break;
        case ScanFamily::scan_i8: scan_kernel_of(kRowsScanI8, p)<<<grid, block, 0, st>>>(a8); break;
        case ScanFamily::scan_i8x16: scan_kernel_of(kRowsScanI8x16, p)<<<grid, block, 0, st>>>(a8); break;
        case ScanFamily::scan_pair_x16: scan_kernel_of(kRowsScanPairX16, p)<<<grid, block, 0, st>>>(a, a8); break;
        default: throw Error(VDB_ERR_INVALID, "internal: no scan kernel for an empty plan");
    }
    VDB_HIP(hipGetLastError());
}

template <int VPL>
void launch_select(const SelectArgs &a, hipStream_t st) {
    select_kernel<VPL><<<dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, st>>>(a);
}

long timing_begin(vdb_index_s *h, hipStream_t st) {
    if (!h->opt.timing || h->ev_used >= kMaxTimedCalls) return -1;
    const size_t slot = h->ev_used++;
    while (h->ev_scan.size() < 2 * (slot + 1)) {
        hipEvent_t e;
        VDB_HIP(hipEventCreate(&e));
        h->ev_scan.push_back(e);
        VDB_HIP(hipEventCreate(&e));
        h->ev_total.push_back(e);
    }
    VDB_HIP(hipEventRecord(h->ev_total[2 * slot], st));
    return (long)slot;
}

// which: 0 = dominant kernel starts, 1 = dominant kernel done, 2 = pipeline done
void timing_mark(vdb_index_s *h, long slot, int which, hipStream_t st) {
    if (slot < 0) return;
    hipEvent_t e = which == 0 ? h->ev_scan[2 * slot] : which == 1 ? h->ev_scan[2 * slot + 1] : h->ev_total[2 * slot + 1];
    VDB_HIP(hipEventRecord(e, st));
}

// PQ index (pq.inc): the smallest batch that takes the panel pass + MFMA scan (measured, profiles/r07_bench_pq.json)
constexpr int64_t kPqScanMinBatch = 1;

// ---- one query batch ---------------------------------------------------------------------------------
// What the three paths of a batch share: search_batch fills it, search_dense / search_exact / search_scan read it.
// outputs: final (D,I) or partial (pk,pi); all device pointers for rows [0,nq) of this batch
struct Batch {
    vdb_index_s *h;
    Workspace &ws;
    const float *dq;
    int64_t nq;
    int k;
    float *D; int64_t *I; double *pk; int64_t *pi;
    hipStream_t st;
    RefineCommon rc;
    ScanGeom g;
    ScanIndexShape shape;        // scan_shape_of(h)
    int direct_rows;
    int32_t *fb_count;
    unsigned long long *stat_counters;
    long tslot;                  // timing_begin
    bool clear_in_prep;          // workgroup 0 of query_prep_kernel clears ws.small (search_batch)
    bool adc;                    // PQ: the bin records come from the lookup-table scan of the codes (search_scan_adc), not from panels
    const float *bias;           // accumulator inits the scans of this batch read: the handle's, or (a filtered search, filter.inc) the
    const int32_t *bias8;        // masked copies of its filter -- rc.allow is set with them
};

// the S partial lists per slot that an exhaustive pass (fa) left in its (pkeys, pids), merged into the outputs of the batch
void merge_splits(const Batch &b, const RefineFullArgs &fa, int64_t max_slots) {
    MergeArgs ma{};
    ma.pkeys = fa.pkeys; ma.pids = fa.pids;
    ma.part_stride = b.k; ma.slot_stride = (int64_t)fa.S * b.k; ma.nparts = fa.S;
    ma.k = b.k; ma.metric = b.h->metric;
    ma.qlist = fa.qlist; ma.count_ptr = fa.count_ptr; ma.count = fa.count;       // (the slots of the pass)
    ma.D = b.D; ma.I = b.I; ma.okeys = b.pk; ma.oids = b.pi;
    launch_merge(ma, max_slots, b.st);
}

// small corpora: dense fp16 scores + per-query guard + exact re-score of the few surviving rows
// (D > 128: corpora of <= 2048 rows keep 32-row tiles for exactly this path -- build_derived -- and take the K-loop form)
void search_dense(const Batch &b) {
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const float *dq = b.dq;
    const int64_t nq = b.nq;
    const int k = b.k, Dm = h->dim, D4 = h->D4;
    hipStream_t st = b.st;
    const int64_t Qp = (nq + 63) / 64 * 64;
    const int cand_cap = std::max(128, 2 * k + 64);
    ws.qpanels.reserve((size_t)(Qp / 32) * h->ksteps * 64 * sizeof(half8));
    ws.eps.reserve((size_t)nq * sizeof(float));
    ws.dense.reserve((size_t)Qp * h->Npad * sizeof(float));
    ws.fallback.reserve((size_t)nq * sizeof(int32_t));
    ws.fb_list.reserve((size_t)nq * sizeof(int32_t));
    QueryBatchInfo *info = batch_info(ws);          // (zeroed with fb_count above)
    const int64_t total = nq * Dm;
    const FinalizeArgs fin{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2, 0};
    const bool fused_stats = total <= kFusedStatsMax && h->opt.fused_stats;     // (serving shapes: statistics inside the prep kernel)
    if (!fused_stats) query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, st>>>(dq, total, info, fin);
    h->info_valid_nq = nq;
    const int64_t threads = (Qp / 32) * h->ksteps * 64;
    EpsArgs ea{dq, nq, Dm, h->ksteps * 16, h->metric, sqrtf(h->maxnorm2) * 1.0000002f,
               h->corpus_fp16_exact ? 1 : 0, h->corpus_int_unscaled ? 1 : 0, h->sx, info, ws.eps.as<float>()};
    {   // fp16 fragments and error bounds in ONE dispatch (query_prep_kernel without its int8 regions)
        QueryPrepArgs qp{};
        qp.Q = dq; qp.nq = nq; qp.nqtiles = Qp / 32;
        qp.D = Dm; qp.D4 = D4; qp.ksteps = h->ksteps;
        qp.info = info;
        qp.qpanels = ws.qpanels.as<half8>();
        qp.eps = ea;
        qp.nA = qp.nB = qp.nC = (unsigned)((threads + 255) / 256);
        qp.fused_stats = fused_stats ? 1 : 0; qp.fin = fin; qp.info_out = info;
        query_prep_kernel<<<dim3(qp.nC + (unsigned)((nq * 16 + 255) / 256)), dim3(256), 0, st>>>(qp);
    }
    // (<= 256 rows sit in the lower half of the one span: tiles past them hold padding only and the register select never reads
    //  their columns)
    const int64_t ntiles = (h->N <= 256 && h->Npad <= 2048 && kpl_for(k) <= 4) ? ((h->N + 63) / 64 * 64) / 16 : h->Npad / kTileRows;
    timing_mark(h, b.tslot, 0, st);
    {
        const dim3 grid((unsigned)((ntiles + 3) / 4), (unsigned)(Qp / 64));
        if (h->ksteps > kMaxKSteps)
            dense_scores_kloop_kernel<<<grid, dim3(256), 0, st>>>(h->scan.panels.as<half8>(), b.bias,
                                                                 ws.qpanels.as<half8>(), info, ntiles, h->Npad, h->N,
                                                                 h->ksteps, ws.dense.as<float>());
        else if (h->ksteps == 4)
            dense_scores_kernel<4><<<grid, dim3(256), 0, st>>>(h->scan.panels.as<half8>(), b.bias,
                                                              ws.qpanels.as<half8>(), info, ntiles, h->Npad,
                                                              ws.dense.as<float>());
        else
            dense_scores_kernel<8><<<grid, dim3(256), 0, st>>>(h->scan.panels.as<half8>(), b.bias,
                                                              ws.qpanels.as<half8>(), info, ntiles, h->Npad,
                                                              ws.dense.as<float>());
    }
    timing_mark(h, b.tslot, 1, st);
    DenseSelectArgs da{};
    da.c = b.rc;
    da.scores = ws.dense.as<float>();
    da.eps = ws.eps.as<float>();
    da.info = info;
    da.nq = nq;
    da.Npad = h->Npad;
    da.cand_cap = cand_cap;
    da.fallback = ws.fallback.as<int32_t>();
    da.fb_list = ws.fb_list.as<int32_t>();
    da.fb_count = b.fb_count;
    da.stat_counters = b.stat_counters;
    da.D = b.D;
    da.I = b.I;
    da.pkeys = b.pk;
    da.pids = b.pi;
    da.set_only = (h->set_only && b.D != nullptr) ? 1 : 0;
    const bool reg_select = h->Npad <= 2048 && kpl_for(k) <= 4;
    da.inline_fallback = reg_select ? 1 : 0;
    // columns the register select reads: rows of the index rounded up to a lane row (<= 256 rows: all in the lower half of
    // the one span, so the columns beyond hold padding scores only)
    const int64_t ncols = h->N <= 256 ? (h->N + 63) / 64 * 64 : h->Npad;
    da.ncols = reg_select ? ncols : 0;
    {
        const int kpl = kpl_for(k);
        if (reg_select) {       // scores in registers, 4 queries per workgroup (dense.hpp)
            const dim3 g4((unsigned)((nq + 3) / 4));
            const size_t lds4 = (size_t)4 * 2 * cand_cap * 4;       // per wave: candidate rows + their keys
            if (ncols <= 256 && kpl <= 2) {
                DISPATCH_KPL(kpl, (dense_select_reg_kernel<(KPL <= 2 ? KPL : 2), 4><<<g4, dim3(256), lds4, st>>>(da)));
            } else if (ncols <= 512) {
                DISPATCH_KPL(kpl, (dense_select_reg_kernel<(KPL <= 4 ? KPL : 4), 8><<<g4, dim3(256), lds4, st>>>(da)));
            } else if (h->Npad <= 1024) {
                DISPATCH_KPL(kpl, (dense_select_reg_kernel<(KPL <= 4 ? KPL : 4), 16><<<g4, dim3(256), lds4, st>>>(da)));
            } else {
                DISPATCH_KPL(kpl, (dense_select_reg_kernel<(KPL <= 4 ? KPL : 4), 32><<<g4, dim3(256), lds4, st>>>(da)));
            }
        } else {
            const size_t lds = (size_t)(h->Npad + cand_cap) * 4;
            DISPATCH_KPL(kpl, (dense_select_kernel<KPL><<<dim3((unsigned)nq), dim3(64), lds, st>>>(da)));
        }
        VDB_HIP(hipGetLastError());
    }
    if (reg_select) {       // (flagged queries were served inside the select kernel)
        timing_mark(h, b.tslot, 2, st);
        h->last.last_path = VDB_PATH_MFMA_SCAN;
        return;
    }
    // queries whose candidate list overflowed (or unusable scales): exhaustive exact pass
    int64_t S = std::min<int64_t>(16, std::max<int64_t>(1, h->N / 1024));
    const int64_t cap = std::max<int64_t>(1, (int64_t)(256ll << 20) / (nq * k * 16));
    S = std::max<int64_t>(1, std::min<int64_t>(S, cap));
    ws.pkeys.reserve((size_t)nq * S * k * sizeof(double));
    ws.pids.reserve((size_t)nq * S * k * sizeof(int64_t));
    RefineFullArgs fa{};
    fa.c = b.rc;
    fa.qlist = da.fb_list;
    fa.count_ptr = b.fb_count;
    fa.S = (int)S;
    fa.rows_per_split = (h->N + S - 1) / S;
    if (S == 1 && b.D) {       // one split: the exhaustive pass writes the final rows itself, nothing to merge
        fa.D = b.D;
        fa.I = b.I;
        launch_refine_full(fa, 1024, st);
    } else {
        fa.pkeys = ws.pkeys.as<double>();
        fa.pids = ws.pids.as<int64_t>();
        launch_refine_full(fa, 1024, st);
        merge_splits(b, fa, 256);
    }
    timing_mark(h, b.tslot, 2, st);
    h->last.last_path = VDB_PATH_MFMA_SCAN;
}

// exhaustive exact scan, split over S waves per query (per group of 4 queries in the query-blocked form,
// which fetches every row once for the four: k <= 128, at least 4 queries)
// (it needs enough (group, split) units to fill the chip: small corpora and tiny batches keep the one-query form)
void search_exact(const Batch &b) {
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const int64_t nq = b.nq;
    hipStream_t st = b.st;
    const int k = b.k;
    bool blocked = kpl_for(k) <= 2 && nq >= 2 * kRefineQB && h->opt.force_path != 3;
    if (blocked) {
        const int64_t g4 = (nq + kRefineQB - 1) / kRefineQB;
        const int64_t s4 = std::min<int64_t>((4096 + g4 - 1) / g4, std::max<int64_t>(1, h->N / 2048));
        blocked = g4 * s4 >= 1024;
    }
    const int64_t ngroups = blocked ? (nq + kRefineQB - 1) / kRefineQB : nq;
    auto launch_full = [&](const RefineFullArgs &fa) {
        if (blocked) launch_refine_full_blocked(fa, ngroups * fa.S, st);
        else launch_refine_full(fa, nq * fa.S, st);
    };
    int64_t S = ((blocked ? 4096 : 8192) + ngroups - 1) / ngroups;
    // (a split is worth >= 1024 rows; the blocked form merges 4x the partial lists per unit, so its splits are larger)
    S = std::min<int64_t>(S, std::max<int64_t>(1, h->N / (blocked ? 2048 : 1024)));
    // a handful of queries on a small corpus (an IVF coarse quantizer asked for 1..63 queries): one wave per query
    // would walk all rows alone (92 us for 8 queries x 1024 centroids) -- up to 64 splits of >= 128 rows instead
    if (!blocked && nq < 64) S = std::max<int64_t>(S, std::min<int64_t>(64, h->N / 128));
    const int64_t cap = std::max<int64_t>(1, (int64_t)(256ll << 20) / (nq * k * 16));
    S = std::max<int64_t>(1, std::min<int64_t>(S, cap));
    RefineFullArgs fa{};
    fa.c = b.rc;
    fa.count = nq;
    fa.S = (int)S;
    fa.rows_per_split = ((h->N + S - 1) / S + 63) / 64 * 64;     // whole 64-row wave iterations
    if (fa.rows_per_split < 64) fa.rows_per_split = 64;
    timing_mark(h, b.tslot, 0, st);
    if (S == 1 && b.D) {
        fa.D = b.D;
        fa.I = b.I;
        launch_full(fa);
    } else if (S == 1) {
        fa.pkeys = b.pk;
        fa.pids = b.pi;
        launch_full(fa);
    } else {
        ws.pkeys.reserve((size_t)nq * S * k * sizeof(double));
        ws.pids.reserve((size_t)nq * S * k * sizeof(int64_t));
        fa.pkeys = ws.pkeys.as<double>();
        fa.pids = ws.pids.as<int64_t>();
        launch_full(fa);
        merge_splits(b, fa, nq);
    }
    h->last.last_path = VDB_PATH_EXACT_SCAN;
    timing_mark(h, b.tslot, 1, st);
    timing_mark(h, b.tslot, 2, st);
}

// ---- MFMA scan path ------------------------------------------------------------------------------
// step 1: batch statistics, B fragments of both scans, int8 query rows, error bounds
void scan_query_prep(const Batch &b, int64_t Qpad, bool use_i8, QueryBatchInfo *info) {
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const float *dq = b.dq;
    const int64_t nq = b.nq;
    const int Dm = h->dim, D4 = h->D4;
    hipStream_t st = b.st;
    const int64_t total = nq * Dm;
    const FinalizeArgs fin{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2,
                           use_i8 ? (1 | ((h->opt.i8_group == 8 || h->x16) ? 4 : 0)) : 0};      // (layout "x16": octs only)
    const bool fused_stats = total <= kFusedStatsMax && !h->tile16 && h->opt.fused_stats;   // (serving shapes, scan_i8.hpp)
    if (!fused_stats) query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, st>>>(dq, total, info, fin);
    h->info_valid_nq = nq;
    EpsArgs ea{dq, nq, Dm, h->ksteps * 16, h->metric, sqrtf(h->maxnorm2) * 1.0000002f,
               h->corpus_fp16_exact ? 1 : 0, h->corpus_int_unscaled ? 1 : 0, h->sx, info, ws.eps.as<float>()};
    const int64_t threads = (Qpad / 32) * h->ksteps * 64;      // (same element count in both layouts)
    if (h->tile16) {
        build_qpanels16_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(dq, nq, Dm, h->ksteps / 2, Qpad / 16, info, ws.qpanels.as<half8>());
        query_eps_kernel<<<dim3((unsigned)((nq * 16 + 255) / 256)), dim3(256), 0, st>>>(ea);
    } else {            // one dispatch: fp16 fragments | int8 fragments | int8 query rows | error bounds (scan_i8.hpp)
        QueryPrepArgs qp{};
        qp.Q = dq; qp.nq = nq; qp.nqtiles = Qpad / 32;
        qp.D = Dm; qp.D4 = D4; qp.ksteps = h->ksteps; qp.ks32 = h->i8_ks; qp.pitch8 = h->rows8_pitch;
        qp.info = info;
        qp.qpanels = ws.qpanels.as<half8>();
        qp.x16 = h->x16 ? 1 : 0;          // (both B-fragment forms follow the layout of the scan copies)
        qp.eps = ea;
        unsigned nblk = (unsigned)((threads + 255) / 256);
        qp.nA = nblk;
        if (use_i8) {   // (the int8 regions return at once unless the device chose the int8 scan for this batch)
            ws.qpanels8.reserve((size_t)(Qpad / 32) * h->i8_ks * 64 * sizeof(int4v));
            qp.qpanels8 = ws.qpanels8.as<int4v>();
            nblk += (unsigned)(((Qpad / 32) * h->i8_ks * 64 + 255) / 256);
        }
        qp.nB = nblk;
        if (use_i8 && b.rc.Q8) {
            qp.qrows8 = ws.qrows8.as<signed char>();
            nblk += (unsigned)((nq * h->rows8_pitch + 255) / 256);
        }
        qp.nC = nblk;
        nblk += (unsigned)((nq * 16 + 255) / 256);
        qp.fused_stats = fused_stats ? 1 : 0; qp.fin = fin; qp.info_out = info;
        if (b.clear_in_prep) {
            if (!fused_stats) throw Error(VDB_ERR_STATE, "ws.small was left to a prep kernel that does not take the statistics");
            qp.clear_small = ws.small.as<unsigned>();
        }
        query_prep_kernel<<<dim3(nblk), dim3(256), 0, st>>>(qp);
    }
    VDB_HIP(hipGetLastError());
}

// Per-search panels (streamed, int8-only and PQ indexes): the chunks are scanned slab by slab.  `fill(tile_a, ntiles, buf)` makes the
// fp16 panels of the slab's tiles [tile_a, tile_a + ntiles) in h->scan.slab (sized by the caller for `slab_chunks` chunks), then the
// scan runs on those chunks with `panels` rebased to the slab.  Layout: tiles per span, k-steps per tile.
template <class Fill>
void scan_in_slabs(const Batch &b, const ScanArgs &sa, int64_t Qpad, int nw_small, int64_t tiles_per_span, int64_t ksl,
                   int64_t slab_chunks, Fill &&fill) {
    vdb_index_s *h = b.h;
    const ScanGeom &g = b.g;
    half8 *buf = h->scan.slab.as<half8>();
    for (int64_t c0 = 0; c0 < g.nchunks; c0 += slab_chunks) {
        const int64_t c1 = std::min<int64_t>(g.nchunks, c0 + slab_chunks);
        const int64_t span_a = chunk_span0((int)c0, g.spc, g.rem), span_b = std::min<int64_t>(g.nspans, chunk_span0((int)c1, g.spc, g.rem));
        const int64_t tile_a = span_a * tiles_per_span, ntiles = (span_b - span_a) * tiles_per_span;
        if ((size_t)ntiles * ksl * 64 * sizeof(half8) > h->scan.slab.cap) throw Error(VDB_ERR_STATE, "internal: a slab of panels exceeds its buffer");
        fill(tile_a, ntiles, buf);
        ScanArgs ss = sa;
        ss.panels = buf - (size_t)tile_a * ksl * 64;
        ss.chunk0 = (int)c0;
        ss.nchunks = (int)(c1 - c0);
        launch(plan_f16(b.shape, h->opt, (int)(c1 - c0), Qpad, b.nq, b.direct_rows, nw_small), h, &ss, nullptr, b.st);   // (planned per slab: its own chunk count)
    }
}

// step 2: the fp16 scan -- resident panels in one launch, per-search panels slab by slab
void scan_fp16(const Batch &b, const ScanArgs &sa, int64_t Qpad, int nw_small) {
    vdb_index_s *h = b.h;
    const ScanGeom &g = b.g;
    hipStream_t st = b.st;
    const int Dm = h->dim, D4 = h->D4;
    if (h->panels_streamed) {
        // streamed panels (option "stream_panels"): chunks are scanned slab by slab -- convert the slab's float32 rows into a
        // scratch slab (p16 panels), then launch the scan on those chunks with `panels` rebased to the slab.  Same bins, same
        // results; one extra pass over the float32 rows per batch (0.65 ms per 786k x 768 rows, 5.5 TB/s).  Two slabs on two
        // streams (the next slab's workgroups filling the tail of the current one) measured 171.6 ms against 178.0 ms for
        // this single slab on a 12.5M x 768 shard, at 1.9 GB more: not kept.
        const int64_t KS = h->ksteps / 2;
        const int64_t chunk_rows = (int64_t)(g.spc + 1) * kSpanRows16;                  // (chunks are spc or spc + 1 spans)
        const int64_t slab_chunks = stream_slab_chunks(b.shape, h->opt, g, Qpad);      // (option "stream_slab_rows": whole rounds of workgroups per XCD)
        h->scan.slab.reserve((size_t)slab_chunks * chunk_rows / kTileRows16 * KS * 64 * sizeof(half8));
        scan_in_slabs(b, sa, Qpad, nw_small, kTilesPerSpan16, KS, slab_chunks, [&](int64_t tile_a, int64_t ntiles, half8 *buf) {
            convert_slab16_kernel<<<dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st>>>(
                h->rows.x32.as<float>(), h->N, Dm, D4, (int)KS, tile_a, ntiles, h->sx, buf);
        });
    } else if (h->int8_only) {
        // int8-only index: there is no resident fp16 copy.  Which scan serves the batch is decided on the device, so the fp16 scan
        // is enqueued all the same, slab by slab: convert_slab_from_i8_kernel turns the slab's int8 panels into fp16 panels (and
        // returns at once, like the scan behind it, when the batch is integer -- the usual case), scan_kernel runs on those chunks
        // with `panels` rebased.  The slab is small by default (option "int8_slab_chunks", 8 chunks = 16 MiB at D = 128): it is
        // resident whether or not a non-integer batch ever comes.
        const int64_t tiles_per_span = kTilesPerSpan;
        const int64_t slab_chunks = std::max<int64_t>(1, std::min<int64_t>(h->opt.int8_slab_chunks > 0 ? h->opt.int8_slab_chunks : 8, g.nchunks));
        const int64_t max_spans = (int64_t)(g.spc + 1) * slab_chunks;
        if (h->scan.slab.cap < (size_t)max_spans * tiles_per_span * h->ksteps * 64 * sizeof(half8))
            h->scan.slab.reserve_exact((size_t)max_spans * tiles_per_span * h->ksteps * 64 * sizeof(half8));
        scan_in_slabs(b, sa, Qpad, nw_small, tiles_per_span, h->ksteps, slab_chunks, [&](int64_t tile_a, int64_t ntiles, half8 *buf) {
            const int64_t threads = ntiles * h->ksteps * 64;
            convert_slab_from_i8_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(
                h->scan.panels8.as<int4v>(), h->i8_ks, h->ksteps, h->i8_cx, tile_a, ntiles, h->N, Dm, sa.info, buf, h->x16 ? 1 : 0);
        });
    } else if (pq_on(h)) {
        // PQ index: nothing but the codes is resident.  pq_panels_kernel turns the code rows of the slab's tiles into the fp16 panels
        // a flat index over x^ would hold (same rounding, so the same bias, scales and error bound serve), the scan runs on those
        // chunks with `panels` rebased.  Slab size: option "pq_slab_chunks", default the chunks of 524 288 rows (128 MiB at D = 128;
        // 64 chunks measured 11 % faster than 32 and as fast as one slab, profiles/r07_bench_pq.json); it does not grow with N (chunks are <= 8192 rows below 8M rows).
        const int64_t tiles_per_span = h->tile16 ? kTilesPerSpan16 : kTilesPerSpan;
        const int64_t ksl = h->tile16 ? h->ksteps / 2 : h->ksteps;
        const int64_t chunk_rows = (int64_t)(g.spc + 1) * (h->tile16 ? kSpanRows16 : kSpanRows);
        int64_t slab_chunks = h->opt.pq_slab_chunks > 0 ? h->opt.pq_slab_chunks : std::max<int64_t>(1, kPqSlabRows / chunk_rows);
        slab_chunks = std::max<int64_t>(1, std::min<int64_t>(slab_chunks, g.nchunks));
        // (default size: the slab is allocated for its full 524 288 rows whatever the corpus holds -- the workspace of a search does
        //  not depend on N; vdb_stats counts it in bytes_workspace)
        const int64_t max_spans = h->opt.pq_slab_chunks > 0 ? (int64_t)(g.spc + 1) * slab_chunks
                                                        : std::max<int64_t>(kPqSlabRows, chunk_rows) / (h->tile16 ? kSpanRows16 : kSpanRows);
        const size_t slab_bytes = (size_t)max_spans * tiles_per_span * ksl * 64 * sizeof(half8);
        if (h->scan.slab.cap < slab_bytes) h->scan.slab.reserve_exact(slab_bytes);
        scan_in_slabs(b, sa, Qpad, nw_small, tiles_per_span, ksl, slab_chunks,
                      [&](int64_t tile_a, int64_t ntiles, half8 *buf) { launch_pq_panels(h, tile_a, ntiles, buf, st); });
    } else
        launch(plan_f16(b.shape, h->opt, g.nchunks, Qpad, b.nq, b.direct_rows, nw_small), h, &sa, nullptr, st);   // (fp16: returns at once when the int8 scan serves the batch)
}

// step 3: the arguments of the int8 scan (byte-valued corpora)
ScanI8Args scan_i8_args(const Batch &b, const ScanArgs &sa, int64_t Qpad) {
    vdb_index_s *h = b.h;
    const ScanGeom &g = b.g;
    ScanI8Args s8{};
    s8.panels = h->scan.panels8.as<int4v>();
    s8.bias8 = b.bias8;
    s8.qpanels = b.ws.qpanels8.as<int4v>();
    s8.info = sa.info;
    s8.bin_m1 = sa.bin_m1; s8.bin_m2 = sa.bin_m2;
    s8.sb_m1 = sa.sb_m1; s8.sb_m2 = sa.sb_m2; s8.sb_span = sa.sb_span;
    s8.nspans = g.nspans; s8.Npad = h->Npad; s8.Qpad = Qpad; s8.nq_valid = b.nq;
    s8.prio = h->opt.scan_prio;
    s8.spans_per_chunk = g.spc; s8.chunk_rem = g.rem; s8.nchunks = g.nchunks;
    return s8;
}

// step 4: candidates per query from the bin minima
SelectArgs scan_select(const Batch &b, const ScanArgs &sa, int64_t Qpad, int cand_cap, int rescan_cap) {
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const ScanGeom &g = b.g;
    const int64_t nq = b.nq;
    const int k = b.k, G = h->tile16 ? 4 : 2;
    hipStream_t st = b.st;
    SelectArgs se{};
    se.bin_m1 = sa.bin_m1;
    se.bin_m2 = sa.bin_m2;
    se.sb_m1 = sa.sb_m1;
    se.sb_m2 = sa.sb_m2;
    se.sb_span = sa.sb_span;
    se.eps = ws.eps.as<float>();
    se.info = sa.info;
    se.nq = nq;
    se.Qpad = Qpad;
    se.nspans = g.nspans;
    se.N = h->N;
    se.spans_per_chunk = g.spc;
    se.chunk_rem = g.rem;
    se.nchunks = g.nchunks;
    se.k = k;
    se.groups = G;
    se.direct_rows = b.direct_rows;
    if (b.direct_rows) {        // the level-1 bins are the superbins
        se.sb_m1 = sa.bin_m1;
        se.sb_m2 = sa.bin_m2;
    }
    se.cand_cap = cand_cap;
    se.rescan_cap = rescan_cap;
    se.f16_gmode = f16_octs(b.shape, h->opt, b.direct_rows) ? 4 : 0;
    se.cand_rows = ws.cand.as<int32_t>();
    se.rescan_rows = ws.rescan.as<int32_t>();
    se.counts = ws.counts.as<int32_t>();
    se.fallback = ws.fallback.as<int32_t>();
    se.fb_list = ws.fb_list.as<int32_t>();
    se.fb_count = b.fb_count;
    se.stat_counters = b.stat_counters;
    const int nsb_i = G * g.nchunks;
    if (nsb_i > 128 && nsb_i <= 256 && h->opt.select_variant == 2 && !b.direct_rows) {   // 32 lanes per query, 2 queries per wave
        select_kernel_v2<8, 32><<<dim3((unsigned)((nq + 7) / 8)), dim3(256), 0, st>>>(se);
    } else if (nsb_i <= 256 && h->opt.select_variant != 1 && !b.direct_rows) {  // multi-lane form: 16 lanes per query, 4 queries per wave
        const unsigned sgrid = (unsigned)((nq + 15) / 16);
        if (nsb_i <= 64)
            select_kernel_v2<4, 16><<<dim3(sgrid), dim3(256), 0, st>>>(se);
        else if (nsb_i <= 128)
            select_kernel_v2<8, 16><<<dim3(sgrid), dim3(256), 0, st>>>(se);
        else
            select_kernel_v2<16, 16><<<dim3(sgrid), dim3(256), 0, st>>>(se);
    } else {
        switch (g.vpl) {
            case 1: launch_select<1>(se, st); break;
            case 2: launch_select<2>(se, st); break;
            case 4: launch_select<4>(se, st); break;
            case 8: launch_select<8>(se, st); break;
            case 16: launch_select<16>(se, st); break;
            default: launch_select<32>(se, st); break;
        }
    }
    VDB_HIP(hipGetLastError());
    return se;
}

// step 5: the refine tail -- exact re-score of every query's candidates ...
void scan_refine_tail(const Batch &b, const SelectArgs &se) {
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const int64_t nq = b.nq;
    const int k = b.k;
    hipStream_t st = b.st;
    RefineListArgs la{};
    la.c = b.rc;
    la.nq = nq;
    la.cand_rows = se.cand_rows;
    la.rescan_rows = se.rescan_rows;
    la.counts = se.counts;
    la.fallback = se.fallback;
    la.cand_cap = se.cand_cap;
    la.rescan_cap = se.rescan_cap;
    la.D = b.D;
    la.I = b.I;
    la.pkeys = b.pk;
    la.pids = b.pi;
    la.f16_shift = se.f16_gmode ? 3 : 2;
    // ... and the queries whose work list overflowed (or whose scales were unusable): exhaustive exact pass, split and merged
    // on the device, in the same launch (refine.hpp, refine_tail_kernel)
    {
        RefineFallbackArgs fa{};
        fa.c = b.rc;
        fa.fb_list = se.fb_list;
        fa.fb_count = b.fb_count;
        fa.max_split = (int)std::min<int64_t>(64, std::max<int64_t>(1, h->N / 4096));
        fa.cap_units = std::max<int64_t>(nq, 4096);
        ws.pkeys.reserve((size_t)fa.cap_units * k * sizeof(double));
        ws.pids.reserve((size_t)fa.cap_units * k * sizeof(int64_t));
        const size_t done_cap = ws.fb_done.cap;
        ws.fb_done.reserve((size_t)nq * sizeof(int32_t));
        if (ws.fb_done.cap != done_cap) VDB_HIP(hipMemsetAsync(ws.fb_done.p, 0, ws.fb_done.cap, st));   // (zero between searches)
        fa.pkeys = ws.pkeys.as<double>();
        fa.pids = ws.pids.as<int64_t>();
        fa.done = ws.fb_done.as<int32_t>();
        fa.D = b.D;
        fa.I = b.I;
        fa.okeys = b.pk;
        fa.oids = b.pi;
        const int kpl = kpl_for(k);
        DISPATCH_KPL(kpl, (refine_tail_kernel<KPL><<<dim3(256 + (unsigned)((nq + 3) / 4)), dim3(256), 0, st>>>(la, fa, 256u)));
        VDB_HIP(hipGetLastError());
    }
}

// PQ, option "pq_adc_max_batch": the lookup-table (ADC) scan of the codes makes the bin records (pq_adc.hpp); select and refine tail
// are those of search_scan.  The prep takes the batch statistics, the tables and the ADC error bounds -- no fp16 B fragments -- and
// no slab of panels is made or allocated.
void search_scan_adc(const Batch &b) {
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const ScanGeom &g = b.g;
    const int64_t nq = b.nq;
    const int k = b.k;
    hipStream_t st = b.st;
    const int64_t Qpad = (nq + 511) / 512 * 512;
    const int G = h->tile16 ? 4 : 2;
    const int64_t nbins = g.nspans * G, nsb = (int64_t)g.nchunks * G;
    const int cand_cap = h->opt.list_cap > 0 ? h->opt.list_cap : std::max(64, 2 * k + 32);
    const int rescan_cap = std::max(16, k / 2 + 8);
    ws.eps.reserve((size_t)nq * sizeof(float));
    ws.adc_tab.reserve((size_t)nq * h->pq.M * 256 * sizeof(float));
    ws.bin_m1.reserve((size_t)nbins * Qpad * sizeof(float));
    ws.bin_m2.reserve((size_t)nbins * Qpad * sizeof(float));
    ws.sb_m1.reserve((size_t)nsb * Qpad * sizeof(float));
    ws.sb_m2.reserve((size_t)nsb * Qpad * sizeof(float));
    ws.sb_span.reserve((size_t)nsb * Qpad * sizeof(int32_t));
    ws.cand.reserve((size_t)nq * cand_cap * sizeof(int32_t));
    ws.rescan.reserve((size_t)nq * rescan_cap * 2 * sizeof(int32_t));
    ws.counts.reserve((size_t)nq * 2 * sizeof(int32_t));
    ws.fallback.reserve((size_t)nq * sizeof(int32_t));
    ws.fb_list.reserve((size_t)nq * sizeof(int32_t));

    QueryBatchInfo *info = batch_info(ws);              // (zeroed by search_batch)
    const int64_t total = nq * h->dim;
    query_stats_kernel<<<dim3(query_stats_blocks(total)), dim3(256), 0, st>>>(
        b.dq, total, info, FinalizeArgs{h->sx, h->metric, h->corpus_int_unscaled ? 1 : 0, h->maxnorm2, 0});
    h->info_valid_nq = nq;
    launch_pq_adc_tables(h, b.dq, nq, info, ws.adc_tab.as<float>(), ws.eps.as<float>(), st);

    ScanArgs sa{};                                      // (what scan_select reads of it)
    sa.info = info;
    sa.bin_m1 = ws.bin_m1.as<float>();
    sa.bin_m2 = ws.bin_m2.as<float>();
    sa.sb_m1 = ws.sb_m1.as<float>();
    sa.sb_m2 = ws.sb_m2.as<float>();
    sa.sb_span = ws.sb_span.as<int32_t>();
    PqAdcScanArgs aa = pq_adc_args(h, ws.adc_tab.as<float>(), info);
    aa.bin_m1 = sa.bin_m1; aa.bin_m2 = sa.bin_m2;
    aa.sb_m1 = sa.sb_m1; aa.sb_m2 = sa.sb_m2; aa.sb_span = sa.sb_span;
    aa.nspans = g.nspans; aa.Qpad = Qpad;
    aa.spans_per_chunk = g.spc; aa.chunk_rem = g.rem; aa.nchunks = g.nchunks;
    timing_mark(h, b.tslot, 0, st);
    launch_pq_adc_scan(h, aa, nq, st);
    timing_mark(h, b.tslot, 1, st);
    const SelectArgs se = scan_select(b, sa, Qpad, cand_cap, rescan_cap);
    scan_refine_tail(b, se);
    timing_mark(h, b.tslot, 2, st);
    h->last.last_path = VDB_PATH_PQ_ADC;
}

// the steps in the order they are enqueued
void search_scan(const Batch &b) {
    if (b.adc) return search_scan_adc(b);
    vdb_index_s *h = b.h;
    Workspace &ws = b.ws;
    const ScanGeom &g = b.g;
    const int64_t nq = b.nq;
    const int k = b.k;
    hipStream_t st = b.st;
    const int64_t Qpad = (nq + 511) / 512 * 512;
    const int G = h->tile16 ? 4 : 2;
    const int64_t nbins = g.nspans * G * (b.direct_rows ? kBinRows / b.direct_rows : 1), nsb = (int64_t)g.nchunks * G;
    const int cand_cap = h->opt.list_cap > 0 ? h->opt.list_cap : std::max(64, 2 * k + 32);
    const int rescan_cap = std::max(16, k / 2 + 8);
    const bool i8 = use_i8(b.shape, h->opt, b.direct_rows);
    ws.qpanels.reserve((size_t)(Qpad / 32) * h->ksteps * 64 * sizeof(half8));
    ws.eps.reserve((size_t)nq * sizeof(float));
    ws.bin_m1.reserve((size_t)nbins * Qpad * sizeof(float));
    ws.bin_m2.reserve((size_t)nbins * Qpad * sizeof(float));
    ws.sb_m1.reserve((size_t)nsb * Qpad * sizeof(float));
    ws.sb_m2.reserve((size_t)nsb * Qpad * sizeof(float));
    ws.sb_span.reserve((size_t)nsb * Qpad * sizeof(int32_t));
    ws.cand.reserve((size_t)nq * cand_cap * sizeof(int32_t));
    ws.rescan.reserve((size_t)nq * rescan_cap * 2 * sizeof(int32_t));
    ws.counts.reserve((size_t)nq * 2 * sizeof(int32_t));
    ws.fallback.reserve((size_t)nq * sizeof(int32_t));
    ws.fb_list.reserve((size_t)nq * sizeof(int32_t));

    QueryBatchInfo *info = batch_info(ws);              // (zeroed with fb_count above)
    scan_query_prep(b, Qpad, i8, info);

    ScanArgs sa{};
    sa.panels = h->scan.panels.as<half8>();
    sa.bias = b.bias;
    sa.qpanels = ws.qpanels.as<half8>();
    sa.info = info;
    sa.bin_m1 = ws.bin_m1.as<float>();
    sa.bin_m2 = ws.bin_m2.as<float>();
    sa.sb_m1 = ws.sb_m1.as<float>();
    sa.sb_m2 = ws.sb_m2.as<float>();
    sa.sb_span = ws.sb_span.as<int32_t>();
    sa.nspans = g.nspans;
    sa.spans_per_chunk = g.spc;
    sa.chunk_rem = g.rem;
    sa.nchunks = g.nchunks;
    sa.Qpad = Qpad;
    sa.nq_valid = nq;
    sa.prio = h->opt.scan_prio;
    timing_mark(h, b.tslot, 0, st);
    // the scan the device did not choose for the batch returns at once; layout "x16" with both copies resident: both in ONE launch
    const int nw = nw_small(h->opt, nq);
    const ScanLaunch pair = plan_pair(b.shape, h->opt, g.nchunks, Qpad, nq, b.direct_rows, nw);
    if (pair.family != ScanFamily::none) {
        const ScanI8Args s8 = scan_i8_args(b, sa, Qpad);
        launch(pair, h, &sa, &s8, st);
    } else {
        scan_fp16(b, sa, Qpad, nw);
        if (i8) {
            const ScanI8Args s8 = scan_i8_args(b, sa, Qpad);
            launch(plan_i8(b.shape, h->opt, g.nchunks, Qpad, nq, nw), h, nullptr, &s8, st);
        }
    }
    timing_mark(h, b.tslot, 1, st);
    const SelectArgs se = scan_select(b, sa, Qpad, cand_cap, rescan_cap);
    scan_refine_tail(b, se);
    timing_mark(h, b.tslot, 2, st);
    h->last.last_path = VDB_PATH_MFMA_SCAN;
}

// what all paths share -- padded queries, where the rows live, geometry and path choice, the clearing of ws.small, timing_begin --
// then the path
// (filtered: a vdb_search_filtered call -- the same batch with the scans' accumulator inits pointing at the masked copies of the
//  handle's filter and the allow words in RefineCommon; what follows reasons about the rows that EXIST with the admitted count)
void search_batch(vdb_index_s *h, const float *dq, int64_t nq, int k, float *D, int64_t *I, double *pk, int64_t *pi,
                  hipStream_t st, bool filtered = false) {
    Workspace &ws = h->ws;
    const int Dm = h->dim, D4 = h->D4;
    // float32 queries padded to D4 for the refine kernels
    const float *qpad = dq;
    if (D4 != Dm) {
        ws.qpad.reserve((size_t)nq * D4 * sizeof(float));
        pad_rows_kernel<<<dim3((unsigned)((nq * D4 + 255) / 256)), dim3(256), 0, st>>>(dq, nq, Dm, D4, ws.qpad.as<float>());
        VDB_HIP(hipGetLastError());
        qpad = ws.qpad.as<float>();
    }
    RefineCommon rc = flat_rows(h, qpad, k);
    rc.info = batch_info(ws);                             // (group size of the candidates: 4 rows, 8 on the int8 scan)
    if (filtered) rc.allow = h->filter.words.as<uint32_t>();
    const int64_t n_live = filtered ? h->filter_count : h->N;
    const bool i8_off = h->opt.panel_dtype && !h->int8_only;   // (an int8-only index has nothing but the int8 copies)
    if (h->i8_ok && h->scan.rows8.p && !i8_off) {              // (int8 rows: batches the device puts on the int8 scan; int8-only: every batch)
        rc.X8 = h->scan.rows8.as<signed char>();
        rc.rowstat = h->scan.rowstat8.as<int>();
        rc.x8_pitch = h->rows8_pitch;
        rc.cx = h->i8_cx;
        rc.D = Dm;
        ws.qrows8.reserve((size_t)nq * h->rows8_pitch);
        rc.Q8 = ws.qrows8.as<signed char>();               // (filled next to the B fragments when the int8 scan is offered)
    }

    ScanGeom g;
    const ScanIndexShape shape = scan_shape_of(h);
    // (PQ: a batch below "pq_scan_min_batch" takes the exact kernels on the codes instead of decoding the corpus for it -- DESIGN 4.9)
    const bool pq_small = pq_on(h) && h->opt.force_path != 2 && nq < (h->opt.pq_scan_min_batch > 0 ? h->opt.pq_scan_min_batch : kPqScanMinBatch);
    const bool exact_only = h->opt.force_path == 1 || h->opt.force_path == 3 || pq_small;   // 3: also without query blocking (A/B runs)
    bool use_scan = h->scan_ok && !exact_only && k <= 1024;
    int direct_rows = 0;
    if (use_scan) {
        g = scan_geometry(shape, h->opt, k, nq);
        if (!g.ok) direct_rows = scan_geometry_direct(shape, h->opt, k, g);
    }
    // (measured on 1M x 128 with host I/O: the MFMA pipeline answers 1..512 queries in 0.13..0.18 ms, the exhaustive float64
    //  kernel needs 0.3 ms for one query -- scripts/latency_small_batches.py -- so the batch size does not gate the path)
    // Between the dense small-corpus path (<= 8192 rows) and 32768 rows the scan pays off once the batch carries
    // enough (query, row) pairs: ~0.3 ms of fixed pipeline cost against ~7e-8 ms per pair in the exhaustive kernel.
    use_scan = use_scan && g.ok &&
               (h->opt.force_path == 2 || h->N >= 32768 || (h->Npad > 8192 && (double)nq * (double)h->N >= 4.0e6));
    // (corpora of 8193..15360 rows whose chunking cannot give 4k superbins still have the dense path below)

    // (PQ, option "pq_adc_max_batch": batches up to that size on the standard 256-row-bin geometry take the lookup-table scan of the
    //  codes -- pq_adc.hpp -- unless the table of M sub-spaces does not fit a workgroup's LDS)
    const bool use_adc = pq_on(h) && use_scan && direct_rows == 0 && nq <= h->opt.pq_adc_max_batch && pq_adc_fits(h->pq.M);

    h->info_valid_nq = -1;
    // fb_count restarts with every batch (it indexes this batch's fb_list); the statistics counters behind it were
    // zeroed once for the whole call (search_device_impl) and accumulate over the batches
    // (serving-shaped calls on the MFMA scan path: no memset at all -- workgroup 0 of query_prep_kernel, which takes the batch
    //  statistics itself, clears ws.small around the QueryBatchInfo it writes; one ~4.5 us dispatch less per search)
    bool clear_in_prep = false;
    if (h->small_clear_pending) {
        h->small_clear_pending = false;
        h->small_is_clean = false;
        clear_in_prep = use_scan && !use_adc && nq * Dm <= kFusedStatsMax && !h->tile16 && h->opt.fused_stats;
        if (!clear_in_prep) VDB_HIP(hipMemsetAsync(ws.small.p, 0, kSmallBytes, st));
    } else if (h->small_is_clean) h->small_is_clean = false;      // the first batch of a call: search_device_impl has just cleared all of it
    else VDB_HIP(hipMemsetAsync(ws.small.p, 0, 64, st));
    int32_t *fb_count = ws.small.as<int32_t>();
    unsigned long long *stat_counters = reinterpret_cast<unsigned long long *>(ws.small.as<char>() + 64);

    const long tslot = timing_begin(h, st);

    // small corpora: the dense path (search_dense)
    const bool use_dense = !use_scan && h->scan_ok && !exact_only && h->scan.panels.p != nullptr && (h->ksteps <= kMaxKSteps || h->ksteps % 4 == 0) &&
                           h->Npad <= kDenseMaxRows && nq >= 64 && k <= 1024 && (int64_t)k * 2 <= n_live &&
                           !h->tile16 && (h->Npad + std::max(128, 2 * k + 64)) * 4 <= 65536;   // scores + candidates in LDS
    const Batch b{h, ws, dq, nq, k, D, I, pk, pi, st, rc, g, shape, direct_rows, fb_count, stat_counters, tslot, clear_in_prep, use_adc,
                  filtered ? h->filter.bias_f.as<float>() : h->scan.bias.as<float>(),
                  filtered ? h->filter.bias8_f.as<int32_t>() : h->scan.bias8.as<int32_t>()};
    if (use_dense) search_dense(b);
    else if (!use_scan) search_exact(b);
    else search_scan(b);
}

// ---- hipGraph replay of a repeated device-resident search -----------------------------------------------------------
// A small batch is a chain of ~9 (flat) / ~18 (IVF) short dependent dispatches.  With option "graph" = 1 the first call
// of a (buffers, shape, stream) combination runs eagerly (it sizes the workspace: allocation is illegal while capturing),
// the second is captured into a graph and launched, later ones replay the graph.  Anything that changes the index or an
// option drops the graph (graph_reset).
// An executable graph may still be running on the caller's stream when it is dropped (a serving loop that alternates two
// shapes never synchronises in between): every launch is followed by an event, and the exec is destroyed only once that
// event has completed.
void graph_drop_exec(vdb_index_s *h) {
    if (!h->graph_exec) return;
    if (h->graph_ev) (void)hipEventSynchronize(h->graph_ev);
    alloc_note("GRAPH_DESTROY", h->graph_exec, 0);
    (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
}
void graph_launch(vdb_index_s *h, hipStream_t st) {
    alloc_note("GRAPH_LAUNCH", h->graph_exec, (size_t)h->graph_replays);
    VDB_HIP(hipGraphLaunch(h->graph_exec, st));
    if (!h->graph_ev) VDB_HIP(hipEventCreateWithFlags(&h->graph_ev, hipEventDisableTiming));
    VDB_HIP(hipEventRecord(h->graph_ev, st));
    ++h->graph_replays;
}

void graph_reset(vdb_index_s *h) {
    graph_drop_exec(h);
    h->graph_key = vdb_index_s::GraphKey{};
    h->graph_warm = vdb_index_s::GraphKey{};
}

constexpr int64_t kGraphMaxQueries = 4096;

template <class F>
void graph_or_run(vdb_index_s *h, const vdb_index_s::GraphKey &key, F &&run) {
    const bool eligible = h->opt.graph && key.st != nullptr && !h->opt.timing && key.nq > 0 && key.nq <= kGraphMaxQueries;
    if (!eligible) {
        run();
        return;
    }
    if (h->graph_exec && key == h->graph_key && h->graph_epoch == g_alloc_epoch.load(std::memory_order_relaxed)) {
        graph_launch(h, key.st);
        return;
    }
    if (h->graph_exec) {      // another shape, or a buffer moved since the capture (the graph holds raw addresses): drop it
        // ... and let THIS call run eagerly as the new warm-up, whatever the key.  Rule: never hipGraphInstantiate in the call that
        // destroyed an executable graph.  Cause (profiles/r04_graph_fault_cause.txt, found with $VDBHIP_ALLOC_LOG): with the
        // runtime's graph packet capture on (ROCm 7.x default), a successor instantiated right behind the destroy -- no other
        // submission in between -- runs a kernel with a wild pointer on its SECOND replay: the fault address belongs to no
        // allocation this library or the caller ever made (live or freed), every buffer the graph bakes in was live at every
        // launch, and the same build and sequence with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 replays correctly.  Not a stale pointer
        // of ours; the eager call in between is what the runtime needs.
        const bool same_key = key == h->graph_key;
        graph_drop_exec(h);
        h->graph_key = vdb_index_s::GraphKey{};
        h->graph_warm = vdb_index_s::GraphKey{};
        if (h->opt.graph_recapture_at_once && same_key) h->graph_warm = key;     // (diagnostic: the old ordering)
    }
    if (!(key == h->graph_warm)) {
        run();
        h->graph_warm = key;
        return;
    }
    const vdb_index_s::GraphKey warm = h->graph_warm;
    graph_reset(h);
    VDB_HIP(hipStreamBeginCapture(key.st, hipStreamCaptureModeThreadLocal));
    hipGraph_t g = nullptr;
    bool captured = true;
    try {
        run();
    } catch (...) {
        captured = false;
    }
    const hipError_t e_end = hipStreamEndCapture(key.st, &g);
    hipGraphExec_t ex = nullptr;
    if (captured && e_end == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
        if (alloc_log()) {        // what the graph bakes in: the caller's buffers and every buffer of the handle (by name)
            alloc_note("GRAPH_INSTANTIATE", ex, 0);
            alloc_note("  arg.q", key.q, 0); alloc_note("  arg.o1", key.o1, 0); alloc_note("  arg.o2", key.o2, 0);
            const auto dump = [](vdb_index_s *x, const char *owner) {
                for_each_group(x, [&](auto &g) {
                    for_each_buf(g, [&](const char *name, DevBuf &b) { alloc_note((std::string("  ") + owner + name).c_str(), b.p, b.cap); });
                });
            };
            dump(h, "");
            if (h->coarse) dump(h->coarse, "coarse.");
        }
        (void)hipGraphDestroy(g);
        h->graph_exec = ex;
        h->graph_key = key;
        h->graph_warm = warm;
        h->graph_epoch = g_alloc_epoch.load(std::memory_order_relaxed);
        graph_launch(h, key.st);
        return;
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    run();          // the capture did not work out (e.g. a workspace had to grow): this call runs eagerly, the next one warms up again
}

void search_device_impl(vdb_index_s *h, const float *dq, int64_t nq, int k, float *D, int64_t *I, double *pk,
                        int64_t *pi, hipStream_t st, bool filtered = false) {
    if (!h->built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (nq < 0) throw Error(VDB_ERR_INVALID, "negative query count");
    h->last.last_nq = nq;
    if (nq == 0) return;
    if (!dq) throw Error(VDB_ERR_INVALID, "null query pointer");
    if (h->N == 0) {  // empty shard: all padding
        MergeArgs ma{};
        ma.nparts = 0;
        ma.k = k;
        ma.metric = h->metric;
        ma.count = nq;
        ma.D = D;
        ma.I = I;
        ma.okeys = pk;
        ma.oids = pi;
        launch_merge(ma, nq, st);
        h->last.last_path = VDB_PATH_EXACT_SCAN;
        return;
    }
    // queries per pass: the level-1 bin arrays cost 8 bytes per (256-row bin, query); keep them within kBinBudget so
    // that a large batch on a large shard is served in several passes instead of failing with VDB_ERR_NOMEM
    int64_t kBatch = 16384;
    {
        const int64_t nbins = std::max<int64_t>(1, h->Npad / kBinRows);
        const int64_t fit = (int64_t)(kBinBudget / (8.0 * (double)nbins)) / 512 * 512;
        kBatch = std::max<int64_t>(512, std::min<int64_t>(kBatch, fit));
    }
    h->ws.small.reserve(kSmallBytes);
    h->small_clear_pending = false;
    if (h->small_preset) h->small_preset = false;        // (an IVF parent cleared it together with its own buffers)
    else if (nq <= kBatch && nq * h->dim <= kFusedStatsMax && h->opt.fused_stats && !h->tile16)
        h->small_clear_pending = true;                   // serving-shaped call: the first batch's prep kernel clears it (search_batch), or a memset there
    else VDB_HIP(hipMemsetAsync(h->ws.small.p, 0, kSmallBytes, st));
    h->small_is_clean = true;
    const size_t ev_mark = h->ev_used;
    try {
        for (int64_t b0 = 0; b0 < nq; b0 += kBatch) {
            const int64_t nb = std::min<int64_t>(kBatch, nq - b0);
            search_batch(h, dq + (size_t)b0 * h->dim, nb, k, D ? D + (size_t)b0 * k : nullptr,
                         I ? I + (size_t)b0 * k : nullptr, pk ? pk + (size_t)b0 * k : nullptr,
                         pi ? pi + (size_t)b0 * k : nullptr, st, filtered);
        }
    } catch (...) {
        h->ev_used = ev_mark;      // events of a failed search were never all recorded: do not leave them to vdb_stats
        h->small_is_clean = false;
        throw;
    }
    h->small_is_clean = false;
}

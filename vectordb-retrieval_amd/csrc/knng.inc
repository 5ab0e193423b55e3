// knng.inc -- host side of the k-NN graph index (kernels: knng.hpp): exact graph build through the partial self-search, the
// injected graph, the beam search.  Included by vdbhip.hip; the handle's state is knng_degree + codes.knng_nbrs.

namespace {

constexpr int64_t kKnngBuildBlock = 65536;       // rows per self-search block (option "knng_build_block")
constexpr int kKnngDefaultEntries = 32;
constexpr size_t kKnngWaveLdsTarget = 20 << 10;  // 8 waves per CU out of 160 KiB of LDS
constexpr size_t kKnngGroupLds = 64 << 10;       // dynamic LDS of one workgroup

void knng_drop(vdb_index_s *h) {
    h->codes.knng_nbrs.release();
    h->knng_degree = 0;
}

// What the k-NN graph entry points admit: a flat handle, for the graph is searched against the resident float32 rows of ONE
// device, in insertion order (and none of the options that drop them: refuse_options_set).
constexpr unsigned kKnngCalls = kFlat | kKnng;

void knng_require_rows(const vdb_index_s *h) {
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (h->N >= 2147483647ll - 1024) throw Error(VDB_ERR_UNSUPPORTED, "the k-NN graph holds int32 row numbers: ntotal must be below 2^31");
}

void knng_build_impl(vdb_index_s *h, int degree, int ncand) {
    hipStream_t st = nullptr;
    const int64_t N = h->N;
    const int k = (int)std::min<int64_t>((int64_t)ncand + 1, N);
    const int64_t block = std::min<int64_t>(N, h->opt.knng_build_block > 0 ? h->opt.knng_build_block : kKnngBuildBlock);
    VDB_HIP(hipDeviceSynchronize());
    graph_reset(h);
    knng_drop(h);
    DevBuf pk, pi, cand, ckeys, qtmp;
    pk.reserve((size_t)block * k * sizeof(double));
    pi.reserve((size_t)block * k * sizeof(int64_t));
    cand.reserve((size_t)block * ncand * sizeof(int32_t));
    ckeys.reserve((size_t)block * ncand * sizeof(unsigned long long));
    if (h->D4 != h->dim) qtmp.reserve((size_t)block * h->dim * sizeof(float));
    h->codes.knng_nbrs.reserve_exact((size_t)N * degree * sizeof(int32_t));
    try {
        for (int64_t r0 = 0; r0 < N; r0 += block) {
            const int64_t nb = std::min<int64_t>(block, N - r0);
            const float *q = h->rows.x32.as<float>() + (size_t)r0 * h->D4;
            if (h->D4 != h->dim) {       // the search takes queries `dim` floats apart
                VDB_HIP(hipMemcpy2DAsync(qtmp.p, (size_t)h->dim * 4, q, (size_t)h->D4 * 4, (size_t)h->dim * 4, (size_t)nb, hipMemcpyDeviceToDevice, st));
                q = qtmp.as<float>();
            }
            search_device_impl(h, q, nb, k, nullptr, nullptr, pk.as<double>(), pi.as<int64_t>(), st);
            KnngStripArgs sa{pk.as<double>(), pi.as<int64_t>(), r0, nb, k, ncand, h->id_base, cand.as<int32_t>(), ckeys.as<unsigned long long>()};
            knng_strip_self_kernel<<<dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st>>>(sa);
            VDB_HIP(hipGetLastError());
            KnngPruneArgs pa{h->rows.x32.as<float>(), h->D4, h->metric, r0, nb, ncand, degree, cand.as<int32_t>(), ckeys.as<unsigned long long>(),
                             h->codes.knng_nbrs.as<int32_t>()};
            knng_prune_kernel<<<dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st>>>(pa);
            VDB_HIP(hipGetLastError());
        }
        VDB_HIP(hipStreamSynchronize(st));
    } catch (...) {
        knng_drop(h);
        throw;
    }
    h->knng_degree = degree;
}

// nbrs (N, degree): local row numbers, -1 only as a row's tail, no self loop, no duplicate within a row
void knng_validate(const int32_t *nbrs, int64_t N, int degree) {
    std::vector<int64_t> stamp((size_t)N, -1);
    for (int64_t r = 0; r < N; ++r) {
        bool tail = false;
        for (int j = 0; j < degree; ++j) {
            const int32_t v = nbrs[(size_t)r * degree + j];
            const std::string at = " (row " + std::to_string(r) + ", slot " + std::to_string(j) + ")";
            if (v == -1) {
                tail = true;
                continue;
            }
            if (tail) throw Error(VDB_ERR_INVALID, "k-NN graph: an entry follows a -1" + at);
            if (v < 0 || v >= N) throw Error(VDB_ERR_INVALID, "k-NN graph: neighbour " + std::to_string(v) + " is out of range" + at);
            if (v == r) throw Error(VDB_ERR_INVALID, "k-NN graph: self loop" + at);
            if (stamp[(size_t)v] == r) throw Error(VDB_ERR_INVALID, "k-NN graph: duplicate neighbour " + std::to_string(v) + at);
            stamp[(size_t)v] = r;
        }
    }
}

void knng_require_ready(vdb_index_s *h, const char *what) {
    refuse_options_set(h, what, kKnng);
    if (h->opt.graph) throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + ": the k-NN graph search is not available with option 'graph'");
    if (!h->built || h->N == 0) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (!knng_on(h)) throw Error(VDB_ERR_STATE, std::string(what) + ": no k-NN graph (call vdb_knng_build or vdb_knng_set; an add or a reset drops it)");
}

void knng_check_args(const void *q, int64_t nq, int k, int ef, const void *o1, const void *o2) {
    if (k < 1) throw Error(VDB_ERR_INVALID, "k must be at least 1");
    if (k > ef) throw Error(VDB_ERR_INVALID, "k must not exceed ef");
    if (ef > kKnngMaxEf) throw Error(VDB_ERR_INVALID, "ef must be at most 512");
    if (nq < 0) throw Error(VDB_ERR_INVALID, "negative query count");
    if (nq > 0 && (!q || !o1 || !o2)) throw Error(VDB_ERR_INVALID, "null pointer");
}

template <int EPL>
void launch_knng_search(const KnngSearchArgs &a, size_t lds, hipStream_t st) {
    knng_search_kernel<EPL><<<dim3((unsigned)((a.nq + a.waves - 1) / a.waves)), dim3((unsigned)a.waves * 64), lds, st>>>(a);
    VDB_HIP(hipGetLastError());
}

void knng_search_impl(vdb_index_s *h, const float *dq, int64_t nq, int k, int ef, float *D, int64_t *I, hipStream_t st) {
    const int efp = ef <= 64 ? 64 : ef <= 128 ? 128 : ef <= 256 ? 256 : 512;
    // the seen filter: as asked, else the largest (up to 4096 slots) that keeps a query within the LDS of 8 waves per CU; whatever
    // was asked, a workgroup's 64 KiB bound it (the filter is a cache: its size never changes a result)
    int vbits = h->opt.knng_visited_bits;
    if (vbits == 0) {
        vbits = 12;
        while (vbits > 8 && knng_wave_lds(efp, h->D4, vbits) > kKnngWaveLdsTarget) --vbits;
    }
    while (vbits > 1 && knng_wave_lds(efp, h->D4, vbits) > kKnngGroupLds) --vbits;
    const size_t per_wave = knng_wave_lds(efp, h->D4, vbits);
    if (per_wave > kKnngGroupLds) throw Error(VDB_ERR_UNSUPPORTED, "the k-NN graph search keeps the query in LDS: the dimension is too large");
    const float *qpad = dq;
    if (h->D4 != h->dim) {
        h->ws.qpad.reserve((size_t)nq * h->D4 * sizeof(float));
        pad_rows_kernel<<<dim3((unsigned)((nq * h->D4 + 255) / 256)), dim3(256), 0, st>>>(dq, nq, h->dim, h->D4, h->ws.qpad.as<float>());
        VDB_HIP(hipGetLastError());
        qpad = h->ws.qpad.as<float>();
    }
    h->knng_ws.knng_stat.reserve((size_t)kStatShards * kStatStride * sizeof(unsigned long long));
    VDB_HIP(hipMemsetAsync(h->knng_ws.knng_stat.p, 0, (size_t)kStatShards * kStatStride * sizeof(unsigned long long), st));
    h->last.last_nq = nq;
    h->last.last_path = VDB_PATH_KNNG;
    KnngSearchArgs a{};
    a.c = flat_rows(h, qpad, k);
    a.nbrs = h->codes.knng_nbrs.as<int32_t>();
    a.degree = h->knng_degree;
    a.nq = nq;
    a.k = k;
    a.ef = ef;
    {   // the entry rows of this call; uploaded again only when (N, nentry, ef) gave a different list
        const int64_t nentry = h->opt.knng_nentry > 0 ? h->opt.knng_nentry : kKnngDefaultEntries;
        const int64_t ne = std::min<int64_t>(std::min<int64_t>(nentry, ef), h->N);
        std::vector<int32_t> rows;
        for (int64_t j = 0; j < ne; ++j) {
            const int32_t row = (int32_t)(j * h->N / nentry);
            if (rows.empty() || rows.back() != row) rows.push_back(row);
        }
        if (rows != h->knng_entries || !h->knng_ws.knng_entry.p) {
            VDB_HIP(hipStreamSynchronize(st));           // (a search in flight may still read the old list)
            h->knng_ws.knng_entry.reserve((size_t)kKnngMaxEf * sizeof(int32_t));
            VDB_HIP(hipMemcpy(h->knng_ws.knng_entry.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            h->knng_entries = std::move(rows);
        }
        a.entries = h->knng_ws.knng_entry.as<int32_t>();
        a.nentries = (int)h->knng_entries.size();
    }
    a.max_iters = h->opt.knng_max_iters > 0 ? h->opt.knng_max_iters : 8 * ef;
    a.vbits = vbits;
    a.waves = (int)std::min<size_t>(4, kKnngGroupLds / per_wave);
    a.stat = h->knng_ws.knng_stat.as<unsigned long long>();
    a.D = D;
    a.I = I;
    const size_t lds = per_wave * a.waves;
    auto launch = [&](int phases) {
        a.phases = phases;
        switch (efp) {
            case 64: launch_knng_search<1>(a, lds, st); break;
            case 128: launch_knng_search<2>(a, lds, st); break;
            case 256: launch_knng_search<4>(a, lds, st); break;
            default: launch_knng_search<8>(a, lds, st); break;
        }
    };
    const long tslot = timing_begin(h, st);
    if (tslot < 0) {
        launch(7);
        return;
    }
    // a timed call runs the three stages as three launches; L travels between them through memory, the filter starts empty in
    // each (it is a cache: same results)
    h->knng_ws.knng_state_k.reserve((size_t)nq * efp * sizeof(unsigned long long));
    h->knng_ws.knng_state_i.reserve((size_t)nq * efp * sizeof(unsigned));
    a.st_keys = h->knng_ws.knng_state_k.as<unsigned long long>();
    a.st_ids = h->knng_ws.knng_state_i.as<unsigned>();
    launch(1);
    timing_mark(h, tslot, 0, st);
    launch(2);
    timing_mark(h, tslot, 1, st);
    launch(4);
    timing_mark(h, tslot, 2, st);
}

}  // namespace

extern "C" {

int vdb_knng_build(vdb_handle hh, int degree, int ncand) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_knng_build (the k-NN graph)", kKnngCalls);
        refuse_options_set(h, "vdb_knng_build", kKnng);
        if (degree < kKnngMinDegree || degree > kKnngMaxDegree) throw Error(VDB_ERR_INVALID, "k-NN graph: degree must be in [4, 64]");
        if (ncand < degree || ncand > kKnngMaxCand) throw Error(VDB_ERR_INVALID, "k-NN graph: ncand must be in [degree, 128]");
        knng_require_rows(h);
        set_device(h->device);
        knng_build_impl(h, degree, ncand);
    });
}

int vdb_knng_set(vdb_handle hh, int degree, const int32_t *nbrs_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_knng_set (the k-NN graph)", kKnngCalls);
        refuse_options_set(h, "vdb_knng_set", kKnng);
        if (degree < 1 || degree > kKnngMaxDegree) throw Error(VDB_ERR_INVALID, "k-NN graph: degree must be in [1, 64]");
        if (!nbrs_host) throw Error(VDB_ERR_INVALID, "null pointer");
        knng_require_rows(h);
        knng_validate(nbrs_host, h->N, degree);
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        graph_reset(h);
        knng_drop(h);
        h->codes.knng_nbrs.reserve_exact((size_t)h->N * degree * sizeof(int32_t));
        VDB_HIP(hipMemcpy(h->codes.knng_nbrs.p, nbrs_host, (size_t)h->N * degree * sizeof(int32_t), hipMemcpyHostToDevice));
        h->knng_degree = degree;
    });
}

int vdb_knng_get(vdb_handle hh, int *degree, int32_t *nbrs_host) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_knng_get", kAnyKind);
        if (!degree) throw Error(VDB_ERR_INVALID, "null pointer");
        *degree = h->knng_degree;                  // (0 on every other kind)
        if (nbrs_host && *degree > 0) {
            set_device(h->device);
            VDB_HIP(hipMemcpy(nbrs_host, h->codes.knng_nbrs.p, (size_t)h->N * h->knng_degree * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
    });
}

int vdb_knng_search_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, int ef, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_knng_search_device (the k-NN graph)", kKnngCalls);
        knng_require_ready(h, "vdb_knng_search_device");
        knng_check_args(q_dev, nq, k, ef, D_dev, I_dev);
        if (nq == 0) return;
        set_device(h->device);
        knng_search_impl(h, q_dev, nq, k, ef, D_dev, I_dev, as_stream(stream));
    });
}

int vdb_knng_search(vdb_handle hh, const float *q_host, int64_t nq, int k, int ef, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_knng_search (the k-NN graph)", kKnngCalls);
        knng_require_ready(h, "vdb_knng_search");
        knng_check_args(q_host, nq, k, ef, D, I);
        if (nq == 0) return;
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            knng_search_impl(h, dq, nq, k, ef, dD, dI, st);
        });
    });
}

}  // extern "C"

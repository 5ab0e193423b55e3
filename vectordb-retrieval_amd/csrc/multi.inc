// multi.inc -- ONE index handle over several GPUs of the node, driven from ONE process (included at the end of vdbhip.hip).
//
// SURVEY 8b proposed `vdb_create(dim, metric, const int *devs, int ndev, ...)` with `vdb_add` row-sharding across `devs`, and
// the reference's harness is a single process that calls build_index once and batch_search per batch
// (src/experiments/experiment_runner.py:329-331, 428-434) on a plugin it made from a `type:` string
// (src/benchmark/runner.py:177-181, src/algorithms/__init__.py:37-47).  `vdb_create_multi` is that form: the returned handle
// is an ordinary vdb_handle, every entry point of include/vdbhip.h that makes sense on it dispatches here.
//
//   shard s = a complete single-device index (a child vdb_index_s) on devs[s] with its own stream and its own host thread:
//   the ~7 dependent dispatches of a search are enqueued on all devices at once instead of one device after the other.
//   vdb_add:     rows of one call are cut into ndev contiguous blocks (block s -> shard s, SURVEY 8e); children number their
//                rows locally (id base 0) and a segment table (local row range -> global id range, one entry per add and
//                shard) turns local ids into global ones INSIDE the merge kernel -- appends keep working, ids stay
//                "id_base + insertion order" as on a single-device index.
//   vdb_search:  queries -> every device (H2D by each shard's thread, or peer copies from the primary device), per-shard
//                partial top-k (float64 keys + local ids, the same vdb_search_partial_device machinery the multi-process path
//                uses), gathered INTO THE PRIMARY DEVICE's buffer by one peer copy per shard (each over its own xGMI link,
//                1.6 MB at 10 000 queries x k = 10: latency bound), merged there by merge_kernel on (key, global id).
//                In one process an all-gather would deliver every partial to every device for nothing -- only the primary
//                merges -- so the collective is a gather of peer copies; RCCL stays the transport of the one-process-per-GPU
//                form (vdbhip/sharded.py), where every rank wants the result.
//   A device may appear more than once in devs (several shards on one GPU): that is how the single-GPU test box exercises this
//   file (tests/test_gpu_multi.py, devs = [0, 0, 0]).
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>

namespace {

// One persistent host thread per shard.  run_all(f) runs f(s) on thread s for every shard, waits for all of them and
// rethrows the first failure on the calling thread (vdb_last_error is thread-local: a worker's message must travel).
struct MultiPool {
    struct Worker {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<void()> job;
        bool has_job = false, stop = false;
    };
    std::vector<std::unique_ptr<Worker>> workers;
    std::mutex done_mu;
    std::condition_variable done_cv;
    int pending = 0;
    std::vector<int> err_code;
    std::vector<std::string> err_msg;

    void start(int n) {
        err_code.assign((size_t)n, 0);
        err_msg.assign((size_t)n, std::string());
        for (int i = 0; i < n; ++i) {
            workers.emplace_back(new Worker());
            Worker *w = workers.back().get();
            w->th = std::thread([this, w] {
                for (;;) {
                    std::function<void()> job;
                    {
                        std::unique_lock<std::mutex> lk(w->mu);
                        w->cv.wait(lk, [w] { return w->has_job || w->stop; });
                        if (w->stop && !w->has_job) return;
                        job.swap(w->job);
                        w->has_job = false;
                    }
                    job();
                    {
                        std::lock_guard<std::mutex> lk(done_mu);
                        --pending;
                    }
                    done_cv.notify_all();
                }
            });
        }
    }
    void run_all(const std::function<void(int)> &f) {
        const int n = (int)workers.size();
        {
            std::lock_guard<std::mutex> lk(done_mu);
            pending = n;
        }
        for (int i = 0; i < n; ++i) {
            err_code[(size_t)i] = 0;
            Worker *w = workers[(size_t)i].get();
            {
                std::lock_guard<std::mutex> lk(w->mu);
                w->job = [this, i, &f] {
                    try {
                        f(i);
                    } catch (const Error &e) {
                        err_code[(size_t)i] = e.code;
                        err_msg[(size_t)i] = e.what();
                    } catch (const std::exception &e) {
                        err_code[(size_t)i] = VDB_ERR_INVALID;
                        err_msg[(size_t)i] = e.what();
                    } catch (...) {
                        err_code[(size_t)i] = VDB_ERR_INVALID;
                        err_msg[(size_t)i] = "unknown error";
                    }
                };
                w->has_job = true;
            }
            w->cv.notify_one();
        }
        {
            std::unique_lock<std::mutex> lk(done_mu);
            done_cv.wait(lk, [this] { return pending == 0; });
        }
        for (int i = 0; i < n; ++i)
            if (err_code[(size_t)i]) throw Error(err_code[(size_t)i], "shard " + std::to_string(i) + ": " + err_msg[(size_t)i]);
    }
    void stop() {
        for (auto &w : workers) {
            {
                std::lock_guard<std::mutex> lk(w->mu);
                w->stop = true;
            }
            w->cv.notify_one();
        }
        for (auto &w : workers)
            if (w->th.joinable()) w->th.join();
        workers.clear();
    }
};

}  // namespace

struct vdb_multi_s {
    std::vector<vdb_index_s *> shards;   // shard s lives on shards[s]->device
    std::vector<hipStream_t> streams;    // the stream shard s works on (created on its device, non-blocking)
    std::vector<hipEvent_t> done;        // recorded on streams[s] behind shard s's part of a search
    hipEvent_t q_ready = nullptr;        // primary device: the caller's stream has produced the queries (device API)
    hipStream_t main_stream = nullptr;   // primary device: merge + D2H of the host API
    std::vector<DevBuf> q_stage, pack;   // per shard, on its device: the query batch; its packed partial (2, nq, k)
    std::vector<DevBuf> cand_stage, seg_shard;   // per shard: candidate ids of a rerank; its (id0, local0, n) triples
    std::vector<int> nseg_shard;
    DevBuf gather, seg_dev, out_d, out_i;   // primary device: gathered partials (S, 2, nq, k), segment table, host-API staging
    // one entry per (add call, shard with rows): rows [local0, local0 + n) of shard `shard` are rows [global0, global0 + n)
    // of the index (insertion order); kept in global order
    struct Seg { int shard; int64_t local0, n, global0; };
    std::vector<Seg> segs;
    bool seg_dirty = true;
    int mode = 0;                        // 0 empty | 1 rows added by vdb_add | 2 rows filed by vdb_ivf_add
    bool stage_all = false;              // option "multi_stage_all" (tests): shards on the primary device take the remote-shard path
                                         // too -- own query copy, own packed buffer, peer copy into the gather slot -- so that the
                                         // code a multi-GPU node runs is exercised on a one-GPU box
    MultiPool pool;
};

namespace {

constexpr int kMaxMultiShards = 64;

inline int multi_nshards(const vdb_index_s *m) { return (int)m->multi->shards.size(); }

// rows of one add: contiguous block s of ceil(n / S) rows (SURVEY 8e; the last blocks may be short or empty)
inline void multi_block(int64_t n, int S, int s, int64_t &lo, int64_t &hi) {
    const int64_t per = (n + S - 1) / S;
    lo = std::min<int64_t>(n, (int64_t)s * per);
    hi = std::min<int64_t>(n, lo + per);
}

vdb_index_s *multi_first_shard(vdb_index_s *m) { return m->multi->shards[0]; }
void multi_for_each_shard(vdb_index_s *m, const std::function<void(vdb_index_s *)> &f) {
    for (auto *c : m->multi->shards) f(c);
}

void multi_upload_segments(vdb_index_s *m) {
    vdb_multi_s *M = m->multi;
    if (!M->seg_dirty) return;
    const int S = multi_nshards(m);
    // [S + 1 offsets | (local0, id0) pairs grouped by shard, ascending local0]
    std::vector<int64_t> tab((size_t)S + 1, 0);
    for (const auto &sg : M->segs) ++tab[(size_t)sg.shard + 1];
    for (int s = 0; s < S; ++s) tab[(size_t)s + 1] += tab[(size_t)s];
    std::vector<int64_t> cursor(tab.begin(), tab.end() - 1);
    const size_t npairs = M->segs.size();
    tab.resize((size_t)S + 1 + 2 * std::max<size_t>(npairs, 1), 0);
    for (const auto &sg : M->segs) {            // (global order = ascending local0 inside every shard)
        const size_t e = (size_t)cursor[(size_t)sg.shard]++;
        tab[(size_t)S + 1 + 2 * e] = sg.local0;
        tab[(size_t)S + 1 + 2 * e + 1] = m->id_base + sg.global0;
    }
    M->seg_dev.reserve(tab.size() * 8);
    VDB_HIP(hipMemcpy(M->seg_dev.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    // ... and, for candidate re-scoring (global ids -> this shard's rows), every shard's (id0, local0, n) triples on ITS device
    for (int sh = 0; sh < S; ++sh) {
        std::vector<int64_t> tri;
        for (const auto &sg : M->segs)
            if (sg.shard == sh) {
                tri.push_back(m->id_base + sg.global0);
                tri.push_back(sg.local0);
                tri.push_back(sg.n);
            }
        M->nseg_shard[(size_t)sh] = (int)(tri.size() / 3);
        if (tri.empty()) tri.assign(3, 0);
        set_device(M->shards[(size_t)sh]->device);
        M->seg_shard[(size_t)sh].reserve(tri.size() * 8);
        VDB_HIP(hipMemcpy(M->seg_shard[(size_t)sh].p, tri.data(), tri.size() * 8, hipMemcpyHostToDevice));
    }
    M->seg_dirty = false;
}

void multi_create(int dim, int metric, const int *devs, int ndev, vdb_handle *out) {
    if (!out) throw Error(VDB_ERR_INVALID, "null output handle");
    if (!devs || ndev < 1 || ndev > kMaxMultiShards)
        throw Error(VDB_ERR_INVALID, "vdb_create_multi needs 1.." + std::to_string(kMaxMultiShards) + " device ids");
    std::unique_ptr<vdb_index_s> m(new vdb_index_s());
    m->multi = new vdb_multi_s();
    vdb_multi_s *M = m->multi;
    auto cleanup = [&] {
        for (auto *c : M->shards) (void)vdb_destroy(c);
        delete M;
        m->multi = nullptr;
    };
    try {
        for (int s = 0; s < ndev; ++s) {
            vdb_handle c = nullptr;
            const int rc = vdb_create(dim, metric, devs[s], &c);     // (validates dim / metric / device / gfx950)
            if (rc != VDB_OK) throw Error(rc, g_last_error);
            M->shards.push_back(c);
        }
        m->device = devs[0];
        m->dim = dim;
        m->D4 = M->shards[0]->D4;
        m->ksteps = M->shards[0]->ksteps;
        m->metric = metric;
        M->streams.assign((size_t)ndev, nullptr);
        M->done.assign((size_t)ndev, nullptr);
        M->q_stage.resize((size_t)ndev);
        M->pack.resize((size_t)ndev);
        M->cand_stage.resize((size_t)ndev);
        M->seg_shard.resize((size_t)ndev);
        M->nseg_shard.assign((size_t)ndev, 0);
        for (int s = 0; s < ndev; ++s) {
            set_device(devs[s]);
            VDB_HIP(hipStreamCreateWithFlags(&M->streams[(size_t)s], hipStreamNonBlocking));
            VDB_HIP(hipEventCreateWithFlags(&M->done[(size_t)s], hipEventDisableTiming));
            if (devs[s] != devs[0]) {           // direct xGMI copies between the primary and this device (else staged via host)
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, devs[s], devs[0]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devs[0], 0);
                (void)hipGetLastError();
            }
        }
        {
            set_device(devs[0]);
            VDB_HIP(hipStreamCreateWithFlags(&M->main_stream, hipStreamNonBlocking));
            VDB_HIP(hipEventCreateWithFlags(&M->q_ready, hipEventDisableTiming));
            for (int s = 1; s < ndev; ++s)
                if (devs[s] != devs[0]) {
                    int can = 0;
                    if (hipDeviceCanAccessPeer(&can, devs[0], devs[s]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devs[s], 0);
                    (void)hipGetLastError();
                }
        }
        M->pool.start(ndev);
    } catch (...) {
        M->pool.stop();
        cleanup();
        throw;
    }
    *out = m.release();
}

void multi_destroy(vdb_index_s *m) {
    vdb_multi_s *M = m->multi;
    M->pool.stop();
    const int S = multi_nshards(m);
    for (int s = 0; s < S; ++s) {
        set_device(M->shards[(size_t)s]->device);
        (void)hipDeviceSynchronize();
        if (M->streams[(size_t)s]) (void)hipStreamDestroy(M->streams[(size_t)s]);
        if (M->done[(size_t)s]) (void)hipEventDestroy(M->done[(size_t)s]);
    }
    {
        set_device(m->device);
        (void)hipDeviceSynchronize();
        if (M->main_stream) (void)hipStreamDestroy(M->main_stream);
        if (M->q_ready) (void)hipEventDestroy(M->q_ready);
    }
    for (auto *c : M->shards) (void)vdb_destroy(c);
    delete M;
    m->multi = nullptr;
}

void multi_clear_rows(vdb_index_s *m) {
    m->multi->segs.clear();
    m->multi->seg_dirty = true;
    m->multi->mode = 0;
    m->N = 0;
    m->built = false;
    m->ivf_built = false;
}

void multi_reset(vdb_index_s *m) {
    vdb_multi_s *M = m->multi;
    M->pool.run_all([&](int s) {
        const int rc = vdb_reset(M->shards[(size_t)s]);
        if (rc != VDB_OK) throw Error(rc, g_last_error);
    });
    multi_clear_rows(m);
}

int ivf_add_impl(vdb_handle hh, const float *x_host, int64_t n, int64_t id_base, const int32_t *given);

// vdb_add / vdb_add_device / vdb_ivf_add / vdb_ivf_add_assigned on a multi-device handle
void multi_add(vdb_index_s *m, const float *x, bool on_device, int64_t n, int64_t id_base, hipStream_t user_stream, bool ivf,
               const int32_t *given) {
    vdb_multi_s *M = m->multi;
    const int S = multi_nshards(m);
    if (n < 0) throw Error(VDB_ERR_INVALID, "negative row count");
    if (n > 0 && !x) throw Error(VDB_ERR_INVALID, "null corpus pointer");
    if (ivf && m->nlist <= 0) throw Error(VDB_ERR_STATE, "no centroids: train or set them first");
    const int want_mode = ivf ? 2 : 1;
    if (M->mode != 0 && M->mode != want_mode) {      // the children replace their corpus when the kind of add changes
        multi_reset(m);
    }
    if (M->mode != 0 && m->N > 0) require_same_id_base(m, id_base);
    else m->id_base = id_base;
    if (on_device) {
        set_device(m->device);
        VDB_HIP(hipStreamSynchronize(user_stream));         // (the rows are read by other streams / devices below)
    }
    const int64_t N0 = m->N;
    std::vector<int64_t> local0((size_t)S, 0);
    for (int s = 0; s < S; ++s) local0[(size_t)s] = M->mode == 0 ? 0 : M->shards[(size_t)s]->N;
    const int primary = m->device;
    try {
    M->pool.run_all([&](int s) {
        vdb_index_s *c = M->shards[(size_t)s];
        int64_t lo, hi;
        multi_block(n, S, s, lo, hi);
        const float *rows = x ? x + (size_t)lo * m->dim : nullptr;
        set_device(c->device);
        if (ivf) {
            const int rc = ivf_add_impl(c, rows, hi - lo, 0, given ? given + lo : nullptr);
            if (rc != VDB_OK) throw Error(rc, g_last_error);
        } else if (!on_device) {
            append_rows(c, rows, false, hi - lo, 0, nullptr);
        } else if (c->device == primary) {
            append_rows(c, rows, true, hi - lo, 0, M->streams[(size_t)s]);
            VDB_HIP(hipStreamSynchronize(M->streams[(size_t)s]));
        } else {                                            // rows on the primary device: peer copy, then a device add
            DevBuf tmp;
            if (hi > lo) {
                tmp.reserve((size_t)(hi - lo) * m->dim * sizeof(float));
                VDB_HIP(hipMemcpyPeer(tmp.p, c->device, rows, primary, (size_t)(hi - lo) * m->dim * sizeof(float)));
            }
            append_rows(c, tmp.as<float>(), true, hi - lo, 0, M->streams[(size_t)s]);
            VDB_HIP(hipStreamSynchronize(M->streams[(size_t)s]));
        }
    });
    } catch (...) {
        // one shard failed (out of memory, a bad row block): the others may already hold their blocks of this add -- an index
        // whose shards disagree about its rows must not answer queries.  Empty it, loudly: the caller adds again.
        try { multi_reset(m); } catch (...) { multi_clear_rows(m); }
        throw;
    }
    for (int s = 0; s < S; ++s) {
        int64_t lo, hi;
        multi_block(n, S, s, lo, hi);
        if (hi > lo) M->segs.push_back({s, local0[(size_t)s], hi - lo, N0 + lo});
    }
    M->seg_dirty = true;
    M->mode = want_mode;
    m->N = N0 + n;
    m->built = !ivf;
    m->ivf_built = ivf;
}

void ivf_search_device_impl(vdb_index_s *h, const float *dq, int64_t nq, int k, float *D, int64_t *I, double *PK, int64_t *PI,
                            hipStream_t st, bool filtered);

// One search over all shards.  q: host memory (host API) or device memory of the primary device (device API, `user_stream`
// has produced it).  Outputs: host (D, I) for the host API; primary-device (D, I) or partial (PK, PI) for the device API.
void multi_search(vdb_index_s *m, const float *q, bool device_api, int64_t nq, int k, float *D, int64_t *I, double *PK,
                  int64_t *PI, hipStream_t user_stream, bool ivf) {
    vdb_multi_s *M = m->multi;
    const int S = multi_nshards(m);
    if (ivf ? !m->ivf_built : !m->built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (nq < 0) throw Error(VDB_ERR_INVALID, "negative query count");
    m->last.last_nq = nq;
    if (nq == 0) return;
    const bool partial = PK != nullptr;
    if (!q || (partial ? !PI : (!D || !I))) throw Error(VDB_ERR_INVALID, "null pointer");
    const int primary = m->device;
    set_device(primary);
    multi_upload_segments(m);
    hipStream_t mst = device_api ? user_stream : M->main_stream;
    // queries per pass: the gathered partials (16 bytes per (shard, query, neighbour)) stay within 256 MiB
    const int64_t per_pass = std::max<int64_t>(512, ((int64_t)256 << 20) / ((int64_t)16 * k * S));
    for (int64_t b0 = 0; b0 < nq; b0 += per_pass) {
        const int64_t nb = std::min<int64_t>(per_pass, nq - b0);
        const size_t part_words = (size_t)2 * nb * k;                   // 8-byte words of one shard's packed partial
        M->gather.reserve((size_t)S * part_words * 8);
        if (!device_api) {
            M->out_d.reserve((size_t)nb * k * sizeof(float));
            M->out_i.reserve((size_t)nb * k * sizeof(int64_t));
        } else {
            VDB_HIP(hipEventRecord(M->q_ready, user_stream));
        }
        const float *qb = q + (size_t)b0 * m->dim;
        const size_t qbytes = (size_t)nb * m->dim * sizeof(float);
        M->pool.run_all([&](int s) {
            vdb_index_s *c = M->shards[(size_t)s];
            hipStream_t st = M->streams[(size_t)s];
            set_device(c->device);
            const float *qs = nullptr;
            const bool remote = c->device != primary || M->stage_all;
            if (!device_api) {
                M->q_stage[(size_t)s].reserve(qbytes);
                VDB_HIP(hipMemcpyAsync(M->q_stage[(size_t)s].p, qb, qbytes, hipMemcpyHostToDevice, st));
                qs = M->q_stage[(size_t)s].as<float>();
            } else {
                VDB_HIP(hipStreamWaitEvent(st, M->q_ready, 0));
                if (!remote) {
                    qs = qb;
                } else {
                    M->q_stage[(size_t)s].reserve(qbytes);
                    VDB_HIP(hipMemcpyPeerAsync(M->q_stage[(size_t)s].p, c->device, qb, primary, qbytes, st));
                    qs = M->q_stage[(size_t)s].as<float>();
                }
            }
            int64_t *slot = M->gather.as<int64_t>() + (size_t)s * part_words;
            int64_t *dst = slot;
            if (remote) {
                M->pack[(size_t)s].reserve(part_words * 8);
                dst = M->pack[(size_t)s].as<int64_t>();
            }
            double *pk = reinterpret_cast<double *>(dst);
            int64_t *pi = dst + (size_t)nb * k;
            if (ivf) ivf_search_device_impl(c, qs, nb, k, nullptr, nullptr, pk, pi, st);
            else search_device_impl(c, qs, nb, k, nullptr, nullptr, pk, pi, st);
            if (remote)
                VDB_HIP(hipMemcpyPeerAsync(slot, primary, dst, c->device, part_words * 8, st));
            VDB_HIP(hipEventRecord(M->done[(size_t)s], st));
        });
        for (int s = 0; s < S; ++s) VDB_HIP(hipStreamWaitEvent(mst, M->done[(size_t)s], 0));
        MergeArgs ma{};
        ma.pkeys = M->gather.as<double>();
        ma.pids = M->gather.as<int64_t>() + (size_t)nb * k;
        ma.part_stride = (int64_t)part_words;
        ma.slot_stride = k;
        ma.nparts = S;
        ma.k = k;
        ma.metric = m->metric;
        ma.count = nb;
        ma.seg = M->seg_dev.as<int64_t>();
        if (partial) {
            ma.okeys = PK + (size_t)b0 * k;
            ma.oids = PI + (size_t)b0 * k;
        } else if (device_api) {
            ma.D = D + (size_t)b0 * k;
            ma.I = I + (size_t)b0 * k;
        } else {
            ma.D = M->out_d.as<float>();
            ma.I = M->out_i.as<int64_t>();
        }
        launch_merge(ma, nb, mst);
        if (!device_api) {
            VDB_HIP(hipMemcpyAsync(D + (size_t)b0 * k, M->out_d.p, (size_t)nb * k * sizeof(float), hipMemcpyDeviceToHost, mst));
            VDB_HIP(hipMemcpyAsync(I + (size_t)b0 * k, M->out_i.p, (size_t)nb * k * sizeof(int64_t), hipMemcpyDeviceToHost, mst));
            VDB_HIP(hipStreamSynchronize(mst));
        } else if (b0 + per_pass < nq) {
            VDB_HIP(hipStreamSynchronize(mst));      // (the next pass reuses the gather buffer)
        }
    }
    m->last.last_path = M->shards[0]->last.last_path;
}

// vdb_rerank / vdb_rerank_device on a multi-device handle: every shard re-scores the candidates that are ITS rows (global ids
// mapped through its segment triples, the rest skipped), partial lists are gathered and merged as in multi_search.
void multi_rerank(vdb_index_s *m, const float *q, bool device_api, int64_t nq, const int64_t *cand, int ncand, int k, float *D,
                  int64_t *I, hipStream_t user_stream) {
    vdb_multi_s *M = m->multi;
    const int S = multi_nshards(m);
    if (!m->built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (nq < 0 || ncand < 0) throw Error(VDB_ERR_INVALID, "negative size");
    if (nq == 0) return;
    if (!q || !D || !I || (ncand > 0 && !cand)) throw Error(VDB_ERR_INVALID, "null pointer");
    const int primary = m->device;
    set_device(primary);
    multi_upload_segments(m);
    hipStream_t mst = device_api ? user_stream : M->main_stream;
    const size_t part_words = (size_t)2 * nq * k;
    const size_t qbytes = (size_t)nq * m->dim * sizeof(float), cbytes = (size_t)nq * std::max(ncand, 1) * sizeof(int64_t);
    M->gather.reserve((size_t)S * part_words * 8);
    if (!device_api) {
        M->out_d.reserve((size_t)nq * k * sizeof(float));
        M->out_i.reserve((size_t)nq * k * sizeof(int64_t));
    } else {
        VDB_HIP(hipEventRecord(M->q_ready, user_stream));
    }
    M->pool.run_all([&](int s) {
        vdb_index_s *c = M->shards[(size_t)s];
        hipStream_t st = M->streams[(size_t)s];
        set_device(c->device);
        const bool remote = c->device != primary || M->stage_all;
        const float *qs = q;
        const int64_t *cs = cand;
        if (!device_api) {
            M->q_stage[(size_t)s].reserve(qbytes);
            M->cand_stage[(size_t)s].reserve(cbytes);
            VDB_HIP(hipMemcpyAsync(M->q_stage[(size_t)s].p, q, qbytes, hipMemcpyHostToDevice, st));
            if (ncand > 0) VDB_HIP(hipMemcpyAsync(M->cand_stage[(size_t)s].p, cand, cbytes, hipMemcpyHostToDevice, st));
            qs = M->q_stage[(size_t)s].as<float>();
            cs = M->cand_stage[(size_t)s].as<int64_t>();
        } else {
            VDB_HIP(hipStreamWaitEvent(st, M->q_ready, 0));
            if (remote) {
                M->q_stage[(size_t)s].reserve(qbytes);
                M->cand_stage[(size_t)s].reserve(cbytes);
                VDB_HIP(hipMemcpyPeerAsync(M->q_stage[(size_t)s].p, c->device, q, primary, qbytes, st));
                if (ncand > 0) VDB_HIP(hipMemcpyPeerAsync(M->cand_stage[(size_t)s].p, c->device, cand, primary, cbytes, st));
                qs = M->q_stage[(size_t)s].as<float>();
                cs = M->cand_stage[(size_t)s].as<int64_t>();
            }
        }
        int64_t *slot = M->gather.as<int64_t>() + (size_t)s * part_words;
        int64_t *dst = slot;
        if (remote) {
            M->pack[(size_t)s].reserve(part_words * 8);
            dst = M->pack[(size_t)s].as<int64_t>();
        }
        rerank_device_impl(c, qs, nq, cs, ncand, k, nullptr, nullptr, st, reinterpret_cast<double *>(dst), dst + (size_t)nq * k,
                           M->seg_shard[(size_t)s].as<int64_t>(), M->nseg_shard[(size_t)s]);
        if (remote) VDB_HIP(hipMemcpyPeerAsync(slot, primary, dst, c->device, part_words * 8, st));
        VDB_HIP(hipEventRecord(M->done[(size_t)s], st));
    });
    for (int s = 0; s < S; ++s) VDB_HIP(hipStreamWaitEvent(mst, M->done[(size_t)s], 0));
    MergeArgs ma{};
    ma.pkeys = M->gather.as<double>();
    ma.pids = M->gather.as<int64_t>() + (size_t)nq * k;
    ma.part_stride = (int64_t)part_words;
    ma.slot_stride = k;
    ma.nparts = S;
    ma.k = k;
    ma.metric = m->metric;
    ma.count = nq;
    ma.D = device_api ? D : M->out_d.as<float>();
    ma.I = device_api ? I : M->out_i.as<int64_t>();
    launch_merge(ma, nq, mst);          // (the shards' partial ids are already global: no segment table)
    if (!device_api) {
        VDB_HIP(hipMemcpyAsync(D, M->out_d.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, mst));
        VDB_HIP(hipMemcpyAsync(I, M->out_i.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, mst));
        VDB_HIP(hipStreamSynchronize(mst));
    }
}

void multi_reserve(vdb_index_s *m, int64_t nq, int k) {
    vdb_multi_s *M = m->multi;
    const int S = multi_nshards(m);
    if (!(m->built || m->ivf_built)) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (nq < 0 || nq > (1ll << 24)) throw Error(VDB_ERR_INVALID, "query count out of range");
    if (nq == 0 || m->N == 0) return;
    const int64_t per_pass = std::max<int64_t>(512, ((int64_t)256 << 20) / ((int64_t)16 * k * S));
    const int64_t nb = std::min<int64_t>(nq, per_pass);
    M->pool.run_all([&](int s) {
        vdb_index_s *c = M->shards[(size_t)s];
        set_device(c->device);
        const int rc = vdb_reserve(c, nb, k);
        if (rc != VDB_OK) throw Error(rc, g_last_error);
        M->q_stage[(size_t)s].reserve((size_t)nb * m->dim * sizeof(float));
        if (c->device != m->device) M->pack[(size_t)s].reserve((size_t)2 * nb * k * 8);
    });
    set_device(m->device);
    M->gather.reserve((size_t)S * 2 * nb * k * 8);
    M->out_d.reserve((size_t)nb * k * sizeof(float));
    M->out_i.reserve((size_t)nb * k * sizeof(int64_t));
    multi_upload_segments(m);
}

void multi_stats(vdb_index_s *m, vdb_stats_t *out) {
    vdb_multi_s *M = m->multi;
    const int S = multi_nshards(m);
    vdb_stats_t s{};
    s.ntotal = m->N;
    s.dim = m->dim;
    s.metric = m->metric;
    s.corpus_fp16_exact = 1;
    s.has_i8_copy = 2;
    s.last_nq = m->last.last_nq;
    for (int i = 0; i < S; ++i) {
        vdb_stats_t c{};
        const int rc = vdb_stats(M->shards[(size_t)i], &c);
        if (rc != VDB_OK) throw Error(rc, g_last_error);
        s.bytes_resident += c.bytes_resident;
        s.bytes_workspace += c.bytes_workspace;
        s.last_candidates += c.last_candidates;
        s.last_rescan_bins += c.last_rescan_bins;
        s.last_fallback_queries += c.last_fallback_queries;
        s.last_rows_scanned += c.last_rows_scanned;
        s.upload_blocks += c.upload_blocks;
        s.last_scan_ms = std::max(s.last_scan_ms, c.last_scan_ms);        // (the shards run side by side)
        s.last_total_ms = std::max(s.last_total_ms, c.last_total_ms);
        s.last_prep_ms = std::max(s.last_prep_ms, c.last_prep_ms);
        s.last_tail_ms = std::max(s.last_tail_ms, c.last_tail_ms);
        if (c.ntotal > 0 || i == 0) {
            s.corpus_fp16_exact = s.corpus_fp16_exact && c.corpus_fp16_exact;
            s.has_i8_copy = std::min(s.has_i8_copy, c.has_i8_copy);
        }
        if (i == 0) {
            s.last_path = c.last_path;
            s.scan_dtype = c.scan_dtype;
            s.scan_shape = c.scan_shape;
            s.nlist = c.nlist;
            s.nprobe = c.nprobe;
        }
        s.bytes_resident += (int64_t)(M->q_stage[(size_t)i].cap + M->pack[(size_t)i].cap);
    }
    s.bytes_resident += (int64_t)(M->gather.cap + M->seg_dev.cap + M->out_d.cap + M->out_i.cap);
    s.ndevices = S;      // (scan_shape: the first shard's -- every shard is built with the same options)
    *out = s;
}

void multi_set_option(vdb_index_s *m, const char *key, double value) {
    vdb_multi_s *M = m->multi;
    if (std::string(key) == "graph") {
        if (value != 0) throw Error(VDB_ERR_UNSUPPORTED, "hipGraph replay is not available on a multi-device index");
        return;
    }
    if (std::string(key) == "multi_stage_all") {
        M->stage_all = value != 0;
        return;
    }
    for (auto *c : M->shards) {
        const int rc = vdb_set_option(c, key, value);
        if (rc != VDB_OK) throw Error(rc, g_last_error);
    }
}

void multi_set_centroids(vdb_index_s *m, const float *c_host, int nlist) {
    vdb_multi_s *M = m->multi;
    M->pool.run_all([&](int s) {
        const int rc = vdb_ivf_set_centroids(M->shards[(size_t)s], c_host, nlist);
        if (rc != VDB_OK) throw Error(rc, g_last_error);
    });
    multi_clear_rows(m);       // (new centroids: rows filed under the old ones are dropped, as on a single-device index)
    m->nlist = nlist;
}

// k-means runs once, on the first shard's device, over the WHOLE training set (approximate_search.py:44 trains on all
// vectors); every other shard gets the same centroids
void multi_train(vdb_index_s *m, int nlist, const float *x_host, int64_t n, int niter, uint64_t seed, int mppc) {
    vdb_multi_s *M = m->multi;
    int rc = vdb_ivf_train(M->shards[0], nlist, x_host, n, niter, seed, mppc);
    if (rc != VDB_OK) throw Error(rc, g_last_error);
    const std::vector<float> cent = M->shards[0]->ivf_centroids;
    M->pool.run_all([&](int s) {
        if (s == 0) return;
        const int r2 = vdb_ivf_set_centroids(M->shards[(size_t)s], cent.data(), nlist);
        if (r2 != VDB_OK) throw Error(r2, g_last_error);
    });
    multi_clear_rows(m);
    m->nlist = nlist;
}

void multi_get_assignment(vdb_index_s *m, int32_t *out) {
    vdb_multi_s *M = m->multi;
    if (!m->ivf_built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (!out && m->N) throw Error(VDB_ERR_INVALID, "null pointer");
    for (const auto &sg : M->segs) {
        const auto &lor = M->shards[(size_t)sg.shard]->ivf_list_of_row;
        memcpy(out + sg.global0, lor.data() + sg.local0, (size_t)sg.n * sizeof(int32_t));
    }
}

}  // namespace

extern "C" int vdb_create_multi(int dim, int metric, const int *devices, int ndev, vdb_handle *out) {
    return guarded([&] { multi_create(dim, metric, devices, ndev, out); });
}

// vdbhip.hip -- host side of libvdbhip.so: handle management, path selection, kernel launches,
// and the extern "C" entry points declared in include/vdbhip.h.  gfx950 only.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/vdbhip.h"
#include "common.hpp"
#include "prep.hpp"
#include "refine.hpp"
#include "scan.hpp"
#include "scan16.hpp"
#include "scan_i8.hpp"
#include "scan_i8x16.hpp"
#include "scan_x16.hpp"
#include "ivf.hpp"
#include "ivf_mfma.hpp"
#include "ivf_kloop.hpp"
#include "ivf_sq8.hpp"
#include "ivf_i8_plan.hpp"
#include "ivf_i8.hpp"
#include "ivf_pq.hpp"
#include "dense.hpp"
#include "lsh.hpp"
#include "lsh_tables.hpp"
#include "pq.hpp"
#include "pq_adc.hpp"
#include "ivf_pq_adc.hpp"
#include "knng.hpp"
#include "range.hpp"
#include "filter.hpp"
#include "ivf_filter.hpp"
#include "ivf_range.hpp"

using namespace vdb;

namespace {

thread_local std::string g_last_error;

// bumped by every (re)allocation or release of a DevBuf: a captured hipGraph holds raw buffer addresses, so it may only be
// replayed while no buffer of this process has moved since its capture (graph_or_run)
std::atomic<uint64_t> g_alloc_epoch{0};

// Diagnostic allocation log ($VDBHIP_ALLOC_LOG=<file>): one line per device / pinned allocation and release of this library
// ("A <ptr> <bytes>", "F <ptr> <bytes>", "HA"/"HF" for pinned host memory) and per hipGraph event of graph_or_run, flushed as
// it is written -- after a GPU memory fault the faulting address is resolved against it offline (live range, freed range,
// or not ours: profiles/r04_graph_fault_cause.txt).  Off unless the variable is set.
FILE *alloc_log() {
    static FILE *f = [] {
        const char *path = getenv("VDBHIP_ALLOC_LOG");
        return (path && *path) ? fopen(path, "a") : (FILE *)nullptr;
    }();
    return f;
}
void alloc_note(const char *what, const void *p, size_t bytes) {
    if (FILE *f = alloc_log()) {
        fprintf(f, "%s %p %zu\n", what, p, bytes);
        fflush(f);
    }
}

// growable device buffer that owns its memory: freed when it goes out of scope (a temporary of one API call is freed on every
// exit path, an Error thrown by a later hipMalloc included) or with the handle it is a member of.  `name` is what the
// $VDBHIP_ALLOC_LOG dump of a captured graph calls a member of a buffer group (for_each_buf below); temporaries have none.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool borrowed = false;      // a view into another DevBuf's memory (borrow): never freed here, cannot grow
    const char *name = nullptr;
    DevBuf() = default;
    explicit DevBuf(const char *member_name) : name(member_name) {}
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed), name(o.name) {      // (move-only: std::vector<DevBuf> in multi.inc)
        o.p = nullptr;
        o.cap = 0;
        o.borrowed = false;
    }
    ~DevBuf() { release(); }
    void borrow(void *ptr, size_t bytes) {
        if (!borrowed) release();
        p = ptr;
        cap = bytes;
        borrowed = true;
    }
    void reserve(size_t bytes) {
        if (bytes <= cap) return;
        require_owned();
        release();
        allocate(with_slack(bytes));
    }
    // exactly `bytes` (no growth slack): buffers of an index that is built once and never grows (int8-only build)
    void reserve_exact(size_t bytes) {
        if (bytes == cap && p) return;
        require_owned();
        release();
        allocate(bytes ? bytes : 16);
    }
    // reserve that keeps the first `keep` bytes (append): old and new allocation coexist for the copy
    void grow(size_t bytes, size_t keep) {
        if (bytes <= cap) return;
        require_owned();
        void *old = p;
        const size_t old_cap = cap;
        allocate(with_slack(bytes));         // (throws with the old buffer as it was: a failed append leaves the index intact)
        hipError_t e = hipSuccess;
        if (old && keep) e = hipMemcpy(p, old, keep, hipMemcpyDeviceToDevice);
        if (old) {
            alloc_note("F", old, old_cap);
            (void)hipFree(old);
        }
        if (e != hipSuccess) throw Error(VDB_ERR_HIP, std::string("device copy failed: ") + hipGetErrorString(e));
    }
    void release() {
        if (p && !borrowed) {
            g_alloc_epoch.fetch_add(1, std::memory_order_relaxed);
            alloc_note("F", p, cap);
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        borrowed = false;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }

  private:
    static size_t with_slack(size_t bytes) { return bytes + std::min<size_t>(bytes >> 3, (size_t)256 << 20); }   // (growth slack: 1/8, at most 256 MiB)
    void require_owned() const {
        if (borrowed) throw Error(VDB_ERR_INVALID, "internal: a borrowed device buffer cannot grow");
    }
    // the one place that allocates device memory: epoch bump, hipMalloc, error text, log line; throws with p / cap untouched
    void allocate(size_t bytes) {
        g_alloc_epoch.fetch_add(1, std::memory_order_relaxed);
        void *fresh = nullptr;
        if (hipMalloc(&fresh, bytes) != hipSuccess) {
            (void)hipGetLastError();
            throw Error(VDB_ERR_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
        }
        p = fresh;
        cap = bytes;
        alloc_note("A", p, cap);
    }
};

// ---- buffer groups ---------------------------------------------------------------------------------------------------------
// The device buffers of a handle sit in a few plain structs, one per LIFETIME (what frees them together), whose only data
// members are DevBufs declared with their name.  for_each_buf walks such a struct as the array of DevBufs it is, so a new
// buffer is one declaration: its bytes are counted (vdb_stats), it is freed with its group (vdb_reset, a rebuild) and with
// the handle, and the graph dump of $VDBHIP_ALLOC_LOG names it, without a list anywhere to add it to.
template <class G, class F>
void for_each_buf(G &g, F &&f) {
    static_assert(std::is_standard_layout<G>::value && sizeof(G) % sizeof(DevBuf) == 0, "a buffer group holds DevBuf members only");
    DevBuf *b = reinterpret_cast<DevBuf *>(&g);
    for (size_t i = 0; i < sizeof(G) / sizeof(DevBuf); ++i) f(b[i].name, b[i]);
}
template <class G>
size_t group_bytes(G &g) {
    size_t s = 0;
    for_each_buf(g, [&](const char *, DevBuf &b) { s += b.cap; });
    return s;
}
template <class G>
void group_release(G &g) {
    for_each_buf(g, [](const char *, DevBuf &b) { b.release(); });
}

// the float32 rows and their norms                                                            (freed by vdb_reset)
struct RowBufs {
    DevBuf x32{"x32"}, xnorm2{"xnorm2"};
};
// the scan copies derived from the rows (an append frees and re-derives them): fp16 panels and bias, the scratch slab of a
// streamed index, and the int8 copy (scan_i8.hpp) of byte-valued integer corpora with D <= 128, kept NEXT TO the fp16 panels
// (a batch of non-integer queries still takes the fp16 scan)                                  (freed by vdb_reset)
struct ScanBufs {
    DevBuf panels{"panels"}, slab{"slab"}, bias{"bias"};
    DevBuf panels8{"panels8"}, bias8{"bias8"}, rows8{"rows8"}, rowstat8{"rowstat8"};  // rows8 / rowstat8: row-major int8 copy + {sum x^2, sum x} for the list refine
    DevBuf pq_tab{"pq_tab"};                                 // PQ: the codebooks scaled by sx and rounded to fp16, [M][256][dsub] (pq.hpp)
};
// what outlives the rows: the corpus statistics block, and what vdb_ivf_train / set_* installed   (freed with the handle)
struct KeptBufs {
    DevBuf stats{"stats"};
    DevBuf sq8_cent{"sq8_cent"}, sq8_param{"sq8_param"};     // SQ8: centroids [nlist][D4] (IVF-PQ too) and {vmin, vdiff} [2][D4], zero padded
    DevBuf lsh_rt{"lsh_rt"};                                 // sign-LSH: R transposed [dim][nbits]
    DevBuf lsht_pt{"lsht_pt"}, lsht_off{"lsht_off"};         // hash-table LSH: projections transposed [dim][T * H], offsets [T * H]
    DevBuf pq_cb{"pq_cb"};                                   // PQ: codebooks float32 [M][256][dsub]
    DevBuf ivfpq_cb{"ivfpq_cb"};                             // IVF-PQ: codebooks of the residuals, float32 [M][256][dsub]
};
// IVF: the CSR arrays and the panel space (lists padded to whole spans) of the filed rows      (freed by vdb_reset)
struct IvfListBufs {
    DevBuf ivf_offsets{"ivf_offsets"}, ivf_ids{"ivf_ids"};
    DevBuf ivf_list_pspan0{"ivf_list_pspan0"}, ivf_span_row0{"ivf_span_row0"}, ivf_span_valid{"ivf_span_valid"};
};
// IVF: the per-batch plan of the list-major scan and the coarse result                        (freed with the handle)
struct IvfPlanBufs {
    DevBuf ivf_probe_d{"ivf_probe_d"}, ivf_probe_i{"ivf_probe_i"};
    // everything an IVF search needs zeroed, in ONE buffer cleared by ONE memset per batch (each memset is a ~4 us dispatch
    // of its own): [coarse quantizer's ws.small | this handle's ws.small | per-list counts | cursors | slot -> query map |
    // arrival counters of the flagged-query pass].  Both ws.small are views into it (DevBuf::borrow).
    DevBuf ivf_zero{"ivf_zero"};
    DevBuf ivf_slot_off{"ivf_slot_off"}, ivf_list_item0{"ivf_list_item0"}, ivf_item_list{"ivf_item_list"};
    DevBuf ivf_item_slot0{"ivf_item_slot0"}, ivf_item_bin0{"ivf_item_bin0"}, ivf_plan{"ivf_plan"}, ivf_slot_of{"ivf_slot_of"};
};
// compressed codes of the rows                                                                (freed by vdb_reset)
struct CodeBufs {
    DevBuf sq8_codes{"sq8_codes"}, sq8_list{"sq8_list"};     // SQ8: [N][D4] codes and the list of every row (IVF-PQ too), both in list order
    DevBuf lsh_codes{"lsh_codes"};                           // sign-LSH: codes [N][lsh_wp]
    DevBuf lsht_keys{"lsht_keys"};                           // hash-table LSH: table keys [N][lsht_kw]
    DevBuf pq_codes{"pq_codes"};                             // PQ: codes [N][M] in id order (+ 16 spare bytes)
    DevBuf ivfpq_codes{"ivfpq_codes"};                       // IVF-PQ: codes [N][M] in list order
    DevBuf ivfpq_n2{"ivfpq_n2"};                             // IVF-PQ, option "ivfpq_adc_max_batch" only: ||x^||^2 float32 [N] in list order, made by the first
                                                             // admitted batch after an add (ivfpq_adc_prepare; held = valid)
    DevBuf knng_nbrs{"knng_nbrs"};                           // k-NN graph: local row numbers [N][knng_degree], -1 tails
};
// per-search workspace of the LSH calls                                                       (freed with the handle)
struct LshWorkspace {
    DevBuf lsh_qcodes{"lsh_qcodes"}, lsh_hist{"lsh_hist"}, lsh_small{"lsh_small"}, lsh_list{"lsh_list"}, lsh_stat{"lsh_stat"};
    DevBuf lsh_cand_i{"lsh_cand_i"}, lsh_cand_h{"lsh_cand_h"};
    DevBuf lsht_empty{"lsht_empty"};                         // hash-table LSH: count + list of the queries without a colliding row
};
// per-search workspace of the k-NN graph search: the counters, and L between the launches of a timed call   (freed with the handle)
struct KnngWorkspace {
    DevBuf knng_stat{"knng_stat"}, knng_state_k{"knng_state_k"}, knng_state_i{"knng_state_i"}, knng_entry{"knng_entry"};
};
// per-search workspace                                                                        (freed with the handle)
struct Workspace {
    DevBuf qpad{"ws.qpad"}, qpanels{"ws.qpanels"}, qpanels8{"ws.qpanels8"}, qrows8{"ws.qrows8"}, info{"ws.info"}, eps{"ws.eps"};
    DevBuf bin_m1{"ws.bin_m1"}, bin_m2{"ws.bin_m2"}, bin_m3{"ws.bin_m3"}, bin_m4{"ws.bin_m4"}, bin_m5{"ws.bin_m5"};
    DevBuf sb_m1{"ws.sb_m1"}, sb_m2{"ws.sb_m2"}, sb_span{"ws.sb_span"};
    DevBuf cand{"ws.cand"}, rescan{"ws.rescan"}, counts{"ws.counts"}, fallback{"ws.fallback"}, fb_list{"ws.fb_list"};
    DevBuf fb_done{"ws.fb_done"};           // arrival counters of refine_fallback_body (refine_tail_kernel)
    DevBuf small{"ws.small"};               // fb_count (int) + 2 stat counters
    DevBuf dense{"ws.dense"};               // nq x Npad raw scores of the small-corpus path
    DevBuf pkeys{"ws.pkeys"}, pids{"ws.pids"};      // partial lists of the exhaustive / fallback passes
    DevBuf stage_q{"ws.stage_q"}, stage_d{"ws.stage_d"}, stage_i{"ws.stage_i"};  // host-API staging
    DevBuf sq8_panels{"ws.sq8_panels"};     // IVF-SQ8 / IVF-PQ / IVF-I8: the fp16 panels converted from the codes (the int8 panels) for the current batch
    DevBuf adc_tab{"ws.adc_tab"};           // PQ / IVF-PQ, ADC scan: the float32 lookup tables of the current batch, [nq][M][256] (pq_adc.hpp)
    DevBuf adc_scores{"ws.adc_scores"};     // IVF-PQ, ADC scan: the scores of the probed rows, [nq][stride] (ivf_pq_adc.hpp)
    DevBuf adc_aux{"ws.adc_aux"};           // ... its scale, flags, B [nq][nprobe] and score positions [nq][nprobe + 1]
};

// the last range search of the handle (range.inc): its result -- lims, D, I -- and the workspace of the call, the candidate bitmap of one
// query slab first of all                                                                      (freed by vdb_reset and with the handle)
struct RangeBufs {
    DevBuf lims{"range.lims"}, D{"range.D"}, I{"range.I"};
    DevBuf bitmap{"range.bitmap"}, seg{"range.seg"}, qtot{"range.qtot"}, stat{"range.stat"};
    DevBuf qstage{"range.qstage"}, qpad{"range.qpad"}, qpanels{"range.qpanels"}, info{"range.info"}, eps{"range.eps"}, thr{"range.thr"}, flag{"range.flag"};
};

// the installed filter of the handle (filter.inc): the allow words (tail clean, padded to Npad rows), the masked copies of the
// scans' accumulator inits, the ascending list of admitted rows with its segment offsets when the sparse route may need it, and
// the admitted count; every buffer sized exactly        (freed by vdb_filter_clear, vdb_reset and with the handle; dropped by any add
// and vdb_set_option)
struct FilterBufs {
    DevBuf words{"filter.words"}, bias_f{"filter.bias_f"}, bias8_f{"filter.bias8_f"};
    DevBuf list{"filter.list"}, seg{"filter.seg"}, count{"filter.count"};
};

// the installed filter of an IVF-Flat handle (ivf_filter.inc): the allow words in LIST order, the masked copies of the panel space's
// accumulator inits and the admitted count; every buffer sized exactly (ivf_filter_bytes)        (freed and dropped as FilterBufs, and
// by any vdb_ivf_add*, vdb_ivf_set_centroids and vdb_ivf_train)
struct IvfFilterBufs {
    DevBuf words{"ivf_filter.words"}, bias_f{"ivf_filter.bias_f"}, bias8_f{"ivf_filter.bias8_f"}, count{"ivf_filter.count"};
};

// (struct Options -- everything vdb_set_option writes -- is in scan_plan.hpp: the launch rules of the flat scans read it)

void release_pins(vdb_index_s *h);       // (the pinned staging blocks of upload_rows)

// The host side of one set of product-quantizer codebooks (pq.inc): a handle keeps two, those of a flat PQ<M> index and
// those of the residuals of an IVF<nlist>,PQ<M> index.  The device copy sits in the `kept` group.
struct PqCodebooks {
    int M = 0, dsub = 0;                     // sub-spaces (0 = no codebooks) and dims of each
    std::vector<float> host;                 // host copy [M][256][dsub]
};

inline QueryBatchInfo *batch_info(Workspace &ws) {        // inside ws.small (common.hpp, kInfoOffset)
    return reinterpret_cast<QueryBatchInfo *>(ws.small.as<char>() + kInfoOffset);
}

}  // namespace

struct vdb_multi_s;           // multi.inc: the shards, streams and host threads of a multi-device handle

struct vdb_index_s {
    vdb_multi_s *multi = nullptr;            // non-null: a multi-device handle (vdb_create_multi); device = the primary device,
                                             // N / id_base / built / ivf_built / nlist / nprobe describe the whole index
    int device = 0;
    int n_cus = 256;                         // compute units of `device` (vdb_create; a coarse quantizer takes its parent's)
    int dim = 0, D4 = 0, ksteps = 0, metric = 0;
    int64_t N = 0, Npad = 0, id_base = 0;
    bool built = false;
    // device memory, grouped by lifetime (buffer groups above); every group is listed ONCE more, in for_each_group below
    RowBufs rows;
    ScanBufs scan;
    KeptBufs kept;
    IvfListBufs lists;                       // (flat handles leave the IVF / SQ8 / LSH groups empty)
    IvfPlanBufs plan;
    CodeBufs codes;
    LshWorkspace lsh_ws;
    KnngWorkspace knng_ws;
    Workspace ws;
    RangeBufs range;
    FilterBufs filter;
    IvfFilterBufs ivf_filter;
    Options opt;                            // what vdb_set_option has set; every other member is the library's own state
    int rows8_pitch = 0;
    bool i8_ok = false;
    bool x16 = false;                        // the flat scan copies (fp16 and int8, D <= 128) are in layout "x16": 16x16x32 f16 / 16x16x64 i8 MFMA,
                                             // octs only (scan_x16.hpp, scan_i8x16.hpp); corpora the dense small-corpus path serves keep 32-row tiles
    bool int8_only = false;                  // option "int8_only" took effect at the last add: only the int8 copies are kept (build_int8_only)
    // a captured device-resident search (option "graph", graph_or_run)
    struct GraphKey {
        const void *q = nullptr, *o1 = nullptr, *o2 = nullptr;
        int64_t nq = 0;
        int k = 0, kind = 0, nprobe = 0;
        hipStream_t st = nullptr;
        bool operator==(const GraphKey &o) const {
            return q == o.q && o1 == o.o1 && o2 == o.o2 && nq == o.nq && k == o.k && kind == o.kind && nprobe == o.nprobe && st == o.st;
        }
    } graph_key, graph_warm;
    hipGraphExec_t graph_exec = nullptr;
    hipEvent_t graph_ev = nullptr;           // recorded behind every launch of graph_exec (graph_drop_exec waits for it)
    uint64_t graph_epoch = 0;                // g_alloc_epoch when the graph was captured
    int64_t graph_replays = 0;
    int i8_cx = 0, i8_ks = 0;
    int i8_min = 0, i8_max = 0;              // IVF-I8 (ivf_i8.inc): smallest / largest value of the filed rows -- an append re-chooses the byte window over old and new rows
    // host copies of the corpus statistics
    float absmax = 0.f, maxnorm2 = 0.f, sx = 1.f;
    bool nonfinite = false, corpus_int_unscaled = false, corpus_fp16_exact = false, scan_ok = false;
    // row-block ingestion: two pinned staging buffers (upload_rows)
    void *pin[2] = {nullptr, nullptr};
    size_t pin_bytes = 0;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    int64_t last_upload_blocks = 0;          // blocks of the last host upload (vdb_stats: upload_blocks)
    bool small_clear_pending = false;        // search_device_impl left the clearing of ws.small to the first batch (serving-shaped calls)
    bool small_is_clean = false;             // ws.small was cleared for this call and no batch has used it yet
    bool small_preset = false;               // coarse quantizer of an IVF index: the parent has just cleared ws.small (it lives in
                                             // the parent's ivf_zero buffer) -- the next search_device_impl skips its own memset
    int64_t info_valid_nq = -1;              // queries whose statistics the last search_batch left in batch_info(ws) (-1: none)
    bool tile16 = false;                     // panels in the p16 layout (16-row tiles, 1024-row spans, 4 bins per span)
    bool panels_streamed = false;            // option "stream_panels" took effect at the last add (D > 128): the fp16 panels are not kept
    bool set_only = false;                   // coarse quantizer of an IVF index: callers use the SET of the k nearest rows,
                                             // not their order or distances (dense.hpp, DenseSelectArgs.set_only)
    vdb_stats_t last{};
    // timing mode: HIP-event pairs recorded on the search stream around the dominant kernel and the whole
    // device pipeline of every search since timing was switched on (read back by vdb_stats)
    std::vector<hipEvent_t> ev_scan, ev_total;   // [2*i], [2*i+1] = start, stop
    size_t ev_used = 0;
    // ivf (flat handles leave these empty)
    int nlist = 0, nprobe = 1;
    bool ivf_built = false;
    vdb_index_s *coarse = nullptr;           // flat index over the centroids (same metric)
    std::vector<float> ivf_centroids;        // host copy [nlist][dim]
    std::vector<int64_t> ivf_offsets_host;   // [nlist+1]
    std::vector<int32_t> ivf_list_of_row;    // [N] list of every indexed row (original order)
    // list-major MFMA scan (D <= 128): panel space = lists padded to whole 512-row spans
    bool ivf_mfma_ok = false, ivf_last_mfma = false;
    int64_t ivf_pspans = 0;
    int ivf_max_pspans = 0;
    int ivf_span_rows = kSpanRows;           // rows per panel span: 512 (32-row tiles, D <= 128) or 16 * ivf_tps (p16, D > 128)
    int ivf_tps = 0;                         // p16 tiles per span of the IVF panel space (16 / 64; option "ivf_tps" or the rule of ivf.inc)
    // codec of the inverted lists (vdb_ivf_set_codec): 0 Flat (float32 rows + scan copies) | 1 SQ8 (ivf_sq8.inc: 8-bit codes
    // of the residuals, no float32 rows, no scan copies) | 2 PQ (ivf_pq.inc: M-byte product codes of the residuals, likewise)
    // | 3 I8 (ivf_i8.inc: a byte-valued corpus as int8 rows, lossless; only the int8 scan copies are kept)
    int ivf_codec = 0;
    bool sq8_ranges = false;                 // vmin / vdiff trained or set
    std::vector<float> sq8_vmin, sq8_vdiff;  // host copies [dim]
    PqCodebooks ivfpq;                       // IVF-PQ: the codebooks of the residuals (M = 0: none yet) -- NOT `pq`: that marks a flat PQ handle
    // IVF-PQ ADC scan (ivfpq_adc_prepare, valid while codes.ivfpq_n2 is held): max ||x^||^2, Cn + Rn = max ||c_l|| + sqrt(sum_m max_c
    // ||cb[m][c]||^2), and whether both lie in the range the scan's scale can serve
    double ivfpq_adc_xn2 = 0.0, ivfpq_adc_cr = 0.0;
    bool ivfpq_adc_ok = false;
    // sign-LSH codes of a flat index (lsh.inc; vdb_lsh_set_projection): one bit per projection row, kept next to the float32 rows
    int lsh_nbits = 0, lsh_wp = 0;           // bits per row (0 = no projection); words per stored code (nbits / 32 rounded up to a power of two)
    int64_t lsh_rows = 0;                    // rows lsh_codes covers (== N whenever the index is searchable)
    std::vector<float> lsh_proj;             // host copy of R [nbits][dim]
    // hash-table LSH of a flat index (lsh_tables.inc; vdb_lsht_set_tables): T keys per row, kept next to the float32 rows
    int lsht_T = 0, lsht_H = 0, lsht_mode = 0;   // tables (0 = none), projections per table, 0 sign keys | 1 E2 bucket keys
    int lsht_W = 0, lsht_wp = 0, lsht_kw = 0;    // words per table key: of the contract, as stored (lsh_tables.hpp); lsht_kw = T * lsht_wp per row
    float lsht_width = 0.f;                  // E2: bucket width
    int64_t lsht_rows = 0;                   // rows lsht_keys covers (== N whenever the index is searchable)
    std::vector<float> lsht_proj, lsht_off;  // host copies [T][H][dim], [T][H]
    // flat PQ<M> index (pq.inc; vdb_pq_train / vdb_pq_set_codebooks): M code bytes per row, no float32 rows and no resident scan
    // copies -- every search makes its fp16 panels from the codes, slab by slab, in scan.slab
    PqCodebooks pq;                          // (M = 0: not a PQ index)
    // k-NN graph of a flat index (knng.inc; vdb_knng_build / vdb_knng_set): ntotal x degree local row numbers next to the float32 rows
    int knng_degree = 0;                     // 0 = no graph (any add and vdb_reset drop it)
    std::vector<int32_t> knng_entries;       // the entry rows knng_ws.knng_entry holds (knng_search_impl)
    // the last range search (range.inc; on an IVF-Flat handle ivf_range.inc): `range` holds its result while range_valid (any add,
    // vdb_reset, vdb_set_option, vdb_ivf_set_centroids and vdb_ivf_train drop it)
    bool range_valid = false;
    int64_t range_total = 0, range_nq = 0;   // lims[nq] and nq of that result
    int64_t range_cand = 0, range_fb = 0;    // (query, row) pairs scored exactly / queries for which every row was a candidate
    // the installed filter (filter.inc): `filter` holds it while filter_valid (any add, vdb_reset, vdb_set_option and a change of
    // kind drop it)
    bool filter_valid = false, filter_has_list = false;
    unsigned filter_kind = 0;                // kind_of the handle at install
    int64_t filter_count = 0;                // rows it admits
    int64_t filter_cand = 0;                 // (query, row) pairs the last sparse-route search scored
    // the installed filter of an IVF-Flat handle (ivf_filter.inc), dropped with the flat one (filter_drop)
    bool ivf_filter_valid = false;
    int64_t ivf_filter_count = 0;            // rows it admits
    // vdb_destroy has set the device, synchronised it, dropped the graph and destroyed `coarse` (whose ws.small is a view into
    // plan.ivf_zero); the buffer groups free themselves after this body
    ~vdb_index_s() {
        ws.small.release();                  // (our own view into plan.ivf_zero goes before that does)
        if (graph_ev) (void)hipEventDestroy(graph_ev);
        release_pins(this);
        for (auto e : pin_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto e : ev_scan) (void)hipEventDestroy(e);
        for (auto e : ev_total) (void)hipEventDestroy(e);
    }
};

namespace {

// ---- kinds of handle -------------------------------------------------------------------------------------------------------
// What a handle IS decides which entry points it admits and which options it refuses.  kind_of is the only place that reads
// the raw fields to decide that (computed, not stored: nothing to keep in step); kKinds names each kind in messages; admit is
// the first line of every entry point, its mask the kinds that call serves; refuse_options_set is the option rule of kOptions
// read in the other order.  A new kind is one enum bit (and a wider kAnyKind), one row of kKinds, a test in kind_of and its own masks.
enum Kind : unsigned { kFlat = 1, kLsh = 2, kKnng = 4, kPq = 8, kIvfFlat = 16, kIvfSq8 = 32, kIvfPq = 64, kMulti = 128, kLsht = 256, kIvfI8 = 512 };
constexpr unsigned kAnyKind = 1023, kIvf = kIvfFlat | kIvfSq8 | kIvfPq | kIvfI8;
constexpr struct { unsigned kind; const char *phrase; } kKinds[] = {
    {kMulti, "a multi-device index (vdb_create_multi)"},
    {kPq, "a flat PQ index (vdb_pq_*: its rows are codes, its panels are made per search in layout \"x16\" only)"},
    {kIvfPq, "an IVF-PQ index (vdb_ivf_set_codec 2, vdb_ivfpq_*: its rows are codes in list order)"},
    {kIvfSq8, "an IVF index with the SQ8 codec (its rows are codes in list order)"},
    {kIvfI8, "an IVF-I8 index (vdb_ivf_set_codec 3: its rows are int8 bytes in list order, it keeps no float32 rows)"},
    {kIvfFlat, "an IVF index (centroids set: its rows sit in list order)"},
    {kLsh, "an index with sign-LSH codes (vdb_lsh_set_projection: it stays a flat index)"},
    {kLsht, "an index with LSH hash tables (vdb_lsht_set_tables: it stays a flat index)"},
    {kKnng, "an index with a k-NN graph (vdb_knng_build / vdb_knng_set: it stays a flat index)"},
    {kFlat, "a flat index"}};

unsigned kind_of(const vdb_index_s *h) {
    if (h->multi) return kMulti;             // (nlist / ivf_built of such a handle describe the whole index)
    const unsigned ivf = h->ivf_codec == 3 ? kIvfI8 : h->ivf_codec == 2 ? kIvfPq : h->ivf_codec == 1 ? kIvfSq8 : (h->nlist > 0 || h->coarse || h->ivf_built) ? kIvfFlat : 0;
    const unsigned k = (h->pq.M > 0 ? kPq : 0) | ivf | (h->lsh_nbits > 0 ? kLsh : 0) | (h->knng_degree > 0 ? kKnng : 0) | (h->lsht_T > 0 ? kLsht : 0);
    if (k & (k - 1)) throw Error(VDB_ERR_STATE, "internal: handle is two kinds at once");
    return k ? k : kFlat;
}

const char *kind_phrase(unsigned kind) {
    for (const auto &k : kKinds)
        if (k.kind & kind) return k.phrase;
    return "this handle";
}

// `what` (an entry point, or what it would make of the handle) on a handle whose kind is not in `accepted`; `hint`: what to do instead
inline void admit(const vdb_index_s *h, const char *what, unsigned accepted, int code_if_not = VDB_ERR_UNSUPPORTED, const char *hint = "") {
    const unsigned kind = kind_of(h);
    if (!(kind & accepted)) throw Error(code_if_not, std::string(what) + " is not available on " + kind_phrase(kind) + hint);
}

struct OptionRow {
    const char *name;
    int Options::*m;
    int n;                     // > 0: one of v[0 .. n), integers only | 0: v[0] <= value <= v[1], truncated toward zero | < 0: any value, stored as value != 0
    double v[4];
    unsigned not_on = 0;       // kinds of index that refuse a non-zero value
    int not_on_pq = 0;         // a value that a PQ index refuses as well: its panels are made in layout "x16" (octs) only
    int64_t Options::*m64 = nullptr;       // instead of m
    bool vdb_index_s::*effect = nullptr;   // set while the value of the last add is in effect, whatever the option says now
};
constexpr unsigned kNoRows = kIvfSq8 | kPq | kIvfPq | kIvfI8, kNeedsRows = kLsh | kKnng | kLsht;     // no float32 rows at all | encoded from / searched against the resident ones
constexpr OptionRow kOptions[] = {
    {"force_path", &Options::force_path, 4, {0, 1, 2, 3}},
    {"timing", &Options::timing, -1, {}},                            // (re)starts the recording window
    {"list_cap", &Options::list_cap, 0, {0, 65536}},
    {"panel_dtype", &Options::panel_dtype, 2, {0, 1}},               // 0 auto (int8 scan copy used when corpus and queries allow), 1 = fp16 scan only
    {"int8_only", &Options::int8_only, 2, {0, 1}, kNoRows | kNeedsRows, 0, nullptr, &vdb_index_s::int8_only},
    {"int8_slab_chunks", &Options::int8_slab_chunks, 0, {0, 1024}},
    {"int8_block_rows", &Options::int8_block_rows, 0, {0, 2147483647}},
    {"stream_panels", &Options::stream_panels, 2, {0, 1}, kNoRows | kNeedsRows, 0, nullptr, &vdb_index_s::panels_streamed},   // D > 128, next add: 0 keep the fp16 panels resident | 1 convert them per search
    {"stream_slab_rows", nullptr, 0, {0, HUGE_VAL}, 0, 0, &Options::stream_slab_rows},   // rows of the scratch slab of a streamed index (0 = default 1 280 000)
    {"upload_block_mb", &Options::upload_block_mb, 0, {0, 4096}},    // staging block of the row-block ingestion (0 = default 64 MiB)
    {"small_batch", &Options::small_batch, 2, {0, 1}},               // 1 (default): finer chunks / narrower workgroups for batches <= 512 queries
    {"fused_stats", &Options::fused_stats, 2, {0, 1}},               // 1 (default) | 0: separate query_stats_kernel for every batch size (A/B)
    {"ivf_min_batch", &Options::ivf_min_batch, 0, {1, 1e9}},
    {"ivf_i8_scratch", &Options::ivf_i8_scratch, 2, {0, 1}},         // IVF-I8: 1 (default) fp16 panels converted per batch for the batches the int8 scan cannot serve | 0: never, those batches take the exact list scan
    {"graph", &Options::graph, 2, {0, 1}, kNoRows},
    {"graph_recapture_at_once", &Options::graph_recapture_at_once, -1, {}},   // diagnostic: destroy a stale exec and capture its successor in ONE call
    {"lsh_force_fallback", &Options::lsh_force_fallback, 2, {0, 1}}, // 1: every query of an LSH call takes the exact fallback of the select (tests)
    {"pq_slab_chunks", &Options::pq_slab_chunks, 0, {0, 4096}},      // PQ: scan chunks per slab of panels made per search (0 = default: 524 288 rows' worth)
    {"pq_scan_min_batch", &Options::pq_scan_min_batch, 0, {0, 1e9}}, // PQ: smallest query batch that takes the panel pass + MFMA scan (0 = default)
    {"pq_adc_max_batch", &Options::pq_adc_max_batch, 0, {0, 512}},   // PQ: largest query batch that takes the lookup-table (ADC) scan of the codes (0 = off)
    {"ivfpq_adc_max_batch", &Options::ivfpq_adc_max_batch, 0, {0, 512}},   // IVF-PQ: largest query batch that takes the lookup-table (ADC) scan of the probed lists (0 = off)
    {"ivfpq_adc_part_rows", &Options::ivfpq_adc_part_rows, 0, {0, 65536}},   // ... rows per row part of that scan: 0 auto, else a multiple of 256
    {"knng_nentry", &Options::knng_nentry, 0, {0, 512}},             // k-NN graph: entry points of a search (0 = default 32)
    {"knng_max_iters", &Options::knng_max_iters, 0, {0, 2147483647}},   // k-NN graph: step cap of a search (0 = default 8 ef)
    {"knng_visited_bits", &Options::knng_visited_bits, 0, {0, 14}},  // k-NN graph: log2 slots of the seen filter (0 = default; never changes a result)
    {"knng_build_block", &Options::knng_build_block, 0, {0, 1e9}},   // k-NN graph: rows per self-search block of the build (0 = default 65 536)
    {"range_bitmap_mb", &Options::range_bitmap_mb, 0, {0, 4096}},    // range search: MiB of candidate bitmap per query slab (0 = default 256)
    {"filter_sparse_pairs", nullptr, 0, {0, HUGE_VAL}, 0, 0, &Options::filter_sparse_pairs},   // filtered search: (query, admitted row) pairs below which the sparse route serves a call (0 = never by this rule)
    {"i8_variant", &Options::i8_variant, 0, {0, 7}},
    {"i8_group", &Options::i8_group, 2, {4, 8}, 0, 4},               // rows per select group of the int8 scan: 8 (octs, default) or 4 (quads)
    {"f16_group", &Options::f16_group, 2, {4, 8}, 0, 4},             // rows per select group of the fp16 flat scan: 8 (octs, default) or 4 (quads)
    {"flat_shape", &Options::flat_shape, 3, {0, 16, 32}, 0, 32},     // MFMA shape of the flat scans, D <= 128 (layout of the scan copies: set before vdb_add)
    {"i8_shape", &Options::flat_shape, 3, {0, 16, 32}, 0, 32},       // (alias)
    {"scan_pair", &Options::scan_pair, 2, {0, 1}},                   // 1 (default): both x16 scans of an index with an int8 copy in one launch; 0: two launches
    {"scan_prio", &Options::scan_prio, 0, {0, 2}},
    {"f16_wide", &Options::f16_wide, 2, {0, 1}},
    {"f16_stage_tiles", &Options::f16_stage_tiles, 3, {0, 4, 8}},
    {"i8_nt", &Options::i8_nt, 3, {0, 1, 2}},
    {"i8_ring", &Options::i8_ring, 4, {0, 2, 4, 8}},                 // staging ring of the serving-shaped / IVF int8 scans: 0 auto, 2 (double buffer), 4, 8
    {"select_variant", &Options::select_variant, 0, {0, 2}},
    {"spans_per_chunk", &Options::spans_per_chunk, 0, {0, 4096}},    // tuning: rows per workgroup chunk = 512 * value (0 = default 16)
    {"kloop_qgroup", &Options::kloop_qgroup, 0, {0, 1024}},
    {"ivf_bt", &Options::ivf_bt, 3, {0, 4, 16}},
    {"ivf_part", &Options::ivf_part, 0, {0, 1024}},                  // 0 (auto) or 1..1024 spans
    {"ivf_tps", &Options::ivf_tps, 3, {0, 16, 64}},                  // D > 128, next add: tiles per panel span (0 auto, 16 = 64-row bins, 64 = 256-row bins)
    {"ivf_tile", &Options::ivf_tile, 3, {0, 1, 2}},
    {"ivf_i8_group", &Options::ivf_i8_group, 2, {4, 8}},
    {"ivf_group", &Options::ivf_group, 4, {0, 1, 2, 4}},
    {"ivf_nw", &Options::ivf_nw, 4, {0, 2, 4, 8}},
};

// does a handle of `kind` refuse `value` of option r?  (vdb_set_option asks it of the handle's kind and the new value)
inline bool option_refused(const OptionRow &r, unsigned kind, double value) {
    return ((r.not_on & kind) && value != 0) || (kind == kPq && r.not_on_pq && value == r.not_on_pq);
}

// The same rule in the other order: `what` would make the handle a `kind`, and an option holds a value that kind refuses.  The
// kinds that need the resident float32 rows also refuse a value that took effect at the last add and was set back since (for
// the others rows of any sort are a state error of the call itself).
void refuse_options_set(const vdb_index_s *h, const char *what, unsigned kind) {
    for (const OptionRow &r : kOptions) {
        if (!r.m) continue;
        const bool in_effect = r.effect && h->*r.effect && (kind & kNeedsRows & r.not_on);
        if (option_refused(r, kind, h->opt.*r.m) || in_effect)
            throw Error(VDB_ERR_UNSUPPORTED, std::string(what) + ": option '" + r.name + "' = " + std::to_string(in_effect ? 1 : h->opt.*r.m) +
                                                 " is not available on " + kind_phrase(kind));
    }
}

template <class F>
void for_each_group(vdb_index_s *h, F &&f) { f(h->rows); f(h->scan); f(h->kept); f(h->lists); f(h->plan); f(h->codes); f(h->lsh_ws); f(h->knng_ws); f(h->ws); f(h->range); f(h->filter); f(h->ivf_filter); }

// every byte of device memory the handle holds (its ws.small may be a view into plan.ivf_zero: not counted twice)
size_t handle_bytes(vdb_index_s *h) {
    size_t s = 0;
    for_each_group(h, [&](auto &g) { s += group_bytes(g); });
    return s - (h->ws.small.borrowed ? h->ws.small.cap : 0);
}

void release_pins(vdb_index_s *h) {
    for (int i = 0; i < 2; ++i) {
        if (h->pin[i]) {
            alloc_note("HF", h->pin[i], h->pin_bytes);
            (void)hipHostFree(h->pin[i]);
        }
        h->pin[i] = nullptr;
    }
    h->pin_bytes = 0;
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Entry points run on the handle's GPU and leave the caller's current device as they found it.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) VDB_HIP(hipSetDevice(dev));
        else prev = -1;
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define set_device(dev) DeviceGuard device_guard__(dev)

constexpr size_t kMaxTimedCalls = 1024;

// returns the slot of this call, or -1 when timing is off / the ring is full
long timing_begin(vdb_index_s *h, hipStream_t st);
void timing_mark(vdb_index_s *h, long slot, int which, hipStream_t st);
void lsh_encode_rows(vdb_index_s *h, int64_t r0, hipStream_t st);     // lsh.inc: codes of the rows an add appended
void lsht_key_rows(vdb_index_s *h, int64_t r0, hipStream_t st);       // lsh_tables.inc: table keys of the rows an add appended
inline bool pq_on(const vdb_index_s *h) { return h->pq.M > 0; }
inline bool knng_on(const vdb_index_s *h) { return h->knng_degree > 0; }
void knng_drop(vdb_index_s *h);                                       // knng.inc: every add drops the graph
// an installed filter goes (filter.inc installs and uses it; an IVF-Flat handle's: ivf_filter.inc).  Its buffers may still be read
// by a search on a caller's stream.
void filter_drop(vdb_index_s *h) {
    if (group_bytes(h->filter) + group_bytes(h->ivf_filter) > 0) {
        set_device(h->device);
        (void)hipDeviceSynchronize();
        group_release(h->filter);
        group_release(h->ivf_filter);
    }
    h->filter_valid = h->filter_has_list = h->ivf_filter_valid = false;
    h->filter_count = h->ivf_filter_count = 0;
}
PqRows pq_rows(const vdb_index_s *h);                                                                       // pq.inc
void pq_decode_rows(vdb_index_s *h, int64_t r0, int64_t n, int64_t pitch, float *out, hipStream_t st);      // pq.inc: x^ of code rows
void launch_pq_panels(vdb_index_s *h, int64_t tile0, int64_t ntiles, half8 *panels, hipStream_t st);        // pq.inc: one slab of panels
bool pq_adc_fits(int M);                                                                                    // pq.inc: the ADC scan (pq_adc.hpp) serves this M
void launch_pq_adc_tables(vdb_index_s *h, const float *dq, int64_t nq, const QueryBatchInfo *info, float *tables, float *eps, hipStream_t st);
PqAdcScanArgs pq_adc_args(vdb_index_s *h, const float *tables, const QueryBatchInfo *info);
void launch_pq_adc_scan(vdb_index_s *h, PqAdcScanArgs &a, int64_t nq, hipStream_t st);
// Where the rows of a flat handle live, for the exact kernels: float32 rows, or (int8-only) int8 rows + their byte window, or
// (PQ) product codes that refine.hpp's pq_key looks x^ up from.  q: the batch's queries padded to D4.
inline RefineCommon flat_rows(const vdb_index_s *h, const float *q, int k) {
    RefineCommon c{(h->int8_only || pq_on(h)) ? nullptr : h->rows.x32.as<float>(), q, h->N, h->id_base, h->D4, h->metric, k, nullptr};
    if (pq_on(h)) c.pq = pq_rows(h);
    if (h->int8_only) {
        c.X8 = h->scan.rows8.as<signed char>();
        c.x8_pitch = h->rows8_pitch;
        c.cx = h->i8_cx;
    }
    return c;
}

int kpl_for(int k) {
    int kpl = 1;
    while (kpl * 64 < k) kpl *= 2;
    return kpl;
}

#define DISPATCH_KPL(kpl, ...)                                    \
    switch (kpl) {                                                \
        case 1: { constexpr int KPL = 1; __VA_ARGS__; } break;           \
        case 2: { constexpr int KPL = 2; __VA_ARGS__; } break;           \
        case 4: { constexpr int KPL = 4; __VA_ARGS__; } break;           \
        case 8: { constexpr int KPL = 8; __VA_ARGS__; } break;           \
        case 16: { constexpr int KPL = 16; __VA_ARGS__; } break;         \
        case 32: { constexpr int KPL = 32; __VA_ARGS__; } break;         \
        default: throw Error(VDB_ERR_UNSUPPORTED, "k too large"); \
    }

void launch_refine_full(const RefineFullArgs &a, int64_t max_units, hipStream_t st) {
    int64_t blocks = (max_units + 3) / 4;
    blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, 8192));
    const int kpl = kpl_for(a.c.k);
    DISPATCH_KPL(kpl, (refine_full_kernel<KPL><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a)));
    VDB_HIP(hipGetLastError());
}

// query-blocked exhaustive scan (4 queries per wave): max_units = ceil(count / 4) * S
constexpr int kRefineQB = 4;
void launch_refine_full_blocked(const RefineFullArgs &a, int64_t max_units, hipStream_t st) {
    int64_t blocks = (max_units + 3) / 4;
    blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, 8192));
    const bool pq = a.c.X == nullptr && a.c.pq.codes != nullptr;        // (a PQ index: the instantiation with the codes' accessor)
    if (kpl_for(a.c.k) == 1) {
        if (pq) refine_full_blocked_kernel<1, kRefineQB, true><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
        else refine_full_blocked_kernel<1, kRefineQB><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
    } else {
        if (pq) refine_full_blocked_kernel<2, kRefineQB, true><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
        else refine_full_blocked_kernel<2, kRefineQB><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
    }
    VDB_HIP(hipGetLastError());
}

void launch_merge(const MergeArgs &a, int64_t max_slots, hipStream_t st) {
    int64_t blocks = (max_slots + 3) / 4;
    blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, 4096));
    const int kpl = kpl_for(a.k);
    DISPATCH_KPL(kpl, (merge_kernel<KPL><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a)));
    VDB_HIP(hipGetLastError());
}

constexpr double kBinBudget = 6.0 * 1024.0 * 1024.0 * 1024.0;   // bytes of level-1 bin arrays per search pass
constexpr int64_t kDenseMaxRows = 15360;   // dense small-corpus path: one query's scores fit the default 64 KiB of LDS

// ---- row-block ingestion ---------------------------------------------------------------------------
// Host rows reach the device in blocks through TWO pinned staging buffers: block b is copied into pinned memory by
// host threads (this is where a memory-mapped corpus is paged in) while block b-1 is still in flight on the copy
// engine, so a 38 GB shard never has more than two blocks of host staging behind it -- the reference keeps its corpora
// as np.memmap for the same reason (src/benchmark/dataset.py:376-471, 1001-1052).  dst rows are D4 floats apart (D4 >=
// D, the tail must already be zero).
constexpr size_t kUploadBlockBytes = (size_t)64 << 20;

void parallel_memcpy(void *dst, const void *src, size_t bytes) {
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const size_t per = (bytes / hw + 4095) & ~(size_t)4095;
    if (bytes < ((size_t)8 << 20) || hw == 1) {
        memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> th;
    for (size_t off = per; off < bytes; off += per)
        th.emplace_back([=] { memcpy((char *)dst + off, (const char *)src + off, std::min(per, bytes - off)); });
    memcpy(dst, src, std::min(per, bytes));
    for (auto &t : th) t.join();
}

void upload_rows(vdb_index_s *h, float *dst, int D4, const float *src, int64_t n, int D, hipStream_t st) {
    h->last_upload_blocks = 0;
    if (n <= 0) return;
    const size_t row_bytes = (size_t)D * 4;
    const size_t block_bytes = h->opt.upload_block_mb > 0 ? (size_t)h->opt.upload_block_mb << 20 : kUploadBlockBytes;
    const int64_t rows_per_block = std::max<int64_t>(1, (int64_t)(block_bytes / row_bytes));
    const size_t need = (size_t)std::min<int64_t>(rows_per_block, n) * row_bytes;
    if (h->pin_bytes < need) {
        release_pins(h);
        if (hipHostMalloc(&h->pin[0], need, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc(&h->pin[1], need, hipHostMallocDefault) == hipSuccess) {
            h->pin_bytes = need;
            alloc_note("HA", h->pin[0], need);
            alloc_note("HA", h->pin[1], need);
        } else {                         // no pinned memory to be had: one pageable copy (the HIP runtime stages it itself)
            for (int i = 0; i < 2; ++i) {
                if (h->pin[i]) (void)hipHostFree(h->pin[i]);
                h->pin[i] = nullptr;
            }
            (void)hipGetLastError();
            VDB_HIP(hipMemcpy2DAsync(dst, (size_t)D4 * 4, src, row_bytes, row_bytes, (size_t)n, hipMemcpyHostToDevice, st));
            VDB_HIP(hipStreamSynchronize(st));
            h->last_upload_blocks = 1;
            return;
        }
    }
    for (int i = 0; i < 2; ++i)
        if (!h->pin_ev[i]) VDB_HIP(hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming));
    int64_t b = 0;
    for (int64_t r0 = 0; r0 < n; r0 += rows_per_block, ++b) {
        const int64_t rows = std::min<int64_t>(rows_per_block, n - r0);
        const int buf = (int)(b & 1);
        if (b >= 2) VDB_HIP(hipEventSynchronize(h->pin_ev[buf]));       // the copy that last used this buffer is done
        parallel_memcpy(h->pin[buf], src + (size_t)r0 * D, (size_t)rows * row_bytes);
        VDB_HIP(hipMemcpy2DAsync(dst + (size_t)r0 * D4, (size_t)D4 * 4, h->pin[buf], row_bytes, row_bytes, (size_t)rows,
                                 hipMemcpyHostToDevice, st));
        VDB_HIP(hipEventRecord(h->pin_ev[buf], st));
    }
    VDB_HIP(hipStreamSynchronize(st));
    h->last_upload_blocks = b;
}

// ---- index build ---------------------------------------------------------------------------------
// exact row norms + corpus statistics of h->rows.x32 (N rows) -> scales of the fp16 scan copy
void index_stats(vdb_index_s *h, hipStream_t st) {
    const int64_t n = h->N;
    h->rows.xnorm2.reserve((size_t)n * sizeof(float));
    h->kept.stats.reserve(sizeof(IndexStats));
    VDB_HIP(hipMemsetAsync(h->kept.stats.p, 0, sizeof(IndexStats), st));
    corpus_stats_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(h->rows.x32.as<float>(), n, h->D4,
                                                                                h->rows.xnorm2.as<float>(),
                                                                                h->kept.stats.as<IndexStats>());
    VDB_HIP(hipGetLastError());
    IndexStats hs;
    VDB_HIP(hipMemcpyAsync(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
    memcpy(&h->absmax, &hs.absmax_bits, 4);
    memcpy(&h->maxnorm2, &hs.maxnorm2_bits, 4);
    h->nonfinite = hs.nonfinite != 0;
    h->corpus_int_unscaled = !hs.not_integer && !h->nonfinite && h->absmax <= 2048.f;
    h->i8_cx = !hs.not_u8 ? 128 : 0;                        // u8 window first (SIFT), else s8
    h->i8_ok = !h->nonfinite && (!hs.not_u8 || !hs.not_s8) && h->dim <= 128;
    h->sx = 1.f;
    if (!h->corpus_int_unscaled && h->absmax > 0.f && !h->nonfinite) {
        int e;
        frexpf(h->absmax, &e);
        h->sx = ldexpf(1.f, 14 - e);  // absmax*sx in [8192, 16384)
    }
}

// row-major int8 copy of h->rows.x32 (byte-valued corpora only) for the list refine
void build_rows_i8(vdb_index_s *h, hipStream_t st) {
    h->rows8_pitch = h->i8_ks * 32;                        // = the pitch of the int8 query rows (64 or 128 bytes)
    h->scan.rows8.reserve((size_t)h->N * h->rows8_pitch);
    const int64_t words = h->N * (h->rows8_pitch / 4);
    build_rows_i8_kernel<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st>>>(
        h->rows.x32.as<float>(), h->N, h->dim, h->D4, h->rows8_pitch, h->i8_cx, h->scan.rows8.as<signed char>());
}

void graph_reset(vdb_index_s *h);

// layout "x16" for the scan copies of a D <= 128 flat index, unless an option asks for what only the 32-row kernels have
// (quads as the candidate group)
bool x16_wanted(const vdb_index_s *h) {
    return h->ksteps <= kMaxKSteps && h->opt.flat_shape != 32 && h->opt.f16_group == 8 && h->opt.i8_group == 8;
}

// everything derived from the h->N rows in h->rows.x32: statistics, scan copies, biases
void build_derived(vdb_index_s *h, hipStream_t st) {
    const int D = h->dim, D4 = h->D4;
    const int64_t n = h->N;
    // D > 128 (K-loop scan): p16 panels for v_mfma_f32_16x16x32_f16; D <= 128: 32-row tiles, in layout "x16" above the dense
    // path's rows (x16_wanted), else in the 32x32 form of scan_kernel and the dense path
    // (D > 128 with at most 2048 rows -- an IVF coarse quantizer over embeddings: 32-row tiles, served by the dense path's K-loop
    //  scores + register select instead of the float64 exhaustive kernel, search_flat.inc)
    constexpr int64_t kDenseRegRows = 2048;
    h->tile16 = h->ksteps > kMaxKSteps && n > kDenseRegRows;
    const int64_t span_rows = h->tile16 ? kSpanRows16 : kSpanRows;
    h->Npad = (n + span_rows - 1) / span_rows * span_rows;
    h->x16 = x16_wanted(h) && h->Npad > kDenseMaxRows;
    h->scan_ok = false;
    if (n == 0) {
        h->built = true;
        return;
    }
    index_stats(h, st);
    const bool dims_ok = D <= 4096;
    if (dims_ok && !h->nonfinite) {
        const int64_t ntiles = h->Npad / (h->tile16 ? kTileRows16 : kTileRows);
        const int ksl = h->tile16 ? h->ksteps / 2 : h->ksteps;          // k-steps of the layout (32 or 16 dims)
        h->panels_streamed = h->tile16 && h->opt.stream_panels != 0;
        if (h->panels_streamed) h->scan.panels.release();
        else h->scan.panels.reserve((size_t)ntiles * ksl * 64 * sizeof(half8));
        const int64_t threads = ntiles * ksl * 64;
        if (h->tile16)    // (streamed: the pass only takes the fp16-exactness flag)
            build_panels16_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(h->rows.x32.as<float>(), n, D, D4, ksl, ntiles, h->sx, h->panels_streamed ? nullptr : h->scan.panels.as<half8>(), h->kept.stats.as<IndexStats>());
        else
            build_panels_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(h->rows.x32.as<float>(), n, D, D4, h->ksteps, ntiles, h->sx, h->scan.panels.as<half8>(), h->kept.stats.as<IndexStats>(), h->x16 ? 1 : 0);
        VDB_HIP(hipGetLastError());
        h->scan.bias.reserve((size_t)h->Npad * sizeof(float));
        build_bias_kernel<<<dim3((unsigned)((h->Npad + 255) / 256)), dim3(256), 0, st>>>(h->rows.xnorm2.as<float>(), n, h->Npad, h->metric, h->scan.bias.as<float>());
        VDB_HIP(hipGetLastError());
        IndexStats hs;
        VDB_HIP(hipMemcpyAsync(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        h->corpus_fp16_exact = hs.not_fp16_exact == 0;
        h->scan_ok = true;
        h->i8_ok = h->i8_ok && !h->tile16;
        if (h->i8_ok) {
            h->i8_ks = D <= 64 ? 2 : 4;
            h->scan.panels8.reserve((size_t)ntiles * h->i8_ks * 64 * sizeof(int4v));
            const int64_t t8 = ntiles * h->i8_ks * 64;
            build_panels_i8_kernel<<<dim3((unsigned)((t8 + 255) / 256)), dim3(256), 0, st>>>(
                h->rows.x32.as<float>(), n, D, D4, h->i8_ks, ntiles, h->i8_cx, h->scan.panels8.as<int4v>(), 0, h->x16 ? 1 : 0);
            h->scan.bias8.reserve((size_t)2 * h->Npad * sizeof(int32_t));
            h->scan.rowstat8.reserve((size_t)n * 2 * sizeof(int));
            build_bias_i8_kernel<<<dim3((unsigned)((h->Npad + 255) / 256)), dim3(256), 0, st>>>(
                h->rows.x32.as<float>(), n, h->Npad, D, D4, h->metric, h->scan.bias8.as<int32_t>(), h->scan.rowstat8.as<int>());
            build_rows_i8(h, st);
            VDB_HIP(hipGetLastError());
            VDB_HIP(hipStreamSynchronize(st));
        }
    } else {
        h->i8_ok = false;
    }
    h->built = true;
}

// n rows from host or device memory to dst (device, D4 floats apart): rows [row0, row0 + n) of h->rows.x32, which already holds
// room for them, or a block of the int8-only build
void ingest_rows(vdb_index_s *h, float *dst, const float *x_dev_or_host, bool on_device, int64_t n, hipStream_t st) {
    const int D = h->dim, D4 = h->D4;
    if (D4 != D) VDB_HIP(hipMemsetAsync(dst, 0, (size_t)n * D4 * sizeof(float), st));
    if (on_device)
        VDB_HIP(hipMemcpy2DAsync(dst, (size_t)D4 * 4, x_dev_or_host, (size_t)D * 4, (size_t)D * 4, (size_t)n,
                                 hipMemcpyDeviceToDevice, st));
    else
        upload_rows(h, dst, D4, x_dev_or_host, n, D, st);
}

// ---- int8-only build (option "int8_only") ----------------------------------------------------------------------------------
// The float32 rows are never resident as a whole: they pass through in blocks (a window of the caller's device array when its
// rows are 16-byte multiples, else a padded / uploaded temporary of <= 4M rows), and every block leaves only its int8 rows, row
// statistics, int8 panels and accumulator inits behind.  The byte window (u8: x - 128, s8: x) is taken from the first block
// and checked on the flags of all of them; if the other window fits the whole corpus the build runs once more with it.
// Returns false when the corpus is not byte-valued (the caller then builds the default index).
constexpr int64_t kInt8OnlyMinRows = 32768;
bool build_int8_only(vdb_index_s *h, const float *x, bool on_device, int64_t n, hipStream_t st) {
    const int D = h->dim, D4 = h->D4;
    DevBuf *gone[] = {&h->rows.x32, &h->scan.panels, &h->scan.slab};      // (not a whole group: the int8 copies are about to be sized)
    for (auto b : gone) b->release();
    h->Npad = (n + kSpanRows - 1) / kSpanRows * kSpanRows;
    h->i8_ks = D <= 64 ? 2 : 4;
    h->x16 = x16_wanted(h);                 // (more than 32 768 rows: never the dense path's)
    h->rows8_pitch = h->i8_ks * 32;
    const int64_t ntiles = h->Npad / kTileRows;
    h->scan.rows8.reserve_exact((size_t)n * h->rows8_pitch);
    h->scan.rowstat8.reserve_exact((size_t)n * 2 * sizeof(int));
    h->rows.xnorm2.reserve((size_t)n * sizeof(float));
    h->kept.stats.reserve(sizeof(IndexStats));
    h->scan.bias8.reserve_exact((size_t)2 * h->Npad * sizeof(int32_t));
    h->scan.panels8.reserve_exact((size_t)ntiles * h->i8_ks * 64 * sizeof(int4v));
    h->scan.bias.reserve_exact((size_t)h->Npad * sizeof(float));
    const bool direct = on_device && D4 == D && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t block_want = h->opt.int8_block_rows > 0 ? ((int64_t)h->opt.int8_block_rows + kSpanRows - 1) / kSpanRows * kSpanRows : (int64_t)4 << 20;
    const int64_t block_rows = std::min<int64_t>((n + kSpanRows - 1) / kSpanRows * kSpanRows, block_want);
    DevBuf tmp;
    if (!direct) tmp.reserve((size_t)std::min<int64_t>(block_rows, n) * D4 * sizeof(float));
    IndexStats hs{};
    int cx = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        VDB_HIP(hipMemsetAsync(h->kept.stats.p, 0, sizeof(IndexStats), st));
        for (int64_t r0 = 0; r0 < n; r0 += block_rows) {
            const int64_t r1 = std::min<int64_t>(n, r0 + block_rows), nb = r1 - r0;
            const bool last = r1 == n;
            const float *blk;
            if (direct) {
                blk = x + (size_t)r0 * D;
            } else {
                ingest_rows(h, tmp.as<float>(), x + (size_t)r0 * D, on_device, nb, st);
                blk = tmp.as<float>();
            }
            corpus_stats_kernel<<<dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st>>>(blk, nb, D4, h->rows.xnorm2.as<float>() + r0,
                                                                                        h->kept.stats.as<IndexStats>());
            if (cx < 0) {           // the window: from the first block's flags
                VDB_HIP(hipMemcpyAsync(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
                VDB_HIP(hipStreamSynchronize(st));
                if (hs.nonfinite || (hs.not_u8 && hs.not_s8)) return false;
                cx = !hs.not_u8 ? 128 : 0;
            }
            const int64_t words = nb * (h->rows8_pitch / 4);
            build_rows_i8_kernel<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st>>>(
                blk, nb, D, D4, h->rows8_pitch, cx, h->scan.rows8.as<signed char>() + (size_t)r0 * h->rows8_pitch);
            // (panels and accumulator inits index rows globally: base pointer moved back by the rows in front of the block)
            const float *fake = blk - (size_t)r0 * D4;
            const int64_t row_end = last ? h->Npad : r1;
            const int64_t t0 = r0 / kTileRows, nt = (row_end - r0) / kTileRows;
            build_panels_i8_kernel<<<dim3((unsigned)((nt * h->i8_ks * 64 + 255) / 256)), dim3(256), 0, st>>>(
                fake, r1, D, D4, h->i8_ks, nt, cx, h->scan.panels8.as<int4v>(), t0, h->x16 ? 1 : 0);
            build_bias_i8_kernel<<<dim3((unsigned)((row_end - r0 + 255) / 256)), dim3(256), 0, st>>>(
                fake, r1, h->Npad, D, D4, h->metric, h->scan.bias8.as<int32_t>(), h->scan.rowstat8.as<int>(), r0, row_end);
            VDB_HIP(hipGetLastError());
            if (!direct) VDB_HIP(hipStreamSynchronize(st));     // (the temporary is refilled by the next block)
        }
        VDB_HIP(hipMemcpyAsync(&hs, h->kept.stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        if (hs.nonfinite) return false;
        const bool fits = cx == 128 ? !hs.not_u8 : !hs.not_s8;
        if (fits) break;
        const bool other = cx == 128 ? !hs.not_s8 : !hs.not_u8;
        if (!other || attempt == 1) return false;
        cx = cx == 128 ? 0 : 128;       // a later block left the first block's window but the whole corpus fits the other one
    }
    memcpy(&h->absmax, &hs.absmax_bits, 4);
    memcpy(&h->maxnorm2, &hs.maxnorm2_bits, 4);
    h->nonfinite = false;
    h->corpus_int_unscaled = true;      // integers 0..255 / -128..127: stored unscaled, exact in fp16
    h->corpus_fp16_exact = true;
    h->sx = 1.f;
    h->i8_cx = cx;
    h->i8_ok = true;
    h->tile16 = false;
    h->panels_streamed = false;
    build_bias_kernel<<<dim3((unsigned)((h->Npad + 255) / 256)), dim3(256), 0, st>>>(h->rows.xnorm2.as<float>(), n, h->Npad, h->metric,
                                                                                    h->scan.bias.as<float>());
    VDB_HIP(hipGetLastError());
    VDB_HIP(hipStreamSynchronize(st));
    h->rows.xnorm2.release();                // (the float norms only fed `bias`)
    h->int8_only = true;
    h->scan_ok = true;
    h->built = true;
    return true;
}

// the index holds exactly these n rows afterwards (whatever it held before)
void build_index(vdb_index_s *h, const float *x_dev_or_host, bool on_device, int64_t n, int64_t id_base,
                 hipStream_t st) {
    if (n < 0) throw Error(VDB_ERR_INVALID, "negative row count");
    graph_reset(h);
    if (n > 2147483647ll - 1024) throw Error(VDB_ERR_UNSUPPORTED, "more than 2^31 rows per shard");
    h->built = false;
    h->ivf_built = false;              // (rows filed by vdb_ivf_add sat in list order under a CSR that no longer describes x32)
    h->ivf_list_of_row.clear();
    h->N = n;
    h->id_base = id_base;
    h->int8_only = false;
    if (h->opt.int8_only && h->dim <= 128 && n > kInt8OnlyMinRows && !h->coarse) {
        bool ok = false;
        try {
            ok = build_int8_only(h, x_dev_or_host, on_device, n, st);
        } catch (...) {
            h->N = 0;
            h->built = false;
            h->scan_ok = false;
            h->int8_only = false;
            throw;
        }
        if (ok) return;
        h->int8_only = false;          // not byte-valued: the default layout (vdb_stats: has_i8_copy says which one it is)
        DevBuf *i8[] = {&h->scan.rows8, &h->scan.rowstat8, &h->scan.bias8, &h->scan.panels8};   // (not the whole scan group: the bias stays, as it did)
        for (auto b : i8) b->release();
    }
    try {
        if (n > 0) {
            h->rows.x32.reserve((size_t)n * h->D4 * sizeof(float));
            ingest_rows(h, h->rows.x32.as<float>(), x_dev_or_host, on_device, n, st);
        }
        build_derived(h, st);
    } catch (...) {                    // a failed build leaves an EMPTY index (the next add starts over; a search says "not built")
        h->N = 0;
        h->built = false;
        h->scan_ok = false;
        throw;
    }
}

void require_same_id_base(const vdb_index_s *h, int64_t id_base) {
    if (id_base != h->id_base)
        throw Error(VDB_ERR_INVALID, "add appends to the " + std::to_string(h->N) + " rows of this index, whose id base is " +
                                         std::to_string(h->id_base) + " (row i of the index has id base + i): pass the same "
                                         "id_base, or call vdb_reset first; got " + std::to_string(id_base));
}

// what an add refuses from its arguments and the handle's state alone, before it touches the handle (add_rows runs it ahead of
// everything an add drops: a refused add changes nothing)
void refuse_bad_add(const vdb_index_s *h, int64_t n, int64_t id_base) {
    if (n < 0) throw Error(VDB_ERR_INVALID, "negative row count");
    if (h->N == 0 || h->ivf_built) {      // (the add replaces the rows: build_index)
        if (n > 2147483647ll - 1024) throw Error(VDB_ERR_UNSUPPORTED, "more than 2^31 rows per shard");
        return;
    }
    require_same_id_base(h, id_base);
    if (n == 0) return;
    if (h->int8_only)
        throw Error(VDB_ERR_UNSUPPORTED, "an int8_only index keeps no float32 rows to re-derive its scan copies from: it is built by "
                                         "ONE add (vdb_reset, then add everything)");
    if (h->N + n > 2147483647ll - 1024) throw Error(VDB_ERR_UNSUPPORTED, "more than 2^31 rows per shard");
}

// vdb_add / vdb_add_device: APPEND, as faiss.Index.add does (the first add of an empty index is build_index)
void append_rows(vdb_index_s *h, const float *x_dev_or_host, bool on_device, int64_t n, int64_t id_base, hipStream_t st) {
    refuse_bad_add(h, n, id_base);
    if (h->N == 0 || h->ivf_built) {      // (rows filed by vdb_ivf_add are replaced: they sit in list order, not insertion order)
        build_index(h, x_dev_or_host, on_device, n, id_base, st);
        return;
    }
    if (n == 0) return;
    graph_reset(h);
    VDB_HIP(hipDeviceSynchronize());                        // (searches of the rows about to move may still run)
    const int64_t N0 = h->N;
    // the scan copies are re-derived from the float32 rows anyway: free them first, so that the peak is old rows + grown rows
    // (not that plus the copies), and on failure rebuild them from the old rows -- the append is atomic (N, ids and results
    // as before the call)
    group_release(h->scan);
    h->built = false;
    try {
        h->rows.x32.grow((size_t)(N0 + n) * h->D4 * sizeof(float), (size_t)N0 * h->D4 * sizeof(float));
        ingest_rows(h, h->rows.x32.as<float>() + (size_t)N0 * h->D4, x_dev_or_host, on_device, n, st);
    } catch (...) {
        (void)hipGetLastError();
        h->N = N0;
        try {
            build_derived(h, st);
        } catch (...) {                // not even the old copies fit any more: the index is emptied, loudly
            h->N = 0;
            h->built = false;
            h->scan_ok = false;
        }
        throw;
    }
    h->N = N0 + n;
    build_derived(h, st);                                   // (scan copies are rebuilt from the float32 rows: 0.3 s per 12.5M x 768)
}

#include "search_flat.inc"   // scan geometry, launchers, search_batch, graph replay, search_device_impl

// A host-API call: the queries go up through the staging buffers of the workspace, `run(dq, dD, dI, st)` works on the device
// copies, (D, I) come back, and the call returns when they have -- all on the null stream.
template <class F>
void run_staged(vdb_index_s *h, const float *q_host, int64_t nq, int k, float *D, int64_t *I, F &&run) {
    Workspace &ws = h->ws;
    ws.stage_q.reserve((size_t)nq * h->dim * sizeof(float));
    ws.stage_d.reserve((size_t)nq * k * sizeof(float));
    ws.stage_i.reserve((size_t)nq * k * sizeof(int64_t));
    hipStream_t st = nullptr;
    VDB_HIP(hipMemcpyAsync(ws.stage_q.p, q_host, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
    run(ws.stage_q.as<float>(), ws.stage_d.as<float>(), ws.stage_i.as<int64_t>(), st);
    VDB_HIP(hipMemcpyAsync(D, ws.stage_d.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    VDB_HIP(hipMemcpyAsync(I, ws.stage_i.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
}

template <class F>
int guarded(F &&f) {
    try {
        f();
        return VDB_OK;
    } catch (const Error &e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return VDB_ERR_INVALID;
    } catch (...) {
        g_last_error = "unknown error";
        return VDB_ERR_INVALID;
    }
}

vdb_index_s *check(vdb_handle h) {
    if (!h) throw Error(VDB_ERR_INVALID, "null handle");
    return h;
}

// multi-device handles (multi.inc)
void multi_destroy(vdb_index_s *m);
void multi_reset(vdb_index_s *m);
void multi_add(vdb_index_s *m, const float *x, bool on_device, int64_t n, int64_t id_base, hipStream_t user_stream, bool ivf,
               const int32_t *given);
void multi_search(vdb_index_s *m, const float *q, bool device_api, int64_t nq, int k, float *D, int64_t *I, double *PK,
                  int64_t *PI, hipStream_t user_stream, bool ivf);
void multi_reserve(vdb_index_s *m, int64_t nq, int k);
void multi_stats(vdb_index_s *m, vdb_stats_t *out);
void multi_set_option(vdb_index_s *m, const char *key, double value);
void multi_set_centroids(vdb_index_s *m, const float *c_host, int nlist);
void multi_train(vdb_index_s *m, int nlist, const float *x_host, int64_t n, int niter, uint64_t seed, int mppc);
void multi_get_assignment(vdb_index_s *m, int32_t *out);
void multi_rerank(vdb_index_s *m, const float *q, bool device_api, int64_t nq, const int64_t *cand, int ncand, int k, float *D,
                  int64_t *I, hipStream_t user_stream);
vdb_index_s *multi_first_shard(vdb_index_s *m);
void multi_for_each_shard(vdb_index_s *m, const std::function<void(vdb_index_s *)> &f);

// ns of the rows 0 .. n-1 (ns <= n) without replacement, in draw order, as the first ns entries of the result: seeded partial
// Fisher-Yates (the training samples of vdb_ivf_train and vdb_pq_train)
std::vector<int64_t> sample_rows(int64_t n, int64_t ns, uint64_t seed) {
    std::vector<int64_t> pick((size_t)n);
    std::iota(pick.begin(), pick.end(), (int64_t)0);
    std::mt19937_64 rng(seed);
    for (int64_t i = 0; i < std::min<int64_t>(ns, n - 1); ++i) {
        const int64_t j = i + (int64_t)(rng() % (uint64_t)(n - i));
        std::swap(pick[(size_t)i], pick[(size_t)j]);
    }
    return pick;
}

// vdb_add (host rows, null stream) and vdb_add_device (device rows, the caller's stream)
void add_rows(vdb_index_s *h, const char *what, const float *x, bool on_device, int64_t n, int64_t id_base, hipStream_t st) {
    admit(h, what, kAnyKind & ~(kPq | kIvfSq8 | kIvfPq | kIvfI8));      // (those hold their rows as codes: vdb_pq_add, vdb_ivf_add)
    if (n > 0 && !x) throw Error(VDB_ERR_INVALID, "null corpus pointer");
    if (h->multi) return multi_add(h, x, on_device, n, id_base, st, false, nullptr);
    refuse_bad_add(h, n, id_base);             // (a refused add changes nothing: the range result and the filter stay)
    set_device(h->device);
    h->range_valid = false;                    // (the last range result described the rows as they were)
    filter_drop(h);                            // (... and so did an installed filter: one bit per row, nbits == ntotal)
    if (knng_on(h)) {                          // (the graph describes the rows as they were)
        VDB_HIP(hipDeviceSynchronize());
        knng_drop(h);
    }
    const int64_t n0 = (h->N == 0 || h->ivf_built) ? 0 : h->N;
    append_rows(h, x, on_device, n, id_base, st);
    lsh_encode_rows(h, n0, st);
    lsht_key_rows(h, n0, st);
}

// vdb_merge_partials_device (keys and ids in two arrays, parts nq * k apart) and vdb_merge_packed_partials_device (one array of
// [keys | ids] blocks per part): `stride` = elements between the parts
void merge_partials(int metric, int device, const double *keys_dev, const int64_t *ids_dev, int64_t stride, int nparts, int64_t nq,
                    int k, float *D_dev, int64_t *I_dev, hipStream_t st) {
    if (metric != VDB_METRIC_L2 && metric != VDB_METRIC_IP) throw Error(VDB_ERR_INVALID, "unknown metric");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (nparts < 0 || nq < 0) throw Error(VDB_ERR_INVALID, "negative size");
    if (nq == 0) return;
    if (!D_dev || !I_dev || (nparts > 0 && (!keys_dev || !ids_dev))) throw Error(VDB_ERR_INVALID, "null pointer");
    set_device(device);
    MergeArgs ma{};
    ma.pkeys = keys_dev;
    ma.pids = ids_dev;
    ma.part_stride = stride;
    ma.slot_stride = k;
    ma.nparts = nparts;
    ma.k = k;
    ma.metric = metric;
    ma.count = nq;
    ma.D = D_dev;
    ma.I = I_dev;
    launch_merge(ma, nq, st);
}

}  // namespace

// =====================================================================================================
extern "C" {

int vdb_abi_version(void) { return VDB_ABI_VERSION; }

const char *vdb_last_error(void) { return g_last_error.c_str(); }

int vdb_device_count(int *count) {
    return guarded([&] {
        if (!count) throw Error(VDB_ERR_INVALID, "null pointer");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) n = 0;
        *count = n;
    });
}

int vdb_create(int dim, int metric, int device, vdb_handle *out) {
    return guarded([&] {
        if (!out) throw Error(VDB_ERR_INVALID, "null output handle");
        if (dim < 1 || dim > 65536) throw Error(VDB_ERR_INVALID, "dimension must be in [1, 65536]");
        if (metric != VDB_METRIC_L2 && metric != VDB_METRIC_IP) throw Error(VDB_ERR_INVALID, "unknown metric");
        int n = 0;
        VDB_HIP(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) throw Error(VDB_ERR_INVALID, "no such GPU: " + std::to_string(device));
        set_device(device);
        hipDeviceProp_t prop;
        VDB_HIP(hipGetDeviceProperties(&prop, device));
        if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
            throw Error(VDB_ERR_UNSUPPORTED, std::string("libvdbhip is built for gfx950 (MI355X); found ") +
                                                 prop.gcnArchName);
        auto *h = new vdb_index_s();
        h->device = device;
        h->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        h->dim = dim;
        h->D4 = (dim + 3) / 4 * 4;
        h->ksteps = dim <= 64 ? 4 : (dim <= 128 ? 8 : (dim + 63) / 64 * 4);  // D > 128: K-loop kernel, 64-dim steps
        h->metric = metric;
        *out = h;
    });
}

int vdb_destroy(vdb_handle h) {
    return guarded([&] {
        if (!h) return;
        if (h->multi) {
            multi_destroy(h);
            delete h;
            return;
        }
        set_device(h->device);
        (void)hipDeviceSynchronize();
        graph_reset(h);
        if (h->coarse) (void)vdb_destroy(h->coarse);
        delete h;
    });
}

int vdb_add(vdb_handle hh, const float *x_host, int64_t n, int64_t id_base) {
    return guarded([&] { add_rows(check(hh), "vdb_add", x_host, false, n, id_base, nullptr); });
}

int vdb_reset(vdb_handle hh) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_reset", kAnyKind);
        if (h->multi) return multi_reset(h);
        set_device(h->device);
        VDB_HIP(hipDeviceSynchronize());
        graph_reset(h);
        h->N = 0;
        h->built = false;
        h->scan_ok = false;
        h->ivf_built = false;
        h->int8_only = false;
        h->ivf_list_of_row.clear();
        h->ivf_offsets_host.clear();
        // faiss.Index.reset frees its storage: so do we (rows, scan copies, CSR arrays; the workspace and an IVF index's
        // centroids stay) -- a caller that resets a 38 GB shard to load another corpus gets the memory back
        group_release(h->rows);
        group_release(h->scan);
        group_release(h->lists);
        group_release(h->codes);
        group_release(h->range);
        h->range_valid = false;
        filter_drop(h);
        h->lsh_rows = 0;                       // (the projection stays)
        h->lsht_rows = 0;                      // (the hash tables stay)
        h->knng_degree = 0;                    // (the graph went with the codes group)
    });
}

int vdb_add_device(vdb_handle hh, const float *x_dev, int64_t n, int64_t id_base, void *stream) {
    return guarded([&] { add_rows(check(hh), "vdb_add_device", x_dev, true, n, id_base, as_stream(stream)); });
}

int vdb_search(vdb_handle hh, const float *q_host, int64_t nq, int k, float *D, int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_search", kAnyKind);
        if (!h->built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
        if (nq > 0 && (!q_host || !D || !I)) throw Error(VDB_ERR_INVALID, "null pointer");
        if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
        if (nq <= 0) {
            if (nq < 0) throw Error(VDB_ERR_INVALID, "negative query count");
            return;
        }
        if (h->multi) return multi_search(h, q_host, false, nq, k, D, I, nullptr, nullptr, nullptr, false);
        set_device(h->device);
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            search_device_impl(h, dq, nq, k, dD, dI, nullptr, nullptr, st);
        });
    });
}

int vdb_search_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                      void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_search_device", kAnyKind);
        if (nq > 0 && (!D_dev || !I_dev)) throw Error(VDB_ERR_INVALID, "null output pointer");
        if (h->multi) return multi_search(h, q_dev, true, nq, k, D_dev, I_dev, nullptr, nullptr, as_stream(stream), false);
        set_device(h->device);
        vdb_index_s::GraphKey key;
        key.q = q_dev; key.o1 = D_dev; key.o2 = I_dev; key.nq = nq; key.k = k; key.kind = 1; key.st = as_stream(stream);
        graph_or_run(h, key, [&] { search_device_impl(h, q_dev, nq, k, D_dev, I_dev, nullptr, nullptr, as_stream(stream)); });
    });
}

int vdb_search_partial_device(vdb_handle hh, const float *q_dev, int64_t nq, int k, double *keys_dev,
                              int64_t *ids_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_search_partial_device", kAnyKind);
        if (nq > 0 && (!keys_dev || !ids_dev)) throw Error(VDB_ERR_INVALID, "null output pointer");
        if (h->multi) return multi_search(h, q_dev, true, nq, k, nullptr, nullptr, keys_dev, ids_dev, as_stream(stream), false);
        set_device(h->device);
        vdb_index_s::GraphKey key;
        key.q = q_dev; key.o1 = keys_dev; key.o2 = ids_dev; key.nq = nq; key.k = k; key.kind = 2; key.st = as_stream(stream);
        graph_or_run(h, key, [&] { search_device_impl(h, q_dev, nq, k, nullptr, nullptr, keys_dev, ids_dev, as_stream(stream)); });
    });
}

int vdb_merge_partials_device(int metric, int device, const double *keys_dev, const int64_t *ids_dev, int nparts,
                              int64_t nq, int k, float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] { merge_partials(metric, device, keys_dev, ids_dev, nq * k, nparts, nq, k, D_dev, I_dev, as_stream(stream)); });
}

int vdb_merge_packed_partials_device(int metric, int device, const void *packed_dev, int nparts, int64_t nq, int k,
                                     float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        const double *keys = reinterpret_cast<const double *>(packed_dev);
        const int64_t *ids = packed_dev ? reinterpret_cast<const int64_t *>(packed_dev) + nq * k : nullptr;
        merge_partials(metric, device, keys, ids, 2 * nq * k, nparts, nq, k, D_dev, I_dev, as_stream(stream));
    });
}

namespace {
// (pk / pi: partial rows -- float64 keys + ids -- instead of (D, I); segs / nseg: a shard of a multi-device index, see RerankArgs)
void rerank_device_impl(vdb_index_s *h, const float *dq, int64_t nq, const int64_t *cand, int ncand, int k, float *D,
                        int64_t *I, hipStream_t st, double *pk = nullptr, int64_t *pi = nullptr, const int64_t *segs = nullptr,
                        int nseg = 0) {
    if (!h->built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
    if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
    if (nq < 0 || ncand < 0) throw Error(VDB_ERR_INVALID, "negative size");
    if (nq == 0) return;
    if (!dq || (pk ? !pi : (!D || !I)) || (ncand > 0 && !cand)) throw Error(VDB_ERR_INVALID, "null pointer");
    const float *qpad = dq;
    if (h->D4 != h->dim) {
        h->ws.qpad.reserve((size_t)nq * h->D4 * sizeof(float));
        pad_rows_kernel<<<dim3((unsigned)((nq * h->D4 + 255) / 256)), dim3(256), 0, st>>>(dq, nq, h->dim, h->D4,
                                                                                        h->ws.qpad.as<float>());
        qpad = h->ws.qpad.as<float>();
    }
    RerankArgs a{};
    a.c = flat_rows(h, qpad, k);
    a.nq = nq;
    a.cand = cand;
    a.ncand = ncand;
    a.D = pk ? nullptr : D;
    a.I = pk ? nullptr : I;
    a.pkeys = pk;
    a.pids = pi;
    a.segs = segs;
    a.nseg = nseg;
    const int kpl = kpl_for(k);
    DISPATCH_KPL(kpl, (rerank_kernel<KPL><<<dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st>>>(a)));
    VDB_HIP(hipGetLastError());
}
}  // namespace

int vdb_rerank_device(vdb_handle hh, const float *q_dev, int64_t nq, const int64_t *cand_dev, int ncand, int k,
                      float *D_dev, int64_t *I_dev, void *stream) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_rerank_device", kAnyKind & ~kIvfPq, VDB_ERR_STATE);
        if (h->multi) return multi_rerank(h, q_dev, true, nq, cand_dev, ncand, k, D_dev, I_dev, as_stream(stream));
        set_device(h->device);
        rerank_device_impl(h, q_dev, nq, cand_dev, ncand, k, D_dev, I_dev, as_stream(stream));
    });
}

int vdb_rerank(vdb_handle hh, const float *q_host, int64_t nq, const int64_t *cand_host, int ncand, int k, float *D,
               int64_t *I) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_rerank", kAnyKind & ~kIvfPq, VDB_ERR_STATE);       // (the other IVF kinds answer "not built" below: same code)
        if (h->multi) return multi_rerank(h, q_host, false, nq, cand_host, ncand, k, D, I, nullptr);
        if (!h->built) throw Error(VDB_ERR_STATE, "Index has not been built yet.");
        if (nq <= 0) {
            if (nq < 0) throw Error(VDB_ERR_INVALID, "negative query count");
            return;
        }
        if (!q_host || !D || !I || (ncand > 0 && !cand_host) || ncand < 0) throw Error(VDB_ERR_INVALID, "bad argument");
        if (k < 1 || k > 2048) throw Error(VDB_ERR_INVALID, "k must be in [1, 2048]");
        set_device(h->device);
        DevBuf dc;                             // the candidate ids (freed when the call returns, results copied back)
        run_staged(h, q_host, nq, k, D, I, [&](const float *dq, float *dD, int64_t *dI, hipStream_t st) {
            dc.reserve((size_t)nq * std::max(ncand, 1) * sizeof(int64_t));
            if (ncand > 0)
                VDB_HIP(hipMemcpyAsync(dc.p, cand_host, (size_t)nq * ncand * sizeof(int64_t), hipMemcpyHostToDevice, st));
            rerank_device_impl(h, dq, nq, dc.as<int64_t>(), ncand, k, dD, dI, st);
        });
    });
}

int vdb_stats(vdb_handle hh, vdb_stats_t *out) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_stats", kAnyKind);
        if (!out) throw Error(VDB_ERR_INVALID, "null pointer");
        if (h->multi) return multi_stats(h, out);
        set_device(h->device);
        vdb_stats_t s = h->last;
        s.ndevices = 1;
        s.scan_shape = (!h->scan_ok || h->ksteps > kMaxKSteps || h->N == 0) ? 0 : h->x16 ? 16 : 32;
        s.ntotal = h->N;
        s.dim = h->dim;
        s.metric = h->metric;
        s.corpus_fp16_exact = h->corpus_fp16_exact ? 1 : 0;
        // everything the handle holds, and an IVF index's coarse quantizer (its own index and workspace) with it
        s.bytes_resident = (int64_t)(handle_bytes(h) + (h->coarse ? handle_bytes(h->coarse) : 0));
        s.has_i8_copy = (h->int8_only || h->ivf_codec == 3) ? 2 : (h->i8_ok ? 1 : 0);      // (IVF-I8: nothing but the int8 copies)
        s.bytes_workspace = (int64_t)(group_bytes(h->ws) + group_bytes(h->lsh_ws) + group_bytes(h->knng_ws) + group_bytes(h->range) + (pq_on(h) ? h->scan.slab.cap : 0));   // (PQ: + the slab of per-search panels)
        s.upload_blocks = h->last_upload_blocks;
        s.graph_replays = h->graph_replays;
        s.last_rows_scanned = 0;
        // the last search ran an MFMA scan (flat, or the list-major one of an IVF index): ws.small holds its choice and its counters
        const bool mfma_scanned = h->last.last_path == VDB_PATH_MFMA_SCAN || h->last.last_path == VDB_PATH_PQ_ADC || h->last.last_path == VDB_PATH_IVFPQ_ADC ||
                                  (h->last.last_path == VDB_PATH_IVF && h->ivf_last_mfma);
        if (h->last.last_path == VDB_PATH_IVF && h->ivf_last_mfma && h->plan.ivf_plan.p) {   // (of the last batch of the call)
            IvfPlan pl;
            VDB_HIP(hipDeviceSynchronize());
            VDB_HIP(hipMemcpy(&pl, h->plan.ivf_plan.p, sizeof(pl), hipMemcpyDeviceToHost));
            s.last_rows_scanned = (int64_t)pl.rows_scanned;
        }
        s.scan_dtype = 0;
        if (h->i8_ok && h->ws.small.p && mfma_scanned) {   // which scan the device chose
            QueryBatchInfo qi;
            VDB_HIP(hipDeviceSynchronize());
            VDB_HIP(hipMemcpy(&qi, batch_info(h->ws), sizeof(qi), hipMemcpyDeviceToHost));
            s.scan_dtype = qi.i8_mode ? 1 : 0;
        }
        if (h->ivf_codec != 0 && h->last.last_path == VDB_PATH_IVF && h->ivf_last_mfma && !(h->ivf_codec == 3 && s.scan_dtype == 1)) s.scan_dtype = 2;   // fp16 from 8-bit (product) codes, or from the int8 panels of IVF-I8 (whose integer batches take the int8 scan: 1)
        if (pq_on(h) && h->last.last_path == VDB_PATH_MFMA_SCAN) s.scan_dtype = 2;                          // ... of a PQ index
        if (h->last.last_path == VDB_PATH_PQ_ADC || h->last.last_path == VDB_PATH_IVFPQ_ADC) s.scan_dtype = 3;   // float32 lookup-table sums (PQ / IVF-PQ, ADC scan)
        s.nlist = h->nlist;
        s.nprobe = h->nprobe;
        s.last_candidates = s.last_rescan_bins = s.last_fallback_queries = 0;
        s.last_scan_ms = s.last_total_ms = s.last_prep_ms = s.last_tail_ms = 0.f;
        if (h->ws.small.p && mfma_scanned) {
            std::vector<unsigned char> buf(kSmallBytes);
            VDB_HIP(hipDeviceSynchronize());
            VDB_HIP(hipMemcpy(buf.data(), h->ws.small.p, kSmallBytes, hipMemcpyDeviceToHost));
            int32_t fb;
            unsigned long long c[3] = {0, 0, 0};
            memcpy(&fb, buf.data(), 4);
            for (int sh = 0; sh < kStatShards; ++sh) {          // sharded counters (common.hpp, stat_add)
                unsigned long long v[3];
                memcpy(v, buf.data() + 64 + (size_t)sh * kStatStride * 8, 24);
                c[0] += v[0];
                c[1] += v[1];
                c[2] += v[2];
            }
            fb = (int32_t)c[2];        // (counter 2 accumulates over the batches of a call; fb_count restarts per batch)
            s.last_fallback_queries = fb;
            s.last_candidates = (int64_t)c[0];
            s.last_rescan_bins = (int64_t)c[1];
        }
        // last LSH call: queries that took the exact fallback of the select; hash tables also report candidates and brute-force queries
        if ((h->last.last_path == VDB_PATH_LSH || h->last.last_path == VDB_PATH_LSHT) && h->lsh_ws.lsh_stat.p) {
            const bool tables = h->last.last_path == VDB_PATH_LSHT;
            std::vector<unsigned long long> c((size_t)kStatShards * kStatStride);
            VDB_HIP(hipDeviceSynchronize());
            VDB_HIP(hipMemcpy(c.data(), h->lsh_ws.lsh_stat.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int sh = 0; sh < kStatShards; ++sh) {
                s.last_fallback_queries += (int64_t)c[(size_t)sh * kStatStride];
                if (tables) s.last_candidates += (int64_t)c[(size_t)sh * kStatStride + 1];
                if (tables) s.last_rows_scanned += h->N * (int64_t)c[(size_t)sh * kStatStride + 2];
            }
        }
        if (h->last.last_path == VDB_PATH_KNNG && h->knng_ws.knng_stat.p) {   // rows scored / queries the step cap stopped, last k-NN graph search
            std::vector<unsigned long long> c((size_t)kStatShards * kStatStride);
            VDB_HIP(hipDeviceSynchronize());
            VDB_HIP(hipMemcpy(c.data(), h->knng_ws.knng_stat.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int sh = 0; sh < kStatShards; ++sh) {
                s.last_candidates += (int64_t)c[(size_t)sh * kStatStride];
                s.last_fallback_queries += (int64_t)c[(size_t)sh * kStatStride + 1];
            }
        }
        if (h->last.last_path == VDB_PATH_RANGE || h->last.last_path == VDB_PATH_IVF_RANGE) {     // (the call read its counters back when it sized the result)
            s.last_candidates = h->range_cand;
            s.last_fallback_queries = h->range_fb;
        }
        if (h->last.last_path == VDB_PATH_FILTER_ROWS) s.last_candidates = h->filter_cand;     // (sparse route: nq x admitted rows)
        if (h->ev_used > 0) {  // averages over every search recorded since timing was switched on
            double scan = 0.0, total = 0.0, prep = 0.0, tail = 0.0;
            for (size_t i = 0; i < h->ev_used; ++i) {
                float ms = 0.f;
                VDB_HIP(hipEventSynchronize(h->ev_total[2 * i + 1]));
                VDB_HIP(hipEventElapsedTime(&ms, h->ev_scan[2 * i], h->ev_scan[2 * i + 1]));
                scan += ms;
                VDB_HIP(hipEventElapsedTime(&ms, h->ev_total[2 * i], h->ev_total[2 * i + 1]));
                total += ms;
                VDB_HIP(hipEventElapsedTime(&ms, h->ev_total[2 * i], h->ev_scan[2 * i]));
                prep += ms;
                VDB_HIP(hipEventElapsedTime(&ms, h->ev_scan[2 * i + 1], h->ev_total[2 * i + 1]));
                tail += ms;
            }
            s.last_scan_ms = (float)(scan / h->ev_used);
            s.last_total_ms = (float)(total / h->ev_used);
            s.last_prep_ms = (float)(prep / h->ev_used);
            s.last_tail_ms = (float)(tail / h->ev_used);
        }
        *out = s;
    });
}

int vdb_set_option(vdb_handle hh, const char *key, double value) {
    return guarded([&] {
        auto *h = check(hh);
        admit(h, "vdb_set_option", kAnyKind);
        if (!key) throw Error(VDB_ERR_INVALID, "null option name");
        if (h->multi) return multi_set_option(h, key, value);
        const std::string k(key);
        graph_reset(h);                        // (a captured search embodies the options it was captured under)
        h->range_valid = false;                // (... and the last range result goes with any option change)
        filter_drop(h);                        // (... and an installed filter: its list was built under the options in force)
        const OptionRow *r = std::find_if(std::begin(kOptions), std::end(kOptions), [&](const OptionRow &o) { return k == o.name; });
        if (r == std::end(kOptions)) throw Error(VDB_ERR_INVALID, "unknown option '" + k + "'");
        // what this kind of index refuses comes first, whatever the value is otherwise
        if (option_refused(*r, kind_of(h), value))
            throw Error(VDB_ERR_UNSUPPORTED, "option '" + k + "' = " + std::to_string((int)value) + " is not available on " + kind_phrase(kind_of(h)));
        auto number = [](double v) { return v == HUGE_VAL ? std::string("inf") : std::to_string((long)v); };
        if (r->n > 0 && std::find(r->v, r->v + r->n, value) == r->v + r->n) {
            std::string list = number(r->v[0]);
            for (int i = 1; i < r->n; ++i) list += ", " + number(r->v[i]);
            throw Error(VDB_ERR_INVALID, "option '" + k + "' must be one of " + std::move(list));
        }
        if (r->n == 0 && (value < r->v[0] || value > r->v[1]))
            throw Error(VDB_ERR_INVALID, "option '" + k + "' must be in [" + number(r->v[0]) + ", " + number(r->v[1]) + "]");
        if (r->m == &Options::ivfpq_adc_part_rows && (int)value % 256 != 0) throw Error(VDB_ERR_INVALID, "option '" + k + "' must be a multiple of 256");
        if (r->m64) h->opt.*r->m64 = value >= 9.0e18 ? (int64_t)9000000000000000000ll : (int64_t)value;      // (the int64 options take "inf": "stream_slab_rows" too, whose cast of inf was undefined before)
        else h->opt.*r->m = r->n < 0 ? value != 0 : (int)value;
        if (r->m == &Options::timing) h->ev_used = 0;          // (a new recording window)
    });
}

}  // extern "C"

#include "pq.inc"
#include "lsh.inc"
#include "lsh_tables.inc"
#include "knng.inc"
#include "range.inc"
#include "filter.inc"
#include "debug_ivf.inc"
#include "ivf_filter.inc"      // (behind ivf.inc, which debug_ivf.inc ends with)
#include "ivf_range.inc"       // (likewise)
#include "multi.inc"

// scan_plan.hpp -- where the path and the launch shape of a flat scan are decided: plain host C++ (no HIP header, no handle),
// so the rules compile with an ordinary host compiler and tests/host/scan_plan_main.cpp prints what they give.
//   constants of the scan geometry | Options (what vdb_set_option writes) | ScanIndexShape (what the rules read of a handle)
//   scan_geometry / scan_geometry_direct | nw_small, use_i8, pair_candidate, f16_octs, st_tiles_of
//   plan_f16 / plan_i8 / plan_pair -> ScanLaunch: kernel family, template arguments, grid, block
//   VDB_KERNELS_*: every instantiation of a family, once -- the keys the host program walks and (search_flat.inc) the table
//   of kernel pointers `launch` looks a plan up in
#pragma once
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "filter_plan.hpp"      // kFilterSparsePairsDefault

namespace vdb {

// ---- geometry constants of the scan copies (row mapping: common.hpp) ------------------------------------------------------
constexpr int kSpanRows = 512;      // 16 tiles; two bins (h = 0,1) of 256 rows
constexpr int kBinRows = 256;
constexpr int kTilesPerSpan = 16;
// layout "p16" (16-row tiles for v_mfma_f32_16x16x32_f16): span = 64 tiles = 1024 rows = four 256-row bins, one
// per lane group g = lane>>4 of the 16x16 C/D layout
constexpr int kSpanRows16 = 1024;
constexpr int kTilesPerSpan16 = 64;
constexpr int kMaxKSteps = 8;       // register-resident query fragments: D <= 128
constexpr int kNarrowMaxKS = 48;    // 32-dim k-steps of the LDS-resident query block of scan16_kloop_kernel (D <= 1536)
// PQ index (pq.inc): rows per slab of per-search panels (measured, profiles/r07_bench_pq.json)
constexpr int64_t kPqSlabRows = 524288;

// ---- options -----------------------------------------------------------------------------------------------------------------
// Everything vdb_set_option writes and nothing else: one member per option, under the name the caller passes, holding the
// value the caller passed; the initializer is the value of an option never set.  What the library derives from an option at
// the next add (int8_only, panels_streamed, x16, ivf_tps ...) is state of vdb_index_s.  kOptions (vdbhip.hip, behind
// vdb_index_s) has one row per member: what each accepts is written there, what each does in include/vdbhip.h.
struct Options {
    // behaviour
    int force_path = 0, timing = 0, list_cap = 0;
    int panel_dtype = 0;                     // 1: the int8 scan copy is not used (NOT inverted: non-zero switches the int8 scan off)
    // "int8_only" (takes effect at the next add; flat index, D <= 128, > 32768 rows, byte-valued corpus): only the int8 copies
    // are kept -- rows8 + panels8 + their biases, 0.55x the float32 corpus instead of 3x.  Integer query batches run as on the
    // default index; a batch with a non-integer value is scanned in fp16 over slabs converted from the int8 panels per search;
    // the exact kernels read x = byte + cx from the int8 rows (same float64 chains, same keys).  One add builds it (no append).
    int int8_only = 0;
    int int8_slab_chunks = 0;                // scan chunks per converted fp16 slab (0 = default 8)
    int int8_block_rows = 0;                 // rows per ingestion block of the int8-only build (0 = 4M; tests), and of an add to an
                                             // IVF-I8 index (0 = 1M): the float32 rows of one block are all the device holds of them
    // "stream_panels" (D > 128, takes effect at the next add): the fp16 panels are NOT kept -- every search converts the
    // float32 rows slab by slab into one scratch slab and scans it (search_flat.inc).  Halves the footprint of a non-fp16-exact
    // corpus (the float32 rows must stay for the exact refine) at the price of one conversion pass per batch.
    int stream_panels = 0;
    int64_t stream_slab_rows = 0;            // rows of that slab (0 = default); the one option without an upper bound
    int upload_block_mb = 0;                 // staging block of upload_rows (0 = default 64 MiB)
    int small_batch = 1;                     // 0: batches <= 512 queries keep the batch-shaped grid
    int fused_stats = 1;                     // 0 (A/B): small batches keep the separate statistics dispatch
    int ivf_min_batch = 1;                   // smallest query batch the list-major MFMA scan serves
    int ivf_i8_scratch = 1;                  // IVF-I8: 1 = batches the int8 scan cannot serve scan fp16 panels converted from the int8 ones
                                             // (a workspace slab of the whole panel space) | 0 = no slab: those batches are flagged on the
                                             // device and answered by the exact list scan of the tail.  Same results; no effect elsewhere
    // "graph": a device-resident search that repeats with the same shape and buffers (a serving loop) is captured into a
    // hipGraph on its second call and replayed from the third (graph_or_run)
    int graph = 0;
    int graph_recapture_at_once = 0;         // diagnostic: the pre-round-3 ordering (see graph_or_run)
    int lsh_force_fallback = 0;              // every query of an LSH call takes the exact fallback of the select
    int pq_slab_chunks = 0;                  // scan chunks per slab of panels (0 = default: 524 288 rows' worth)
    int pq_scan_min_batch = 0;               // smallest batch the panel pass + MFMA scan serves (0 = default)
    int pq_adc_max_batch = 0;                // largest batch the lookup-table (ADC) scan serves instead of the panel pass (0 = off)
    int ivfpq_adc_max_batch = 0;             // IVF-PQ: largest batch the lookup-table (ADC) scan of the probed lists serves (0 = off; ivf_adc_plan)
    int ivfpq_adc_part_rows = 0;             // ... rows per row part of that scan (0 auto, else a multiple of 256)
    // k-NN graph (knng.inc)
    int knng_nentry = 0;                     // entry points of a search (0 = default 32)
    int knng_max_iters = 0;                  // step cap of a search (0 = default 8 ef)
    int knng_visited_bits = 0;               // log2 slots of the per-query seen filter (0 = default)
    int knng_build_block = 0;                // rows per self-search block of the build (0 = default)
    int range_bitmap_mb = 0;                 // range search (range_plan.hpp): MiB of candidate bitmap per query slab (0 = default 256)
    int64_t filter_sparse_pairs = kFilterSparsePairsDefault;   // filtered search (filter_plan.hpp, kFilterSparsePairsDefault): (query, admitted row) pairs below which the sparse route serves a call
    // tuning of the flat scans
    int i8_variant = 3;                      // (variant 3: +2 % over 0 on the bench shape, scripts/sweep_i8.py)
    int i8_group = 8, f16_group = 8;         // rows per select group of the int8 / fp16 flat scan (4 or 8)
    int flat_shape = 0;                      // (alias "i8_shape"; before vdb_add) MFMA shape of the flat scans for D <= 128: 0 auto (16) | 16 | 32
    int scan_pair = 1;                       // 0: never the paired launch of the two x16 scans (A/B, diagnosis)
    int scan_prio = 0;                       // x16 kernels: issue priority of one half of the workgroup's waves
    int f16_wide = 0;                        // x16 fp16 batch scan, D <= 64: 0 auto (1024-query tiles when they fit), 1 never
    int f16_stage_tiles = 0;                 // x16 fp16 batch scan: tiles per LDS stage, 0 auto | 4 | 8
    int i8_nt = 0;                           // non-temporal staging loads of the serving-shaped int8 scan (0 auto, 1 never, 2 always)
    int i8_ring = 0;                         // LDS staging stages of the streaming-shaped int8 scans (0 auto, 2, 4, 8)
    int select_variant = 0, spans_per_chunk = 0, kloop_qgroup = 0;      // grid shaping
    // tuning of the IVF list scans
    int ivf_bt = 0;                          // tiles per level-1 bin (0 auto, 4, 16)
    int ivf_part = 0;                        // spans per row part (0 auto)
    int ivf_tps = 0;                         // D > 128, next add: p16 tiles per span of the panel space (0 auto, 16, 64)
    int ivf_tile = 0;                        // workgroup tile of the D > 128 scan on 256-row spans (0 / 2 square, 1 = 128 x 512)
    int ivf_i8_group = 4;                    // rows per candidate group of the int8 list scan (4 | 8)
    int ivf_group = 0;                       // rows per candidate group of the D > 128 list scan (0 auto, 1, 2, 4)
    int ivf_nw = 0;                          // waves per IVF work item (0 auto, 2 / 4 / 8)
};

// ---- what the rules read of a handle (scan_shape_of, search_flat.inc) --------------------------------------------------------
struct ScanIndexShape {
    int ksteps = 0;                 // 16-dim k-steps of the fp16 copy: 4 (D <= 64), 8 (D <= 128), a multiple of 4 above
    int i8_ks = 0;                  // 32-dim k-steps of the int8 copy: 2 (D <= 64) or 4
    int64_t Npad = 0;               // rows padded to whole spans
    int n_cus = 256;
    bool tile16 = false;            // p16 panels (D > 128): 1024-row spans of four bins
    bool x16 = false;               // D <= 128: scan copies in layout "x16"
    bool int8_only = false, panels_streamed = false, pq = false;    // per-search fp16 panels, made slab by slab
    bool i8_ok = false;             // byte-valued corpus: there is an int8 copy
};

// ---- geometry of the scan for a given (N, k) --------------------------------------------------------
struct ScanGeom {
    bool ok = false;
    int64_t nspans = 0;
    int spc = 0, rem = 0, nchunks = 0, vpl = 0;
};

// nq: queries of the batch.  Small batches (serving-shaped: up to one 512-query tile) take FINER chunks, so that the
// grid still covers the chip: at 8192 rows per chunk a 1M-row corpus gives 128 workgroups per query tile, half the CUs.
inline ScanGeom scan_geometry(const ScanIndexShape &s, const Options &opt, int k, int64_t nq) {
    ScanGeom g;
    const int G = s.tile16 ? 4 : 2;                         // bins (lane groups) per span
    g.nspans = s.Npad / (G * kBinRows);
    if (g.nspans * G < 16) return g;
    // superbins (G per chunk) must comfortably outnumber k and fit 16 values per lane in the select
    int64_t spc_hi = g.nspans * G / (4 * (int64_t)k);       // nsb >= 4k
    int64_t spc_lo = (g.nspans * G + 1023) / 1024;          // nsb <= 1024
    if (spc_hi < 1 || spc_hi < spc_lo) return g;
    int64_t spc_want = 32 / G;                              // 8192 rows per chunk
    // (one query tile only: from 1024 queries on the batch shape is as fast or faster -- scripts/throughput_vs_batch.py)
    if (nq <= 512 && opt.small_batch) spc_want = std::max<int64_t>(1, std::min<int64_t>(spc_want, g.nspans / 512));
    int64_t spc = std::min<int64_t>(opt.spans_per_chunk > 0 ? opt.spans_per_chunk : spc_want, spc_hi);
    spc = std::max<int64_t>(spc, spc_lo);
    if (spc < 2 && g.nspans * G >= 128) spc = std::min<int64_t>(2, spc_hi);
    int64_t nchunks = (g.nspans + spc - 1) / spc;
    // deal the spans evenly over a multiple of 8 chunks (one XCD label each, see scan_kernel) when possible
    if (nchunks >= 16) {
        int64_t n8 = (nchunks + 7) / 8 * 8;
        if (n8 * G <= 1024 && g.nspans / n8 >= 1) nchunks = n8;   // (more chunks only add superbins)
    }
    // batch shapes: the multi-lane select (select_kernel_v2) takes <= 256 superbins and is 3-4x faster than the one-wave form
    // (GloVe-shaped 1.2M rows: 304 superbins -> 123 us of select_kernel<8> against ~35 us); chunks of up to twice the default
    // length buy that for corpora of up to 2M rows
    {
        const int64_t cap = 256 / G;
        if (nq > 512 && opt.spans_per_chunk == 0 && nchunks > cap && nchunks <= 2 * cap && cap * G >= 4 * (int64_t)k) nchunks = cap;
    }
    g.nchunks = (int)nchunks;
    g.spc = (int)(g.nspans / nchunks);
    g.rem = (int)(g.nspans - (int64_t)g.spc * nchunks);
    if (g.spc < 1) return g;
    const int nsb = G * g.nchunks;
    g.vpl = 1;
    while (g.vpl * 64 < nsb) g.vpl *= 2;
    if (g.vpl > 16) return g;
    g.ok = true;
    return g;
}

// Direct-bin geometry: when N/256 superbins cannot outnumber k four to one, level-1 bins of 128 or 64 rows serve as
// the superbins themselves (SelectArgs.direct_rows, up to 2048 of them); the chunking then only shapes the grid.
// Returns the rows per bin, 0 if not applicable.
inline int scan_geometry_direct(const ScanIndexShape &s, const Options &, int k, ScanGeom &g) {
    const int G = s.tile16 ? 4 : 2;
    // kernels with the finer bins: scan_kernel<.., BT> (32-row tiles, D <= 128) and scan16_kloop_kernel<.., FP> (p16, D > 128)
    if (s.tile16 != (s.ksteps > kMaxKSteps)) return 0;
    const int64_t nspans = s.Npad / (G * kBinRows);
    if (nspans * G < 16) return 0;
    for (int rows : {128, 64}) {
        const int64_t nb = nspans * G * (kBinRows / rows);
        if (nb >= 4 * (int64_t)k && nb <= 2048) {
            g = ScanGeom{};
            g.nspans = nspans;
            int64_t nchunks = (nspans * G + 31) / 32;                 // ~8192 rows per chunk
            if (nchunks >= 16) nchunks = (nchunks + 7) / 8 * 8;
            nchunks = std::max<int64_t>(1, std::min<int64_t>(nchunks, nspans));
            g.nchunks = (int)nchunks;
            g.spc = (int)(nspans / nchunks);
            g.rem = (int)(nspans - (int64_t)g.spc * nchunks);
            g.vpl = 1;
            while (g.vpl * 64 < nb) g.vpl *= 2;
            g.ok = true;
            return rows;
        }
    }
    return 0;
}

// ---- which scans a batch is offered ---------------------------------------------------------------------------------------------
// small batches: as many waves per workgroup as there are 64-query column groups (1, 2, 4; 8 = the batch shape)
inline int nw_small(const Options &opt, int64_t nq) { return !opt.small_batch ? 8 : nq <= 64 ? 1 : nq <= 128 ? 2 : nq <= 256 ? 4 : 8; }

// int8 scan for byte-valued corpora: offered to the device-side choice whenever the standard geometry is in use
inline bool use_i8(const ScanIndexShape &s, const Options &opt, int direct_rows) {
    const bool i8_off = opt.panel_dtype && !s.int8_only;    // (an int8-only index has nothing but the int8 copies)
    return s.i8_ok && !i8_off && !direct_rows && !s.tile16;
}

// layout "x16" with both scan copies resident: ONE launch holds both scans (scan_pair_x16_kernel, scan_x16.hpp) when every tuning
// option is at its default; otherwise (and on the 32-row layout) both are enqueued and the one not needed returns at once
inline bool pair_candidate(const ScanIndexShape &s, const Options &opt, int direct_rows) {
    return s.x16 && use_i8(s, opt, direct_rows) && !s.int8_only && !s.panels_streamed && direct_rows == 0 && opt.scan_pair &&
           opt.i8_ring == 0 && opt.i8_nt == 0 && opt.f16_stage_tiles == 0 && opt.i8_variant == 3;
}

// candidate groups of the fp16 flat scan (D <= 128, 256-row bins): octs unless option "f16_group" = 4
inline bool f16_octs(const ScanIndexShape &s, const Options &opt, int direct_rows) {
    if (s.x16) return !direct_rows;  // (layout "x16": octs; direct-bin mode -- large k, the refine outweighs the scan -- takes the quads of the two blocks)
    return opt.f16_group == 8 && !direct_rows && s.ksteps <= kMaxKSteps;
}

// tiles per LDS stage of the x16 fp16 batch shape (option "f16_stage_tiles"): measured on the bench shapes (profiles/r04_sweeps.txt)
// D = 64: 8 tiles 1.108 ms against 1.163 with 4 (a 4-tile stage is only 16 KiB of panels per barrier); D = 128: 1.730 against 1.722
inline int st_tiles_of(const ScanIndexShape &s, const Options &opt) { return opt.f16_stage_tiles ? opt.f16_stage_tiles : (s.ksteps == 4 ? 8 : 4); }

// 1024-query workgroup tiles (the x16 fp16 scan at D <= 64, the int8 batch scans) need a batch that is a multiple of 1024 and
// enough tiles to cover the chip; without them every int8 variant folds onto its low bit
inline bool wide_tiles(int nchunks, int64_t Qpad) { return Qpad % 1024 == 0 && (int64_t)nchunks * (Qpad / 1024) >= 256; }

// Streamed panels, slab size (option "stream_slab_rows", 0 = 1 280 000): the K-loop scan runs two 512-thread workgroups per CU and a
// workgroup of a 12.5M-row shard takes ~14.5 ms (chunks are ~50k rows: the select takes <= 1024 superbins), so a
// launch whose workgroup count PER XCD (chunk c runs on XCD c % 8) is not just below a multiple of 2 x 32 idles the
// chip for most of a round (measured, 10 000 queries = 20 workgroups per chunk: 16-chunk slabs 14.5 ms per launch,
// 25-chunk slabs -- four chunks on XCD 0 -- 23 ms).  Take the largest chunk count within `slab_rows` whose workgroups
// fill whole rounds; small query batches (few workgroups per chunk) go by rows alone.
inline int64_t stream_slab_chunks(const ScanIndexShape &s, const Options &opt, const ScanGeom &g, int64_t Qpad) {
    const int64_t chunk_rows = (int64_t)(g.spc + 1) * kSpanRows16;                  // (chunks are spc or spc + 1 spans)
    const int64_t wgs_per_chunk = std::max<int64_t>(1, Qpad / 512);
    const int64_t slab_rows = opt.stream_slab_rows > 0 ? opt.stream_slab_rows : 1280000;
    int64_t slab_chunks = std::max<int64_t>(1, slab_rows / chunk_rows);
    for (int r = 8; r >= 1; --r) {                       // (chunk c of a launch runs on XCD c % 8: count per XCD)
        const int64_t fit = 8 * ((int64_t)2 * (s.n_cus / 8) * r / wgs_per_chunk);
        if (fit >= 8 && fit <= slab_chunks) { slab_chunks = fit; break; }
    }
    return std::max<int64_t>(1, std::min<int64_t>(slab_chunks, g.nchunks));
}

// ---- a launch -------------------------------------------------------------------------------------------------------------------
enum class ScanFamily { none, scan, scan16_kloop, scan_x16, scan_i8, scan_i8x16, scan_pair_x16, ivf_kloop };
constexpr const char *kScanFamilyNames[] = {"none", "scan_kernel", "scan16_kloop_kernel", "scan_x16_kernel", "scan_i8_kernel",
                                            "scan_i8x16_kernel", "scan_pair_x16_kernel", "ivf_kloop_scan_kernel"};
constexpr int kScanFamilyArgs[] = {0, 7, 3, 7, 10, 6, 7, 4};    // template parameters of each family's kernel
constexpr int kScanMaxArgs = 10;

// The template arguments of one instantiation in the kernel's own order, defaults written out (bool as 0 / 1, the rest 0):
//   scan_kernel<KSTEPS, NWAVES, ST, WPS, BT, ITEMS, G8>            scan16_kloop_kernel<BS, FP, NARROW>
//   scan_x16_kernel<KS2, NWAVES, ST, WPS, BR, G, CB>               scan_i8_kernel<KS, ST, CB, NWAVES, BT, ITEMS, G, TB, RING, AUX>
//   scan_i8x16_kernel<KS2, ST, CB, NWAVES, RING, AUX>              scan_pair_x16_kernel<W128, NWAVES, STF, STI, CBI, RING, AUX>
//   ivf_kloop_scan_kernel<TPS, BS, GROUP, RH>  (the IVF list scans: ivf_plan.hpp, which also plans scan_kernel / scan_i8_kernel with ITEMS)
struct ScanKey {
    int t[kScanMaxArgs];
};
inline bool operator==(const ScanKey &a, const ScanKey &b) { return std::equal(a.t, a.t + kScanMaxArgs, b.t); }

struct ScanLaunch {
    ScanFamily family = ScanFamily::none;
    ScanKey key{};
    int nqtiles = 0;                // query tiles of the grid (ScanArgs / ScanI8Args.nqtiles; the pair: of the fp16 body)
    int nqtiles8 = 0;               // the pair: query tiles of the int8 body
    unsigned grid = 0, block = 0;
    int qgroup = 0;                 // K-loop scan: query tiles per group of the block order (ScanKloopExtra)
};

inline unsigned scan_grid(int nchunks, int nqtiles) { return 8u * (unsigned)((nchunks + 7) / 8) * (unsigned)nqtiles; }
inline ScanLaunch scan_launch(ScanFamily f, int nqtiles, unsigned grid, unsigned block, std::initializer_list<int> targs) {
    ScanLaunch p;
    p.family = f;
    std::copy(targs.begin(), targs.end(), p.key.t);
    p.nqtiles = nqtiles;
    p.grid = grid;
    p.block = block;
    return p;
}

// ---- the fp16 scan of `nchunks` chunks (the whole corpus, or one slab of per-search panels) ------------------------------------
inline ScanLaunch plan_f16(const ScanIndexShape &s, const Options &opt, int nchunks, int64_t Qpad, int64_t nq, int direct_rows, int nw) {
    if (s.ksteps > kMaxKSteps) {  // D > 128: p16 panels, 512-query tiles
        // option kloop_qgroup = query tiles per group of the block order (0 -> default)
        const int nqtiles = (int)(Qpad / 512);
        int qgroup = opt.kloop_qgroup > 0 ? opt.kloop_qgroup : 4;
        qgroup = std::min(qgroup, nqtiles);
        const unsigned ngroups = (unsigned)((nqtiles + qgroup - 1) / qgroup);
        const unsigned grid = 8u * (unsigned)((nchunks + 7) / 8) * ngroups * (unsigned)qgroup;
        ScanLaunch p;
        if (direct_rows) p = scan_launch(ScanFamily::scan16_kloop, nqtiles, grid, 512, {2, direct_rows == 128 ? 4 : 2, 0});    // finer level-1 bins
        else if (nq > 0 && nq <= 16 && s.ksteps / 2 <= kNarrowMaxKS && opt.small_batch) p = scan_launch(ScanFamily::scan16_kloop, nqtiles, grid, 512, {3, 8, 2});
        else if (nq > 0 && nq < 64 && opt.small_batch) p = scan_launch(ScanFamily::scan16_kloop, nqtiles, grid, 512, {2, 8, 1});
        else p = scan_launch(ScanFamily::scan16_kloop, nqtiles, grid, 512, {2, 8, 0});
        p.qgroup = qgroup;
        return p;
    }
    if (s.x16) {               // D <= 128 on layout "x16" (scan_x16.hpp)
        const bool small = direct_rows == 0 && nw < 8;
        // D <= 64, batch shape: 1024-query workgroup tiles (8 column blocks = 128 queries per wave) when the batch is a multiple of 1024
        // and there are enough of them to cover the chip -- the rule of the int8 scan (option "f16_wide": 0 auto, 1 never)
        const bool wide = !small && direct_rows == 0 && s.ksteps == 4 && opt.f16_wide != 1 && wide_tiles(nchunks, Qpad);
        const int st_tiles = st_tiles_of(s, opt) == 8 ? 8 : 4;
        const int nqtiles = small ? (int)((nq + nw * 64 - 1) / (nw * 64)) : (int)(Qpad / (wide ? 1024 : 512));
        const unsigned grid = scan_grid(nchunks, nqtiles);
        const int KS2 = s.ksteps == 4 ? 2 : 4;
        if (wide) return scan_launch(ScanFamily::scan_x16, nqtiles, grid, 512, {2, 8, st_tiles, 2, 256, 8, 8});
        if (small) return scan_launch(ScanFamily::scan_x16, nqtiles, grid, 64u * (nw == 1 ? 1 : nw == 2 ? 2 : 4), {KS2, nw == 1 ? 1 : nw == 2 ? 2 : 4, 4, nw <= 2 ? 1 : 2, 256, 8, 4});
        if (direct_rows == 128 || direct_rows == 64) return scan_launch(ScanFamily::scan_x16, nqtiles, grid, 512, {KS2, 8, 4, 2, direct_rows, 4, 4});
        return scan_launch(ScanFamily::scan_x16, nqtiles, grid, 512, {KS2, 8, st_tiles, 2, 256, 8, 4});
    }
    // 32-row-tile layout: 512-query workgroup tiles (8 waves, 4 tiles per LDS stage, 2 waves per SIMD) unless the batch is small
    const int KSTEPS = s.ksteps == 4 ? 4 : 8;
    const int bt = direct_rows ? direct_rows / 16 : 16;       // tiles per level-1 bin
    const int g8 = f16_octs(s, opt, direct_rows) ? 1 : 0;
    if (bt == 16 && nw < 8) {   // small batch: 64 * nw queries per workgroup, only the tiles that hold queries
        const int nqtiles = (int)((nq + nw * 64 - 1) / (nw * 64));
        const int W = nw == 1 ? 1 : nw == 2 ? 2 : 4;
        return scan_launch(ScanFamily::scan, nqtiles, scan_grid(nchunks, nqtiles), 64u * W, {KSTEPS, W, 4, W == 4 ? 2 : 1, 16, 0, g8});
    }
    const int nqtiles = (int)(Qpad / 512);
    // direct-bin mode: finer level-1 bins (8 or 4 tiles)
    return scan_launch(ScanFamily::scan, nqtiles, scan_grid(nchunks, nqtiles), 512, {KSTEPS, 8, 4, 2, bt == 8 ? 8 : bt != 16 ? 4 : 16, 0, bt == 16 ? g8 : 0});
}

// ---- the int8 scan (byte-valued corpora) -----------------------------------------------------------------------------------------
// i8_variant (tuning, every variant exact; scripts/sweep_i8.py): 0 = 512-query tiles (2 column blocks per wave),
// 4-tile stages; 1 = 8-tile stages; 2 = 1024-query tiles (4 column blocks per wave); 3 = both (default);
// 4 / 5 = 16 waves per workgroup (4 per SIMD) with 8- / 16-tile stages; 6 / 7: variant 3 with a pacing barrier per 1 / 2 tiles.
// Odd batch sizes, and batches with too few 1024-query tiles to cover the chip, keep 512-query tiles.
inline ScanLaunch plan_i8(const ScanIndexShape &s, const Options &opt, int nchunks, int64_t Qpad, int64_t nq, int nw) {
    const int ring = opt.i8_ring == 0 ? 4 : opt.i8_ring;
    // serving shapes read every panel byte once per search: non-temporal staging loads (option "i8_nt": 0 / 2 on, 1 off).
    // Measured in one process (scripts/sweep_serving_hbm.py): single-query scan of 4M x 128 (512 MB, HBM) 106.2 -> 96.7 us
    // = 4.8 -> 5.3 TB/s; of 1M x 128 (128 MB, Infinity-Cache resident between searches) 33.9 -> 33.3 us
    const bool nt = opt.i8_nt != 1;
    if (s.x16) {
        // layout "x16" (scan_i8x16.hpp, v_mfma_i32_16x16x64_i8): the same launch shapes -- batch: 512- or 1024-query tiles
        // (4 or 8 column blocks of 16 queries per wave), 4- or 8-tile stages (i8_variant bits as above, 4 / 5 -> 3);
        // serving: 1 / 2 / 4 waves of 64 queries, 4-stage staging ring (option "i8_ring": 2, 4, 8), non-temporal loads
        int v = opt.i8_variant & 3;
        if (opt.i8_variant == 4 || opt.i8_variant == 5) v = 3;
        if (!wide_tiles(nchunks, Qpad)) v &= 1;
        const int qtile = nw < 8 ? 64 * nw : (v >= 2) ? 1024 : 512;
        const int nqtiles = (int)((nw < 8 ? nq + qtile - 1 : Qpad) / qtile);
        const unsigned grid = scan_grid(nchunks, nqtiles);
        const int KS2 = s.i8_ks == 2 ? 1 : 2;
        if (nw >= 8 || (nw != 1 && nw != 2 && nw != 4)) return scan_launch(ScanFamily::scan_i8x16, nqtiles, grid, 512, {KS2, (v & 1) ? 8 : 4, v >= 2 ? 8 : 4, 8, 2, 0});
        if (ring == 2) return scan_launch(ScanFamily::scan_i8x16, nqtiles, grid, 64u * nw, {KS2, 4, 4, nw, 2, 0});
        if (ring == 8 && nw >= 2) return scan_launch(ScanFamily::scan_i8x16, nqtiles, grid, 64u * nw, {KS2, 4, 4, nw, 8, 0});
        return scan_launch(ScanFamily::scan_i8x16, nqtiles, grid, 64u * nw, {KS2, 4, 4, nw, 4, nt ? 2 : 0});
    }
    int v8 = opt.i8_variant;
    const int tb8 = v8 == 6 ? 1 : v8 == 7 ? 2 : 0;             // 6 / 7: variant 3 with a pacing barrier per 1 / 2 tiles
    if (tb8) v8 = 3;
    if (!wide_tiles(nchunks, Qpad)) v8 &= 1;                   // too few 1024-query tiles to cover the chip: 512-query tiles
    if (nw < 8) v8 = 8 + nw;
    const int qtile = (v8 > 8) ? 64 * nw : (v8 >= 2) ? 1024 : 512;
    const int nqtiles = (int)((v8 > 8 ? nq + qtile - 1 : Qpad) / qtile);
    const unsigned grid = scan_grid(nchunks, nqtiles);
    const int KS = s.i8_ks == 2 ? 2 : 4, G = opt.i8_group == 8 ? 8 : 4;
    if (tb8 && v8 == 3 && G == 8) return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 512, {KS, 8, 4, 8, 16, 0, 8, tb8, 2, 0});
    if (v8 == 9 || v8 == 10 || v8 == 12) {
        // serving shapes (1 / 2 / 4 waves per workgroup): the scan streams the copy once -- 4- or 8-stage staging ring
        // (option "i8_ring": 0 = auto (4), 2 = the double buffer of the batch shape, 4, 8)
        // (the wait for a stage is s_waitcnt vmcnt((ring - 2) x requests per wave and stage), a 6-bit counter: a one-wave
        //  workgroup issues all 16 + 2 requests of a 4-tile stage itself, which caps its ring at 4)
        const int R = ring == 2 ? 2 : (ring == 8 && nw >= 2) ? 8 : 4;
        const int aux = (ring != 2 && ring != 8 && nt && G == 8) ? 2 : 0;
        return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 64u * nw, {KS, 4, 2, nw, 16, 0, G, 0, R, aux});
    }
    switch (v8) {
        case 1: return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 512, {KS, 8, 2, 8, 16, 0, G, 0, 2, 0});
        case 2: return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 512, {KS, 4, 4, 8, 16, 0, G, 0, 2, 0});
        case 3: return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 512, {KS, 8, 4, 8, 16, 0, G, 0, 2, 0});
        case 4: return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 1024, {KS, 8, 2, 16, 16, 0, G, 0, 2, 0});
        case 5: return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 1024, {KS, 16, 2, 16, 16, 0, G, 0, 2, 0});
        default: return scan_launch(ScanFamily::scan_i8, nqtiles, grid, 512, {KS, 4, 2, 8, 16, 0, G, 0, 2, 0});
    }
}

// ---- both x16 scans in one launch ------------------------------------------------------------------------------------------------
// family none: not a pair candidate, or a shape the paired kernel is not built for -- the fp16 scan and the int8 scan then go as
// two launches (plan_f16, plan_i8), as ever
inline ScanLaunch plan_pair(const ScanIndexShape &s, const Options &opt, int nchunks, int64_t Qpad, int64_t nq, int direct_rows, int nw) {
    if (!pair_candidate(s, opt, direct_rows)) return ScanLaunch{};
    const ScanLaunch i8 = plan_i8(s, opt, nchunks, Qpad, nq, nw);
    const bool small = nw < 8;
    const int st_i8 = i8.key.t[1], cb_i8 = i8.key.t[2];
    if (!small && !(st_i8 == 8)) return ScanLaunch{};       // (the batch forms with 8-tile int8 stages: variants 3 and 1)
    const int nqtiles16 = small ? (int)((nq + nw * 64 - 1) / (nw * 64)) : (int)(Qpad / 512);
    const unsigned grid = std::max(scan_grid(nchunks, nqtiles16), i8.grid);
    const int W = s.i8_ks == 4 ? 1 : 0;
    ScanLaunch p = small ? scan_launch(ScanFamily::scan_pair_x16, nqtiles16, grid, 64u * nw, {W, nw, 4, 4, 4, 4, 2})
                         : scan_launch(ScanFamily::scan_pair_x16, nqtiles16, grid, 512, {W, 8, W ? 4 : 8, 8, cb_i8, 2, 0});
    p.nqtiles8 = i8.nqtiles;
    return p;
}

// ---- every instantiation of each family, once ------------------------------------------------------------------------------------
// X(template arguments in the kernel's own order, defaults written out).  The set is what the flat search can launch; the ITEMS forms of
// the IVF list scans are listed in ivf_plan.hpp.
#define VDB_KERNELS_SCAN_K(X, K) /* serving: 1 / 2 / 4 waves, quads and octs | batch: direct bins of 8 and 4 tiles, quads, octs */ \
    X(K, 1, 4, 1, 16, false, false) X(K, 2, 4, 1, 16, false, false) X(K, 4, 4, 2, 16, false, false) \
    X(K, 1, 4, 1, 16, false, true) X(K, 2, 4, 1, 16, false, true) X(K, 4, 4, 2, 16, false, true) \
    X(K, 8, 4, 2, 8, false, false) X(K, 8, 4, 2, 4, false, false) X(K, 8, 4, 2, 16, false, false) X(K, 8, 4, 2, 16, false, true)
#define VDB_KERNELS_SCAN(X) VDB_KERNELS_SCAN_K(X, 4) VDB_KERNELS_SCAN_K(X, 8)

#define VDB_KERNELS_SCAN16_KLOOP(X) X(2, 4, 0) X(2, 2, 0) X(3, 8, 2) X(2, 8, 1) X(2, 8, 0)

#define VDB_KERNELS_SCAN_X16_K(X, KS2) /* serving | direct bins of 128 and 64 rows (quads) | batch: 8- and 4-tile stages */ \
    X(KS2, 1, 4, 1, 256, 8, 4) X(KS2, 2, 4, 1, 256, 8, 4) X(KS2, 4, 4, 2, 256, 8, 4) \
    X(KS2, 8, 4, 2, 128, 4, 4) X(KS2, 8, 4, 2, 64, 4, 4) X(KS2, 8, 8, 2, 256, 8, 4) X(KS2, 8, 4, 2, 256, 8, 4)
#define VDB_KERNELS_SCAN_X16(X) /* D <= 64: 1024-query tiles */ \
    X(2, 8, 8, 2, 256, 8, 8) X(2, 8, 4, 2, 256, 8, 8) VDB_KERNELS_SCAN_X16_K(X, 2) VDB_KERNELS_SCAN_X16_K(X, 4)

// serving rows of NW waves: ring 2, ring 4 with non-temporal loads (octs only), ring 4 -- (ring 8 at one wave is the ring-4 kernel)
#define VDB_KERNELS_SCAN_I8_S(X, KS, NW) \
    X(KS, 4, 2, NW, 16, false, 8, 0, 2, 0) X(KS, 4, 2, NW, 16, false, 4, 0, 2, 0) X(KS, 4, 2, NW, 16, false, 8, 0, 4, 2) \
    X(KS, 4, 2, NW, 16, false, 8, 0, 4, 0) X(KS, 4, 2, NW, 16, false, 4, 0, 4, 0)
#define VDB_KERNELS_SCAN_I8_G(X, KS, G) /* batch variants 0, 1, 2, 3, 4, 5 | serving, ring 8 at 2 and 4 waves */ \
    X(KS, 4, 2, 8, 16, false, G, 0, 2, 0) X(KS, 8, 2, 8, 16, false, G, 0, 2, 0) X(KS, 4, 4, 8, 16, false, G, 0, 2, 0) \
    X(KS, 8, 4, 8, 16, false, G, 0, 2, 0) X(KS, 8, 2, 16, 16, false, G, 0, 2, 0) X(KS, 16, 2, 16, 16, false, G, 0, 2, 0) \
    X(KS, 4, 2, 2, 16, false, G, 0, 8, 0) X(KS, 4, 2, 4, 16, false, G, 0, 8, 0)
#define VDB_KERNELS_SCAN_I8_K(X, KS) /* ... | variants 6, 7: a pacing barrier per 1 / 2 tiles */ \
    VDB_KERNELS_SCAN_I8_G(X, KS, 8) VDB_KERNELS_SCAN_I8_G(X, KS, 4) X(KS, 8, 4, 8, 16, false, 8, 1, 2, 0) X(KS, 8, 4, 8, 16, false, 8, 2, 2, 0) \
    VDB_KERNELS_SCAN_I8_S(X, KS, 1) VDB_KERNELS_SCAN_I8_S(X, KS, 2) VDB_KERNELS_SCAN_I8_S(X, KS, 4)
#define VDB_KERNELS_SCAN_I8(X) VDB_KERNELS_SCAN_I8_K(X, 2) VDB_KERNELS_SCAN_I8_K(X, 4)

#define VDB_KERNELS_SCAN_I8X16_S(X, KS2, NW) X(KS2, 4, 4, NW, 2, 0) X(KS2, 4, 4, NW, 4, 2) X(KS2, 4, 4, NW, 4, 0)
#define VDB_KERNELS_SCAN_I8X16_K(X, KS2) /* batch variants 3, 2, 1, 0 | serving | ring 8 at 2 and 4 waves */ \
    X(KS2, 8, 8, 8, 2, 0) X(KS2, 4, 8, 8, 2, 0) X(KS2, 8, 4, 8, 2, 0) X(KS2, 4, 4, 8, 2, 0) \
    VDB_KERNELS_SCAN_I8X16_S(X, KS2, 1) VDB_KERNELS_SCAN_I8X16_S(X, KS2, 2) VDB_KERNELS_SCAN_I8X16_S(X, KS2, 4) \
    X(KS2, 4, 4, 2, 8, 0) X(KS2, 4, 4, 4, 8, 0)
#define VDB_KERNELS_SCAN_I8X16(X) VDB_KERNELS_SCAN_I8X16_K(X, 1) VDB_KERNELS_SCAN_I8X16_K(X, 2)

#define VDB_KERNELS_SCAN_PAIR_X16_W(X, W, STF) \
    X(W, 1, 4, 4, 4, 4, 2) X(W, 2, 4, 4, 4, 4, 2) X(W, 4, 4, 4, 4, 4, 2) X(W, 8, STF, 8, 8, 2, 0) X(W, 8, STF, 8, 4, 2, 0)
#define VDB_KERNELS_SCAN_PAIR_X16(X) VDB_KERNELS_SCAN_PAIR_X16_W(X, true, 4) VDB_KERNELS_SCAN_PAIR_X16_W(X, false, 8)

#define VDB_SCAN_KEY(...) ScanKey{{__VA_ARGS__}},
constexpr ScanKey kKeysScan[] = {VDB_KERNELS_SCAN(VDB_SCAN_KEY)};
constexpr ScanKey kKeysScan16Kloop[] = {VDB_KERNELS_SCAN16_KLOOP(VDB_SCAN_KEY)};
constexpr ScanKey kKeysScanX16[] = {VDB_KERNELS_SCAN_X16(VDB_SCAN_KEY)};
constexpr ScanKey kKeysScanI8[] = {VDB_KERNELS_SCAN_I8(VDB_SCAN_KEY)};
constexpr ScanKey kKeysScanI8x16[] = {VDB_KERNELS_SCAN_I8X16(VDB_SCAN_KEY)};
constexpr ScanKey kKeysScanPairX16[] = {VDB_KERNELS_SCAN_PAIR_X16(VDB_SCAN_KEY)};

}  // namespace vdb

// ivf_plan.hpp -- where the path and the launch shapes of an IVF search batch are decided: plain host C++ (no HIP header, no handle),
// beside scan_plan.hpp, so the rules compile with an ordinary host compiler and tests/host/ivf_plan_main.cpp prints what they give.
//   constants of the IVF panel space and of the per-batch plan | IvfIndexShape (what the rules read of a handle) | ivf_tps_of
//   ivf_geometry -> IvfGeom: does the list-major MFMA scan serve the batch, and with which bins, waves, capacities
//   ivf_part_spans | plan_ivf_f16 / plan_ivf_i8 / plan_ivf_kloop -> IvfLaunch: kernel family, template arguments, grid, block, row parts
//   ivf_caps / ivf_select_caps: the capacities of the work lists and of the select | ivf_exact_splits: the exact list scan
//   ivf_adc_plan -> IvfAdcPlan: does the lookup-table (ADC) scan of an IVF-PQ index serve the batch, and with which row parts
//   VDB_KERNELS_IVF_*: every instantiation of a family, once -- the keys the host program walks and (ivf.inc) the table of
//   kernel pointers `ivf_launch` looks a plan up in
// (the coarse search over the centroids is a flat search: scan_plan.hpp)
#pragma once
#include <stddef.h>

#include <cmath>

#include "scan_plan.hpp"

namespace vdb {

// ---- constants the rules and the kernels share ------------------------------------------------------------------------------------
// IVF panel space (D <= 128): every inverted list is padded to whole spans, so its spans are SMALLER -- 8 tiles = 256 rows,
// each lane half walking 128 consecutive rows: k-means lists of ~750 rows then carry 2 % of padding instead of 36 %
// (512-row spans padded the median list of the SIFT1M / nlist 1024 index from 752 to 1024 rows).  Same row mapping inside a
// span as the flat layout (common.hpp) with 16 -> kIvfTilesPerSpan tiles.
constexpr int kIvfTilesPerSpan = 8;
constexpr int kIvfSpanRows = kIvfTilesPerSpan * 32;     // (32-row tiles: kTileRows, common.hpp)
// per-list probe counts (ivf_mfma.hpp).  Workgroup-local LDS histogram first (nlist <= kIvfLdsLists), then one global atomic
// per (workgroup, touched list): 1.28 M probes on 1024 lists would otherwise serialise on 1024 addresses.
constexpr int kIvfLdsLists = 8192;
constexpr int kIvfPairsPerBlock = 4096;
constexpr int kIvfMaxProbes = 512;      // probes per query ivf_select_kernel resolves
constexpr int kIvfMaxEntries = 4096;    // bins per query the select keeps in LDS
// Quad minima kept per bin of the D > 128 list scan (ivf_kloop.hpp).  The D <= 128 scans keep three (one v_med3 each per quad: their
// select is issue-bound); there the select runs once per pass of D / 64 K-steps, so two more cost ~1 % -- and they matter: the near
// neighbours of a query sit in one or two of its probed lists, i.e. several per 64-row bin, and a bin with more close quads than
// minima kept must be re-scored whole (with three minima the msmarco-shaped leg re-scored 5.8 bins = 370 rows of 1.5 KB per query,
// 70 % of its time; with five a bin yields up to four candidate quads before it has to be re-scanned).
constexpr int kIvfKloopMinima = 5;
constexpr int kIvfKloopGroup = 512;     // query slots per work item of the D > 128 list scan
constexpr int kIvfKloopGroupRows = 1;   // default candidate group of the D > 128 list scan on 64-row bins (measured: DESIGN 4.4, round 4)

// ---- what the rules read of a handle (ivf_shape_of, ivf.inc) ------------------------------------------------------------------------
struct IvfIndexShape {
    bool mfma_ok = false;           // the panel space of the lists is built (ivf_build_panel_space)
    bool tile16 = false;            // D > 128: p16 panels, the K-loop list scan
    int nlist = 0;
    int64_t N = 0;
    int64_t pspans = 0;             // panel spans of all lists
    int max_pspans = 0;             // ... of the longest list
    int span_rows = 0, tps = 0;     // rows of a panel span; D > 128: its p16 tiles (16 or 64), else 0
    int ksteps = 0, i8_ks = 0;      // as ScanIndexShape
    bool has_i8 = false;            // byte-valued rows with the int8 copy of the panel space
};

// D > 128, the span size of the build (option "ivf_tps"): 64 tiles (1024-row spans) for lists of thousands of rows, else 16
inline int ivf_tps_of(const Options &opt, int64_t N, int nlist) {
    return (opt.ivf_tps == 16 || opt.ivf_tps == 64) ? opt.ivf_tps : ((double)N / nlist > 2048.0 ? 64 : 16);
}

// ---- geometry of one batch on the list-major path (ok = false: the batch takes the exact list scan) -------------------------------
struct IvfGeom {
    bool ok = false, kloop = false;
    int bt = 16, bps = 1, bins_per_span = 2, bin_rows = 256, nw = 2, group = 128, run_groups = 0;
    int64_t pairs = 0, max_items = 0, max_slots = 0, max_bins = 0;
    size_t bin_bytes = 0, cnt_words = 0;
};

inline IvfGeom ivf_geometry(const IvfIndexShape &s, const Options &opt, int64_t nb, int k, int nprobe) {
    IvfGeom g;
    if (!s.mfma_ok || opt.force_path == 1 || opt.force_path == 3 || nb < opt.ivf_min_batch || k > 256 || nprobe > kIvfMaxProbes) return g;
    const int nlist = s.nlist;
    const double avg_pspans = (double)s.pspans / (double)nlist;
    const bool kloop = s.tile16;                                  // D > 128: ivf_kloop_scan_kernel on p16 panels
    // bin size: 128 rows (bt = 8: one bin per half of a 256-row span) when the probed lists still give >= 8k bins per
    // query, else 64 rows (bt = 4)
    int bt = kIvfTilesPerSpan;
    if ((double)nprobe * (double)s.span_rows / 128.0 * avg_pspans < 8.0 * k) bt = 4;
    if (opt.ivf_bt == 4) bt = 4;                                       // option "ivf_bt" (A/B, both exact): 4, or 16 = the largest
    else if (opt.ivf_bt == 16) bt = kIvfTilesPerSpan;
    const int bps = kIvfTilesPerSpan / bt;
    // level-1 bins of a panel span and rows per bin (p16: one bin per lane group, fixed by the span size of the build)
    const int bins_per_span = kloop ? 4 : 2 * bps;
    const int bin_rows = kloop ? s.tps * 4 : bt * 16;
    const double est_entries = (double)nprobe * bins_per_span * avg_pspans;
    if (est_entries < 4.0 * k || est_entries > 0.7 * kIvfMaxEntries) return g;
    const int64_t pairs = nb * nprobe;
    // waves per work item (64 query slots each): every probed list gets ceil(pairs of the list / (64 nw)) items, so a
    // group much larger than the typical number of pairs per list wastes MFMA work on padding slots; a smaller group
    // streams the list's panels more often (from L2).  Option "ivf_nw" forces 2 / 4 / 8.
    const double per_list = (double)pairs / nlist;
    int nw = 2;
    {   // padded slots of a typical list, with a 5 % preference per doubling of the group (measured, scripts/sweep_ivf.py:
        // nprobe 8 / 32 / 128 at nlist 1024 and 10k queries -> 2 / 2 / 4 waves)
        double best = 1.0e300;
        for (int cand : {2, 4, 8}) {
            const double slots = std::ceil(per_list / (64.0 * cand)) * 64.0 * cand;
            const double cost = slots * (cand == 2 ? 1.10 : (cand == 4 ? 1.05 : 1.0));
            if (cost < best) {
                best = cost;
                nw = cand;
            }
        }
    }
    if (opt.ivf_nw == 2 || opt.ivf_nw == 4 || opt.ivf_nw == 8) nw = opt.ivf_nw;
    // (K-loop scan: 8 waves share the A staging; 512 slots per item, or 256 with the square workgroup tile -- 256-row spans,
    //  option "ivf_tile" = 2; measured equal within 3 %, so 128 x 512 stays the default: ivf_kloop.hpp)
    if (kloop) nw = (s.tps == 16 && opt.ivf_tile == 2 ? kIvfKloopGroup / 2 : kIvfKloopGroup) / 64;
    const int group = 64 * nw;
    const int64_t max_items = (pairs + group - 1) / group + std::min<int64_t>(nlist, pairs);
    const int64_t max_slots = max_items * group;
    // (32-row-tile scans: one run of bins per lane half, each padded to a multiple of 4 -- at most 3 more bins per half)
    const int run_groups = kloop ? 0 : 2;
    const int64_t run_pad = run_groups * 3;
    const int64_t max_bins = ((pairs + group - 1) / group) * (bins_per_span * s.max_pspans + run_pad) +
                             (int64_t)bins_per_span * s.pspans + run_pad * std::min<int64_t>(nlist, pairs);
    const size_t bin_bytes = (size_t)max_bins * group * sizeof(float);
    if (bin_bytes > ((size_t)3 << 30) || max_slots > (1ll << 30)) return g;
    g.kloop = kloop; g.bt = bt; g.bps = bps; g.bins_per_span = bins_per_span; g.bin_rows = bin_rows; g.nw = nw; g.group = group;
    g.run_groups = run_groups;
    g.pairs = pairs; g.max_items = max_items; g.max_slots = max_slots; g.max_bins = max_bins; g.bin_bytes = bin_bytes;
    // per-list counters, cursors, the slot -> query map (query + 1, 0 = padding slot) and one arrival counter per query for
    // the split fallback pass (ivf_fallback_body in ivf_tail_kernel): all cleared with the two ws.small by ONE memset per batch
    g.cnt_words = (size_t)2 * nlist + (size_t)max_slots + (size_t)nb;
    g.ok = true;
    return g;
}

// ---- capacities of the work lists and of the per-batch plan kernels (ivf_lists_reserve) -------------------------------------------
struct IvfCaps {
    bool use_i8 = false, small_ppb = false;
    int kgroup = 4, cand_cap = 0, rescan_cap = 0, ppb = 0;
    unsigned pblocks = 0;
    size_t hist_bytes = 0;
};

inline IvfCaps ivf_caps(const IvfIndexShape &s, const Options &opt, const IvfGeom &g, int k) {
    IvfCaps c;
    // rows per candidate group of the K-loop scan (option "ivf_group": 0 auto, 1, 2, 4): 64-row bins can name single rows
    c.kgroup = (g.kloop && s.tps == 16) ? (opt.ivf_group > 0 ? opt.ivf_group : kIvfKloopGroupRows) : 4;
    // (five minima per bin: a dense bin hands over up to four candidate quads instead of one re-scan)
    c.cand_cap = opt.list_cap > 0 ? opt.list_cap : (g.kloop ? std::max(96, 4 * k + 32) : std::max(64, 2 * k + 32));
    c.rescan_cap = std::max(16, k / 2 + 8);
    c.use_i8 = s.has_i8 && !opt.panel_dtype;
    c.small_ppb = g.pairs < 256 * (int64_t)kIvfPairsPerBlock && s.nlist <= 2048;   // (fewer than 256 workgroups otherwise)
    c.ppb = c.small_ppb ? kIvfPairsPerBlock / 4 : kIvfPairsPerBlock;
    c.pblocks = (unsigned)((g.pairs + c.ppb - 1) / c.ppb);
    c.hist_bytes = s.nlist <= kIvfLdsLists ? (size_t)s.nlist * 4 : 0;
    return c;
}

// ---- capacities of ivf_select_kernel's LDS arrays (their word count: ivf_select_lds_words, ivf_mfma.hpp) ---------------------------
struct IvfSelectCaps {
    int max_entries = 0, probe_cap = 0, vals_entries = 0, act_cap = 0, nm = 0;
};

inline IvfSelectCaps ivf_select_caps(const IvfIndexShape &s, const IvfGeom &g, const IvfCaps &c, int k, int nprobe) {
    IvfSelectCaps e;
    e.nm = g.kloop ? kIvfKloopMinima : 3;
    // a query can meet at most nprobe * (bins of the longest list) entries
    const int64_t worst = (int64_t)nprobe * (s.max_pspans * g.bins_per_span + g.run_groups * 3);
    e.max_entries = (int)std::min<int64_t>(kIvfMaxEntries, (worst + 63) / 64 * 64);
    e.probe_cap = (nprobe + 63) / 64 * 64;
    e.vals_entries = k > 64 ? e.max_entries : 0;
    e.act_cap = std::min(c.cand_cap + c.rescan_cap, e.max_entries);       // (entry numbers are packed into 16 bits: <= 4096)
    {   // two waves per workgroup within the 64 KiB a kernel gets without opting in: 8192 words per wave
        const int fixed = e.vals_entries + 4 * e.probe_cap + 64;
        e.act_cap = std::max(64, std::min(e.act_cap, (8192 - fixed) / (1 + e.nm)));
    }
    return e;
}

// ---- the exact list scan: splits of a query's probed lists (one wave each, merged when S > 1) ------------------------------------
inline int64_t ivf_exact_splits(int64_t N, int nlist, int nprobe, int64_t nb, int k) {
    // waves per query: keep each wave's share of rows moderate and the GPU full
    const double rows_per_query = (double)nprobe * (double)N / (double)nlist;
    int64_t S = (int64_t)std::ceil(rows_per_query / 4096.0);
    S = std::max<int64_t>(S, (8192 + nb - 1) / nb);
    S = std::max<int64_t>(1, std::min<int64_t>(S, nprobe));
    const int64_t cap = std::max<int64_t>(1, (int64_t)(256ll << 20) / (nb * k * 16));
    return std::min<int64_t>(S, cap);
}

// ---- IVF-PQ: the lookup-table (ADC) scan of the probed lists (ivf_pq_adc.hpp, DESIGN 4.4 "IVF-PQ ADC scan") -------------------------
// Asked BEFORE ivf_geometry: an admitted batch takes neither the panel pass nor the exact list scan.  Off unless option
// "ivfpq_adc_max_batch" is set.  The LDS rule is the flat ADC scan's (pq.inc, pq_adc_fits), so an M is served by both scans or by
// neither: M <= 159.  `ranges_ok`: the handle's norms are usable (ivfpq_adc_prepare, ivf_pq.inc).  The scores of a batch are kept
// as [nb][stride] float32, stride = the most rows a query can probe.
constexpr int kIvfAdcMaxBatch = 512, kIvfAdcMaxK = 1024, kIvfAdcMaxParts = 64;
constexpr int kIvfAdcAuxBytes = 128, kIvfAdcLdsBudget = 160 * 1024;
constexpr int64_t kIvfAdcScoreBytes = 256ll << 20;
constexpr int kIvfAdcCandMax = 4096;    // candidates per query the tail keeps in LDS (row + exact key: 48 KiB)
struct IvfAdcPlan {
    bool ok = false;
    int part_rows = 0;              // rows per row part, a multiple of 256
    unsigned parts = 0;             // grid: row parts of the longest list (<= kIvfAdcMaxParts); parts beyond a list's end exit
    int64_t stride = 0;             // scores per query: min(N, nprobe * longest list)
    int cand_cap = 0;               // candidates per query before it is flagged
    size_t lds_bytes = 0;           // dynamic LDS of the scan: the query's table
};
inline IvfAdcPlan ivf_adc_plan(const Options &opt, int codec, int M, bool ranges_ok, int64_t N, int64_t max_list, int64_t nb, int k, int nprobe) {
    IvfAdcPlan p;
    if (codec != 2 || opt.force_path != 0) return p;
    if (nb < 1 || nb > opt.ivfpq_adc_max_batch || nb > kIvfAdcMaxBatch || k > kIvfAdcMaxK) return p;
    if (M < 1 || (int64_t)M * 1024 + kIvfAdcAuxBytes > kIvfAdcLdsBudget) return p;
    if (!ranges_ok || N <= 0 || max_list <= 0 || nprobe < 1) return p;
    p.stride = std::min<int64_t>(N, (int64_t)nprobe * max_list);
    if (nb * p.stride * 4 > kIvfAdcScoreBytes) return p;
    // row parts: one workgroup per (part, probe, query), each loads the table (M KiB, from L2) for M bytes of codes per row -- few
    // (query, probe) pairs take 256-row parts to put more workgroups on the chip, many take 1024-row parts
    const int64_t pairs = nb * nprobe;
    int part = opt.ivfpq_adc_part_rows > 0 ? opt.ivfpq_adc_part_rows : pairs < 256 ? 256 : pairs < 1024 ? 512 : 1024;
    const int64_t least = ((max_list + kIvfAdcMaxParts - 1) / kIvfAdcMaxParts + 255) / 256 * 256;
    p.part_rows = (int)std::max<int64_t>(part, least);
    p.parts = (unsigned)((max_list + p.part_rows - 1) / p.part_rows);
    p.cand_cap = std::min(kIvfAdcCandMax, opt.list_cap > 0 ? opt.list_cap : std::max(64, 2 * k + 32));
    p.lds_bytes = (size_t)M * 1024;
    p.ok = true;
    return p;
}

// ---- row parts ----------------------------------------------------------------------------------------------------------------------
// Long lists are cut into row parts of some spans each, one workgroup per (item, part): the scan's duration is otherwise the
// LONGEST list's (k-means lists are far from even: 5x the median on SIFT-like data).  `base` = the scan's own choice of the
// part size (option "ivf_part" overrides it), rounded up to `unit` spans.  At most 64 parts per item: every (item, part) is
// a workgroup, and the parts beyond a short list's end only exit -- one giant list must not turn the launch into millions of
// empty workgroups.  Returns the part size (0 = whole lists) and the grid
struct IvfParts {
    int part_spans;
    unsigned grid_x, grid_y;
};
inline IvfParts ivf_part_spans(const Options &opt, int max_pspans, int64_t max_items, int base, int unit) {
    int part = std::min(std::max(opt.ivf_part > 0 ? opt.ivf_part : base, (max_pspans + 63) / 64), max_pspans);
    part = (part + unit - 1) / unit * unit;
    const int part_spans = part >= max_pspans ? 0 : part;
    return {part_spans, (unsigned)max_items, (unsigned)(part_spans ? (max_pspans + part - 1) / part : 1)};
}

// ---- a launch of a list scan --------------------------------------------------------------------------------------------------------
// family: scan (scan_kernel, ITEMS), scan_i8 (scan_i8_kernel, ITEMS) or ivf_kloop; key: as ScanLaunch.  Grid x = work items, y = row parts
struct IvfLaunch {
    ScanFamily family = ScanFamily::none;
    ScanKey key{};
    unsigned grid_x = 0, grid_y = 0, block = 0;
    int part_spans = 0;             // ScanArgs / ScanI8Args / IvfKloopArgs.part_spans
};
inline IvfLaunch ivf_launch_of(ScanFamily f, const IvfParts &parts, unsigned block, std::initializer_list<int> targs) {
    IvfLaunch p;
    p.family = f;
    std::copy(targs.begin(), targs.end(), p.key.t);
    p.grid_x = parts.grid_x; p.grid_y = parts.grid_y; p.block = block; p.part_spans = parts.part_spans;
    return p;
}

// D <= 128: scan_kernel in ITEMS mode on 32-row tiles
inline IvfLaunch plan_ivf_f16(const IvfIndexShape &s, const Options &opt, const IvfGeom &g) {
    // row parts of 256-row spans (measured in 512-row units, scripts/sweep_ivf.py --option ivf_part: nprobe 8 / 32 / 128 at
    //  nlist 1024, 10k queries -> 1 / 2 / 4 spans; the fewer work items there are, the finer the parts)
    const int part_auto = (kSpanRows / kIvfSpanRows) * (g.max_items <= 2048 ? 1 : g.max_items <= 4096 ? 2 : 4);
    // a row part starts at a multiple of 4 bins of the lane's run (the bins leave as 16-byte vectors; bps = bins of a span half)
    const IvfParts parts = ivf_part_spans(opt, s.max_pspans, g.max_items, part_auto, 4 / g.bps);
    const int NW = g.nw == 2 ? 2 : g.nw == 4 ? 4 : 8;
    return ivf_launch_of(ScanFamily::scan, parts, 64u * NW, {s.ksteps == 4 ? 4 : 8, NW, 2, 2, g.bt == 4 ? 4 : 8, 1, 0});
}

// the int8 form of the same scan, on the fp16 scan's grid and row parts
inline IvfLaunch plan_ivf_i8(const IvfIndexShape &s, const Options &opt, const IvfGeom &g) {
    const IvfLaunch f = plan_ivf_f16(s, opt, g);
    const IvfParts parts{f.part_spans, f.grid_x, f.grid_y};
    const int NW = f.key.t[1], BT = f.key.t[4];
    // (tiles per LDS stage: 2 -- 8 pieces per stage for 8 waves make it 4 at two k-steps; deeper stages measured
    //  slower at nprobe 32 / 128 and equal at 8 once the lists are scanned in row parts)
    const int KS = s.i8_ks == 2 ? 2 : 4, ST = s.i8_ks == 2 ? 4 : 2;
    // (select groups stay quads here: measured with octs the list scan gains 5 % and the refine loses more -- the
    //  probed lists are dense in near neighbours, so an 8-row group drags in more re-scans and twice the rows)
    // staging ring of the work items (option "i8_ring"; 0 = auto): a work item streams its list once, and few of them
    // are resident per CU -- 4 stages of 2 (4 at two k-steps) tiles in flight instead of 1
    const int ring = opt.i8_ring == 0 ? 4 : opt.i8_ring;
    if (opt.ivf_i8_group == 8) return ivf_launch_of(ScanFamily::scan_i8, parts, 64u * NW, {KS, ST, 2, NW, BT, 1, 8, 0, 4, 0});
    return ivf_launch_of(ScanFamily::scan_i8, parts, 64u * NW, {KS, ST, 2, NW, BT, 1, 4, 0, ring == 2 ? 2 : ring == 8 ? 8 : 4, 0});
}

// D > 128: the K-loop scan on p16 panels (ivf_kloop.hpp); kgroup: IvfCaps
inline IvfLaunch plan_ivf_kloop(const IvfIndexShape &s, const Options &opt, const IvfGeom &g, int kgroup) {
    // row parts: 128 rows x 512 slots x D of matrix work per pass -- a part of ~1024 rows keeps a workgroup busy for
    // tens of microseconds at 384 dims; few work items -> finer parts (down to one span) to cover the chip
    // (measured on the msmarco shape, 725 items of ~4 spans: scripts/sweep_ivf.py --workload msmarco_ivf --option ivf_part:
    //  whole lists (8 spans) 0.612 ms, 4 spans 0.525, 2 spans 0.510, 1 span 0.528 -- ~1500 workgroups for the chip's 512
    //  slots, and never less than 512 rows per workgroup: every part gathers its B fragments and fills its pipeline anew)
    const int spans_512 = std::max(1, 512 / s.span_rows);
    const double item_spans = (double)g.max_items * (double)s.pspans / (double)s.nlist;
    const IvfParts parts = ivf_part_spans(opt, s.max_pspans, g.max_items,
                                          (int)std::min<double>(8.0 * spans_512, std::max<double>(spans_512, std::floor(item_spans / 1536.0))), 1);
    if (s.tps != 16) return ivf_launch_of(ScanFamily::ivf_kloop, parts, 512, {64, 2, 4, 1});
    const int GROUP = kgroup == 1 ? 1 : kgroup == 2 ? 2 : 4;
    const int RH = g.group == kIvfKloopGroup / 2 ? 2 : 1;           // square tile: 256 rows x 256 slots
    return ivf_launch_of(ScanFamily::ivf_kloop, parts, 512, {16, 2, GROUP, RH});
}

// ---- every instantiation of each family, once ------------------------------------------------------------------------------------
// X(template arguments in the kernel's own order, defaults written out); the flat search's instantiations: scan_plan.hpp
//   scan_kernel<KSTEPS, NWAVES, ST, WPS, BT, ITEMS, G8>: 2 / 4 / 8 waves x bins of 4 / 8 tiles
#define VDB_KERNELS_IVF_SCAN_K(X, K) \
    X(K, 2, 2, 2, 4, true, false) X(K, 2, 2, 2, 8, true, false) X(K, 4, 2, 2, 4, true, false) X(K, 4, 2, 2, 8, true, false) \
    X(K, 8, 2, 2, 4, true, false) X(K, 8, 2, 2, 8, true, false)
#define VDB_KERNELS_IVF_SCAN(X) VDB_KERNELS_IVF_SCAN_K(X, 4) VDB_KERNELS_IVF_SCAN_K(X, 8)

//   scan_i8_kernel<KS, ST, CB, NWAVES, BT, ITEMS, G, TB, RING, AUX>: octs on ring 4 | quads on rings 2, 8, 4
#define VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, NW, BT) \
    X(KS, ST, 2, NW, BT, true, 8, 0, 4, 0) X(KS, ST, 2, NW, BT, true, 4, 0, 2, 0) X(KS, ST, 2, NW, BT, true, 4, 0, 8, 0) \
    X(KS, ST, 2, NW, BT, true, 4, 0, 4, 0)
#define VDB_KERNELS_IVF_SCAN_I8_K(X, KS, ST) \
    VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, 2, 4) VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, 4, 4) VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, 8, 4) \
    VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, 2, 8) VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, 4, 8) VDB_KERNELS_IVF_SCAN_I8_F(X, KS, ST, 8, 8)
#define VDB_KERNELS_IVF_SCAN_I8(X) VDB_KERNELS_IVF_SCAN_I8_K(X, 2, 4) VDB_KERNELS_IVF_SCAN_I8_K(X, 4, 2)

//   ivf_kloop_scan_kernel<TPS, BS, GROUP, RH>: the square tile | 128 x 512 on 256-row spans | on 1024-row spans
#define VDB_KERNELS_IVF_KLOOP(X) X(16, 2, 1, 2) X(16, 2, 2, 2) X(16, 2, 4, 2) X(16, 2, 1, 1) X(16, 2, 2, 1) X(16, 2, 4, 1) X(64, 2, 4, 1)

constexpr ScanKey kKeysIvfScan[] = {VDB_KERNELS_IVF_SCAN(VDB_SCAN_KEY)};
constexpr ScanKey kKeysIvfScanI8[] = {VDB_KERNELS_IVF_SCAN_I8(VDB_SCAN_KEY)};
constexpr ScanKey kKeysIvfKloop[] = {VDB_KERNELS_IVF_KLOOP(VDB_SCAN_KEY)};

}  // namespace vdb

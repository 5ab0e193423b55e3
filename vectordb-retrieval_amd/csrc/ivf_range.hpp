// ivf_range.hpp -- kernels of the range search on IVF-Flat indexes (vdb_ivf_range_search; host side: ivf_range.inc; rules:
// ivf_range_plan.hpp).
//
// The answer is "every row of the query's probed lists within `radius`", exactly, in list order.  What the flat range search does
// with a scan of its own (range.hpp) the list-major scans of the IVF search already leave behind: per (query slot, bin) the nm
// smallest quad minima, each carrying its quad number.  With a radius there is no tau to find:
//   mark     every kept minimum <= thr[q] names a candidate quad; a bin whose nm kept minima all pass is a candidate as a whole
//            (quads that were not kept may pass too).  A superset of the answer, without capacities.  thr[q] carries the bound
//            eps[q] of the list scans, whose pack_err term (query_eps_body, prep.hpp) is the six mantissa bits a kept minimum
//            gives up for its quad number: the packed values are compared as they are.
//   filter / prefix / lims / emit   those of range.hpp over list-order rows; the emit writes ivf_ids[row].
// The candidate bitmap is [query][list-order row / 32] with the flat pitch range_words(N).  A wave owns its query's bitmap row; lists
// are not word aligned and two lanes may mark the same word, so the marks are vector atomic ORs into a row cleared beforehand.
#pragma once
#include "common.hpp"
#include "ivf_mfma.hpp"
#include "ivf_range_plan.hpp"
#include "range.hpp"

namespace vdb {

// bits of rows [r0, r1) of one bitmap row
__device__ __forceinline__ void ivf_range_or_rows(unsigned *brow, int r0, int r1) {
    if (r1 <= r0) return;
    for (int w = r0 >> 5; w <= (r1 - 1) >> 5; ++w) {
        const int lo = max(r0 - w * 32, 0), hi = min(r1 - w * 32, 32);
        const unsigned m = (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
        atomicOr(brow + w, m);
    }
}

struct IvfRangeMarkArgs {
    const float *bin_m[kIvfMaxMinima];   // as IvfSelectArgs
    int nm;
    const float *thr;             // [nq] range_thr_kernel
    const int *flag;              // [nq] 1: every probed row is a candidate (already counted)
    const IvfPlan *plan;
    const int64_t *probes;        // [nq][nprobe]
    const int64_t *offsets;       // [nlist + 1] list-order rows of every list
    const int32_t *slot_of, *slot_off, *list_item0, *item_bin0, *list_pspan0, *span_row0, *span_valid;
    int64_t nq, N, W;
    int nprobe, nlist, group, max_entries, probe_cap;
    int group_rows;               // rows per quad: 4, K-loop scan on 64-row bins 1 / 2 / 4
    int bins_per_span, bin_rows, run_groups;      // as IvfSelectArgs
    int fill;                     // 1: the exact route -- no scan ran, every probed row is marked, nothing but probes / offsets is read
    unsigned *bitmap;             // [nq][W], cleared
    unsigned long long *stat;     // sharded counters: [1] += fallback queries found here
};

// every row of the query's probed lists: lanes take the probes 64 at a time, then stride over the words of each list
__device__ __forceinline__ void ivf_range_fill_query(const IvfRangeMarkArgs &a, int64_t q, unsigned *brow, int lane) {
    for (int p0 = 0; p0 < a.nprobe; p0 += 64) {
        const int p = p0 + lane;
        int lo = 0, hi = 0;
        if (p < a.nprobe) {
            const int64_t l = a.probes[(size_t)q * a.nprobe + p];
            if (l >= 0 && l < a.nlist) {
                lo = (int)a.offsets[l];
                hi = (int)min(a.offsets[l + 1], a.N);
            }
        }
        const int np = min(64, a.nprobe - p0);
        for (int j = 0; j < np; ++j) {
            const int r0 = __shfl(lo, j), r1 = __shfl(hi, j);
            if (r1 <= r0) continue;
            for (int w = (r0 >> 5) + lane; w <= (r1 - 1) >> 5; w += 64) {
                const int b0 = max(r0 - w * 32, 0), b1 = min(r1 - w * 32, 32);
                atomicOr(brow + w, (b1 >= 32 ? 0xffffffffu : ((1u << b1) - 1u)) & ~((1u << b0) - 1u));
            }
        }
    }
}

// one wave per query, two per workgroup.  Phase 1 is ivf_select_kernel's: lane p resolves probe p, a wave prefix sum lays the
// probes' bins out as one entry range.  Then lanes stride over the entries with four loads of the first minimum in flight; an
// entry that passes reads its other minima and marks its quads or its whole bin.
// 32-bit words of LDS per wave: ivf_range_mark_lds_words(nprobe)
__global__ __launch_bounds__(128) void ivf_range_mark_kernel(IvfRangeMarkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_range_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 2 + wave));
    if (q >= a.nq) return;
    unsigned *brow = a.bitmap + (size_t)q * a.W;
    if (a.fill) {
        ivf_range_fill_query(a, q, brow, lane);
        return;
    }
    int *p_off = reinterpret_cast<int *>(ivf_range_smem) + (size_t)wave * (4 * (size_t)a.probe_cap + 64);
    unsigned *p_base_lo = reinterpret_cast<unsigned *>(p_off + a.probe_cap + 32);
    unsigned *p_base_hi = p_base_lo + a.probe_cap;
    int *p_list = reinterpret_cast<int *>(p_base_hi + a.probe_cap);
    const bool flagged = a.flag[q] != 0;
    bool fb = flagged || a.plan->overflow || a.nprobe > kIvfMaxProbes;
    int E = 0;
    if (!fb) {
        for (int p0 = 0; p0 < a.nprobe; p0 += 64) {
            const int p = p0 + lane;
            int nb = 0, lst = -1;
            size_t base = 0;
            if (p < a.nprobe) {
                const int64_t l = a.probes[(size_t)q * a.nprobe + p];
                const int slot = a.slot_of[(size_t)q * a.nprobe + p];
                if (l >= 0 && slot >= 0) {
                    const int rel = slot - a.slot_off[l];
                    const int item = a.list_item0[l] + rel / a.group, col = rel % a.group;
                    nb = ivf_bins_of_list(a.list_pspan0[l + 1] - a.list_pspan0[l], a.bins_per_span, a.run_groups);
                    base = (size_t)a.item_bin0[item] * a.group + (size_t)col * nb;
                    lst = (int)l;
                }
            }
            int incl = nb;                                  // inclusive wave prefix sum of nb
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            if (p < a.nprobe) {
                p_off[p] = E + incl - nb;
                p_base_lo[p] = (unsigned)base;
                p_base_hi[p] = (unsigned)(base >> 32);
                p_list[p] = lst;
            }
            E += __shfl(incl, 63);
        }
        if (lane == 0) p_off[a.nprobe] = E;
        if (E > a.max_entries) fb = true;
    }
    if (fb) {
        ivf_range_fill_query(a, q, brow, lane);
        if (lane == 0 && !flagged) stat_add(a.stat, q, 1, 1ull);
        return;
    }
    const float thr = a.thr[q];
    auto probe_of = [&](int e) {              // largest p with p_off[p] <= e  (p_off is non-decreasing)
        int lo = 0, hi = a.nprobe;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (p_off[mid] <= e) lo = mid; else hi = mid;
        }
        return lo;
    };
    int pcur = lane < E ? probe_of(lane) : 0;
    auto advance = [&](int e) {               // (a lane's entries ascend: its probe only moves forward; p_off[nprobe] = E ends the walk)
        while (p_off[pcur + 1] <= e) ++pcur;
        return pcur;
    };
    for (int e0 = lane; e0 < E; e0 += 256) {
        float raw[4];
        int pv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 64 * u;
            raw[u] = __builtin_inff();
            pv[u] = 0;
            if (e < E) {
                pv[u] = advance(e);
                const size_t base = ((size_t)p_base_hi[pv[u]] << 32) | p_base_lo[pv[u]];
                raw[u] = a.bin_m[0][base + (e - p_off[pv[u]])];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 64 * u;
            if (!(e < E && raw[u] <= thr)) continue;
            const int p = pv[u], ei = e - p_off[p], l = p_list[p];
            const size_t base = ((size_t)p_base_hi[p] << 32) | p_base_lo[p];
            float mv[kIvfMaxMinima];
            mv[0] = raw[u];
#pragma unroll
            for (int i = 1; i < kIvfMaxMinima; ++i) mv[i] = i < a.nm ? a.bin_m[i][base + ei] : __builtin_inff();
            int span_local, bin;
            if (a.run_groups) {              // (an entry that passes is never run padding: that holds +inf)
                const int bpg = a.bins_per_span / a.run_groups;
                const int run_len = ((a.list_pspan0[l + 1] - a.list_pspan0[l]) * bpg + 3) & ~3;
                const int grp = ei / run_len, r = ei - grp * run_len;
                span_local = r / bpg;
                bin = grp * bpg + (r - span_local * bpg);
            } else {
                span_local = ei / a.bins_per_span;
                bin = ei - span_local * a.bins_per_span;
            }
            const int pspan = a.list_pspan0[l] + span_local;
            const int row0 = a.span_row0[pspan] + bin * a.bin_rows;
            const int end = a.span_row0[pspan] + a.span_valid[pspan];
            const int row1 = min(row0 + a.bin_rows, end);
            int active = 0;                  // (the minima ascend: the passing ones are a prefix)
#pragma unroll
            for (int i = 0; i < kIvfMaxMinima; ++i) active += (i < a.nm && mv[i] <= thr) ? 1 : 0;
            if (active < a.nm) {
#pragma unroll
                for (int i = 0; i < kIvfMaxMinima - 1; ++i) {
                    if (i >= active) break;
                    const int qr = row0 + (int)(__float_as_uint(mv[i]) & 0x3Fu) * a.group_rows;
                    ivf_range_or_rows(brow, qr, min(qr + a.group_rows, row1));
                }
            } else {
                ivf_range_or_rows(brow, row0, row1);
            }
        }
    }
}

// range_emit_kernel's units over list-order rows: the id of row r is ids[r]
__global__ __launch_bounds__(256) void ivf_range_emit_kernel(RangeTailArgs a) { range_emit_body<true>(a); }

}  // namespace vdb

// lsh_select.hpp -- the counting top-c select behind sign-LSH (lsh.hpp) and hash-table LSH (lsh_tables.hpp) (gfx950 only).
// Host side: lsh.inc (lsh_candidates_core).
//
// Every (row, query) pair has an integer score in [0, hb), smaller is nearer, or no score at all (-1: the pair is dropped at
// once).  The candidates of a query are its scored rows smallest under (score, row), the first `want` of them (fewer when
// fewer rows have a score); since scores are small integers the cut is found by counting.  Per query
//   1. sample kernel          histogram of a row sample (128 runs of 256 rows) -> t_hi, a generous upper bound of the cut score
//                             (the whole corpus when it is no larger than the sample: the histogram is exact, step 2 is skipped)
//   2. scan kernel, MODE 0    every (query, row) pair: the rare pairs with score <= t_hi count into hist[q][score] and are
//                             appended to the query's list as (score << 32 | row), as far as the list has room
//   3. lsh_threshold_kernel   t = the smallest score at which the cumulative count reaches `want`; m = that count; c = want.
//                             When the bound is the largest score every scored row was counted, and a query with fewer than
//                             `want` of them takes them all: c = m = that count, its tail padding.  Three routes:
//                             complete -- every counted pair fitted the list, which therefore holds the m rows up to t;
//                             rescan   -- the list overflowed (or step 2 was skipped) but m fits: the list restarts empty;
//                             flagged  -- t_hi was too small (fewer than `want` rows counted) or m exceeds the list (ties at t)
//   4. scan kernel, MODE 1    the same scan for the `rescan` queries only, appending the m pairs with score <= t (workgroups
//                             none of whose queries is one return at once)
//   5. lsh_select_kernel      sorts the entries with score <= t (bitonic; compacted into LDS up to 4096 of them, else in place)
//                             and emits the first c; a flagged query first takes the exact fallback: full histogram of its
//                             scores -> c, t, then the rows below t and the lowest-id rows at t (ordered compaction): exactly
//                             c entries.  A query with c = 0 enters the list of empty queries, where the call keeps one.
//
// Steps 1, 2 and 4 keep rows in registers and score them against query words in LDS, and there the two kinds differ in
// everything but the bookkeeping (words per row, rows per thread, query tile, the score itself), so each kind has a sample
// and a scan kernel of its own over these args: lsh_sample_kernel<WP> / lsh_scan_kernel<MODE, WP> in lsh.hpp,
// lsht_sample_kernel<WP, TMAX> / lsht_scan_kernel<MODE, WP, TMAX> in lsh_tables.hpp.  Steps 3 and 5 are the kernels below, one
// of each in the source: the select scores from memory, on the flagged path only (lsh_score_mem), and is compiled once per kind
// (VOTES = a.T > 0), which picks the score there and what it emits.
#pragma once
#include "common.hpp"

namespace vdb {

constexpr int kLshMaxBits = 1024;      // scores lie in [0, kLshMaxBits]
constexpr int kLshMaxCand = 65536;
constexpr int kLshtMaxWords = 128;     // hash-table LSH: T * (words per table of the contract); stored rows have at most 64 more
constexpr int kLshSampleMax = 32768;   // rows of the threshold sample (a multiple of 256)
constexpr int kLshSampleQ = 4;         // queries per workgroup of the sample kernel
constexpr int kLshSortLds = 4096;      // list entries sorted in LDS

struct LshSelArgs {
    const uint32_t *codes;       // [n][kw]
    const uint32_t *qcodes;      // [nq][kw]
    int64_t n, nq, q_base;       // q_base: number of the chunk's first query within the call's batch (empty_list holds q_base + q)
    int kw, T, wp;               // words per row; hash tables: T tables of wp words (sign codes: T = 0)
    int hb;                      // histogram bins per query: scores lie in [0, hb)
    int want, ncand;             // candidates wanted per query (sign codes: min(ncand, n); hash tables: ncand); width of the output rows
    int cap, qtile;              // list entries per query (a power of two); queries per scan workgroup
    int64_t sample_n, sample_stride;
    int force_fallback;
    int64_t id_base;
    int *hist;                   // [nq][hb]
    int *thi, *tq, *cnt, *flag, *tsel, *msel, *csel;  // [nq] each: upper bound, cut for MODE 1 (-1: none), list fill, fallback flag, cut, rows up to it, candidates
    int scanned0;                // the MODE 0 scan ran (the corpus is larger than the sample)
    unsigned long long *list;    // [nq][cap]
    unsigned long long *stat;    // sharded counters: 0 flagged queries, 1 candidates, 2 empty queries listed
    int32_t *empty_list, *empty_count;    // (null: the call lists no empty queries)
    int32_t *out_score;          // [nq][ncand]: Hamming distances (padding 0x7fffffff) | votes (padding 0)
    int64_t *out_ids;            // (padding -1)
};

__device__ __forceinline__ int lsh_ham(const uint32_t *__restrict__ a, const uint32_t *b, int wp) {
    int d = 0;
    for (int w = 0; w < wp; ++w) d += __popc(a[w] ^ b[w]);
    return d;
}

// class (T - votes) T + first of a (row, query) pair of table keys, -1 without a vote (lsh_tables.hpp)
__device__ __forceinline__ int lsht_class_mem(const uint32_t *__restrict__ row, const uint32_t *q, int T, int wp) {
    int votes = 0, first = 0;
    for (int t = 0; t < T; ++t) {
        uint32_t diff = 0;
        for (int w = 0; w < wp; ++w) diff |= row[t * wp + w] ^ q[t * wp + w];
        if (diff == 0) {
            if (votes == 0) first = t;
            ++votes;
        }
    }
    return votes ? (T - votes) * T + first : -1;
}

template <bool VOTES>
__device__ __forceinline__ int lsh_score_mem(const LshSelArgs &a, const uint32_t *__restrict__ row, const uint32_t *q) {
    return VOTES ? lsht_class_mem(row, q, a.T, a.wp) : lsh_ham(row, q, a.kw);
}

// one thread per query: its candidates c, the cut t, the rows m up to it, and which route the query takes
__global__ __launch_bounds__(256) void lsh_threshold_kernel(LshSelArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nq) return;
    const int *hq = a.hist + (size_t)q * a.hb;
    const int thi = a.thi[q];
    long long cum = 0, m = 0;
    int t = -1, c = a.want;
    for (int d = 0; d <= thi; ++d) {
        cum += hq[d];
        if (t < 0 && cum >= a.want) { t = d; m = cum; }
    }
    bool flagged = a.force_fallback != 0;
    if (t < 0) {
        if (thi == a.hb - 1) {         // every scored row was counted and they are fewer than wanted: all of them
            t = thi;                   // (sign codes: every row has a score and want <= n, so this cannot happen)
            m = cum;
            c = (int)cum;
        } else {
            flagged = true;
        }
    }
    if (m > a.cap) flagged = true;
    // MODE 0 appended every pair it counted: if they all fitted, the list already holds the m rows up to t (and a few beyond)
    const bool complete = !flagged && a.scanned0 && cum <= a.cap;
    a.flag[q] = flagged ? 1 : 0;
    a.tq[q] = (flagged || complete) ? -1 : t;
    a.tsel[q] = t;
    a.msel[q] = (int)m;
    a.csel[q] = c;
    if (!complete) a.cnt[q] = 0;
    if (flagged) stat_add(a.stat, q, 0, 1ull);
}

// one workgroup per query: (flagged: exact fallback ->) sort the list -> emit.  VOTES: the score and the emit of the hash tables
// (a.T > 0); compiled for each kind, since a switch inside the two row walks of the fallback cost the hash tables 1 ms in 37.
template <bool VOTES>
__global__ __launch_bounds__(256) void lsh_select_kernel(LshSelArgs a) {
    __shared__ unsigned long long sbuf[kLshSortLds];
    __shared__ int sh[kLshMaxBits + 1];
    __shared__ uint32_t qc[kLshtMaxWords + 64];
    __shared__ int s_t, s_below, s_c, s_fill, wtot[4];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *lq = a.list + (size_t)q * a.cap;
    int n = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;      // list entries: the m rows up to the cut, and after MODE 0 a few beyond it
    int t_cut = a.tsel[q], m = a.msel[q], c = a.csel[q];
    if (tid == 0) s_fill = 0;
    if (a.flag[q]) {       // (uniform over the workgroup)
        for (int i = tid; i < a.hb; i += 256) sh[i] = 0;
        if (tid < a.kw) qc[tid] = a.qcodes[(size_t)q * a.kw + tid];
        __syncthreads();
        for (int64_t r = tid; r < a.n; r += 256) {
            const int s = lsh_score_mem<VOTES>(a, a.codes + (size_t)r * a.kw, qc);
            if (s >= 0) atomicAdd(&sh[s], 1);
        }
        __syncthreads();
        if (tid == 0) {
            long long total = 0;
            for (int d = 0; d < a.hb; ++d) total += sh[d];
            const int cc = (int)(total < a.ncand ? total : (long long)a.ncand);
            long long cum = 0;
            int t = a.hb - 1;
            for (int d = 0; d < a.hb; ++d) {
                if (cum + sh[d] >= cc) { t = d; break; }
                cum += sh[d];
            }
            s_t = t;
            s_below = (int)cum;
            s_c = cc;
        }
        __syncthreads();
        c = s_c;
        const int t = s_t, below = s_below, need = c - below;
        int taken = 0;          // rows with score t seen so far (uniform)
        for (int64_t base = 0; base < a.n; base += 256) {
            const int64_t r = base + tid;
            int d = 0x7fffffff;
            if (r < a.n) {
                const int s = lsh_score_mem<VOTES>(a, a.codes + (size_t)r * a.kw, qc);
                if (s >= 0) d = s;
            }
            if (d < t) lq[atomicAdd(&s_fill, 1)] = ((unsigned long long)d << 32) | (unsigned long long)r;
            const bool tie = d == t;
            const unsigned long long mask = __ballot(tie);
            if (lane == 0) wtot[wave] = __popcll(mask);
            __syncthreads();
            int pos = taken + __popcll(mask & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) pos += wtot[w];
            if (tie && pos < need) lq[below + pos] = ((unsigned long long)d << 32) | (unsigned long long)r;
            taken += wtot[0] + wtot[1] + wtot[2] + wtot[3];
            __syncthreads();
        }
        n = m = c;
        t_cut = 0x7fffffff;
        __syncthreads();
        if (tid == 0) s_fill = 0;
    }
    __syncthreads();
    // the m entries with score <= t_cut: compacted into LDS when they fit, else sorted in place with the others blanked
    int P = 1;
    unsigned long long *buf = lq;
    if (m <= kLshSortLds) {
        buf = sbuf;
        while (P < m) P <<= 1;
        for (int i = tid; i < n; i += 256) {
            const unsigned long long key = lq[i];
            if ((int)(key >> 32) <= t_cut) buf[atomicAdd(&s_fill, 1)] = key;
        }
        for (int i = m + tid; i < P; i += 256) buf[i] = ~0ull;
    } else {
        while (P < n) P <<= 1;
        for (int i = tid; i < P; i += 256)
            if (i >= n || (int)(lq[i] >> 32) > t_cut) buf[i] = ~0ull;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = buf[i], y = buf[ixj];
                    if ((x > y) == ((i & k) == 0)) {
                        buf[i] = y;
                        buf[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    // sign codes: (distance, id); hash tables: (votes, id) with votes = T - class / T
    int32_t *os = a.out_score + (size_t)q * a.ncand;
    int64_t *oi = a.out_ids + (size_t)q * a.ncand;
    for (int i = tid; i < a.ncand; i += 256) {
        if (i < c) {
            const unsigned long long key = buf[i];
            const int32_t s = (int32_t)(key >> 32);
            os[i] = VOTES ? a.T - s / a.T : s;
            oi[i] = a.id_base + (int64_t)(key & 0xffffffffull);
        } else {
            os[i] = VOTES ? 0 : 0x7fffffff;
            oi[i] = -1;
        }
    }
    if (tid == 0) {
        stat_add(a.stat, q, 1, (unsigned long long)c);
        if (c == 0 && a.empty_list) {
            a.empty_list[atomicAdd(a.empty_count, 1)] = (int32_t)(a.q_base + q);
            stat_add(a.stat, q, 2, 1ull);
        }
    }
}

}  // namespace vdb

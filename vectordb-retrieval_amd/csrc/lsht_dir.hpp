// lsht_dir.hpp -- hash-table LSH, option "lsht_directory": the per-table bucket directory and the lookup kernels that take the place of
// the two vote scans of the counting select (gfx950 only).  Rules: lsht_dir_plan.hpp; host side: lsh_tables.inc.
//
// Directory (device, one buffer): offsets[T][S + 1] then rows[T][N], int32.  Bucket `slot` of table t holds the rows whose table key
// hashes to it, rows[t][offsets[t][slot] .. offsets[t][slot + 1]), in no particular order (the select orders candidates by
// (class, id) itself).  Built whole behind the keys of every add -- a CSR has no room to grow, an incremental directory is out of
// scope -- by four kernels, no library:
//   count   one thread per (row, table): atomicAdd on the slot's cursor
//   scan    one workgroup per table walks its S cursors 1024 at a time: a wave scan by lane shuffles, the four wave totals through
//           LDS, and a carry in a register from step to step (a workgroup-level scan with a carry: S counts of a table take
//           S / 1024 dependent steps, which 32 tables at most share out over 32 CUs; the build is not the hot path).  Leaves the
//           exclusive prefix in the offsets and in the cursors
//   fill    one thread per (row, table): its place is atomicAdd on the slot's cursor
//   stats   visits = sum over tables and slots of count^2 (read back once per build: the routing rule)
// The cursors (T S int32) are a temporary of the build.
//
// Lookup, lsht_lookup_kernel<MODE, WP>: grid (nq, splits), a workgroup serves one query.  Its T WP key words sit in LDS; T threads
// hash them and read the T slot ranges once; the T buckets then form one run of `total` entries, of which workgroup (q, s) takes
// the 256-entry steps s, s + splits, ...: a giant bucket is spread over `splits` workgroups, and 24 buckets of 15 entries fill two
// steps, not 24.  A lane takes an entry (t, row), gathers the row's WP key words of table t and drops the entry if they differ from
// the query's (a slot shared by different keys).  On a hit it reads the row's other keys -- the tables below t first: a match
// there means the row is also in that earlier bucket, whose lane emits it, so this lane leaves; then the tables above t for the
// votes.  So a pair is emitted by the lane of its first colliding table alone: the emitted pairs are exactly those of the vote
// scan, each once, with no dedupe pass, and the bookkeeping (lsht_emit) is the scan's own.  Nothing is indexed dynamically in
// registers: no scratch.
#pragma once
#include "common.hpp"
#include "lsh_select.hpp"
#include "lsh_tables.hpp"
#include "lsht_dir_plan.hpp"

namespace vdb {

struct LshtDirArgs {
    const uint32_t *keys;        // [n][kw]
    int64_t n, S;                // rows, slots per table
    int T, W, wp, kw;            // tables, key words per table of the contract (hashed) and as stored, words per row
    int *cursor;                 // [T][S]: counts, then the next free place of every slot
    int *off;                    // [T][S + 1]
    int *rows;                   // [T][n]
    unsigned long long *visits;
};

template <bool FILL>
__global__ __launch_bounds__(256) void lsht_dir_place_kernel(LshtDirArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n * a.T) return;
    const int64_t r = i / a.T;
    const int t = (int)(i - r * a.T);
    const uint32_t slot = lsht_dir_hash(a.keys + (size_t)r * a.kw + (size_t)t * a.wp, a.W) & (uint32_t)(a.S - 1);
    const int pos = atomicAdd(&a.cursor[(size_t)t * a.S + slot], 1);
    if (FILL && (int64_t)pos < a.n) a.rows[(size_t)t * a.n + pos] = (int)r;
}

__global__ __launch_bounds__(256) void lsht_dir_scan_kernel(LshtDirArgs a) {
    __shared__ int wsum[4];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *cur = a.cursor + (size_t)t * a.S;
    int *off = a.off + (size_t)t * (a.S + 1);
    int carry = 0;
    for (int64_t base = 0; base < a.S; base += 1024) {      // (S is a multiple of 1024)
        const int4 c = *reinterpret_cast<const int4 *>(cur + base + tid * 4);
        const int s = c.x + c.y + c.z + c.w;
        int incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry + incl - s;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
        const int4 o = make_int4(before, before + c.x, before + c.x + c.y, before + c.x + c.y + c.z);
        *reinterpret_cast<int4 *>(cur + base + tid * 4) = o;
        int *dst = off + base + tid * 4;          // (a table's offsets start at any word: four scalar stores)
        dst[0] = o.x;
        dst[1] = o.y;
        dst[2] = o.z;
        dst[3] = o.w;
    }
    if (tid == 0) off[a.S] = carry;
}

__global__ __launch_bounds__(256) void lsht_dir_stats_kernel(LshtDirArgs a) {
    __shared__ unsigned long long total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned long long mine = 0;
    const int64_t slots = (int64_t)a.T * a.S;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i / a.S, slot = i - t * a.S;
        const int *off = a.off + (size_t)t * (a.S + 1) + slot;
        const unsigned long long c = (unsigned long long)(off[1] - off[0]);
        mine += c * c;
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(a.visits, total);
}

// do the WP words of table t agree?  (row: global, q: LDS)
template <int WP>
__device__ __forceinline__ bool lsht_table_equal(const uint32_t *__restrict__ row, const uint32_t *q, int t) {
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < WP; ++w) diff |= row[t * WP + w] ^ q[t * WP + w];
    return diff == 0;
}

// MODE 0 / MODE 1 as lsht_scan_kernel: the bound is thi (every query) | tq (the rescan queries; the others leave at once)
template <int MODE, int WP>
__global__ __launch_bounds__(kLshtDirThreads) void lsht_lookup_kernel(LshSelArgs a) {
    __shared__ uint32_t qc[kLshtMaxWords + 64];
    __shared__ int b_start[kLshtMaxTables];
    __shared__ long long b_pre[kLshtMaxTables + 1];      // entries of the buckets below table t
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, T = a.T;
    const int bound = (MODE == 0 ? a.thi : a.tq)[q];
    if (bound < 0) return;                                // (uniform)
    if (tid < a.kw) qc[tid] = a.qcodes[(size_t)q * a.kw + tid];
    __syncthreads();
    if (tid < T) {
        const uint32_t slot = lsht_dir_hash(qc + tid * WP, a.dir_w) & (uint32_t)(a.dir_slots - 1);
        const int *off = a.dir_off + (size_t)tid * (a.dir_slots + 1) + slot;
        b_start[tid] = off[0];
        b_pre[tid + 1] = off[1] - off[0];
    }
    __syncthreads();
    if (tid == 0) {
        b_pre[0] = 0;
        for (int t = 0; t < T; ++t) b_pre[t + 1] += b_pre[t];
    }
    __syncthreads();
    const long long total = b_pre[T];
    const long long step = (long long)gridDim.y * kLshtDirThreads;
    for (long long base = (long long)blockIdx.y * kLshtDirThreads; base < total; base += step) {
        const long long i = base + tid;
        if (i >= total) continue;
        int t = 0;
        while (i >= b_pre[t + 1]) ++t;
        const int64_t r = a.dir_rows[(size_t)t * a.n + b_start[t] + (i - b_pre[t])];
        const uint32_t *row = a.codes + (size_t)r * a.kw;
        if (!lsht_table_equal<WP>(row, qc, t)) continue;          // another key in the same slot
        bool earlier = false;
        for (int u = 0; u < t && !earlier; ++u) earlier = lsht_table_equal<WP>(row, qc, u);
        if (earlier) continue;                                    // the lane of that table's bucket has the pair
        int votes = 1;
        for (int u = t + 1; u < T; ++u) votes += lsht_table_equal<WP>(row, qc, u) ? 1 : 0;
        const int cl = (T - votes) * T + t;
        if (cl <= bound) lsht_emit<MODE>(a, q, cl, r);
    }
    if (tid == 0) {       // entries this workgroup walked: its 256-entry steps of the run, the last one short
        const long long steps = (total + kLshtDirThreads - 1) / kLshtDirThreads, y = blockIdx.y, g = gridDim.y;
        long long walked = steps > y ? ((steps - 1 - y) / g + 1) * kLshtDirThreads : 0;
        if (steps > y && (steps - 1) % g == y) walked -= steps * kLshtDirThreads - total;
        if (walked) stat_add(a.stat, q, 3, (unsigned long long)walked);
    }
}

}  // namespace vdb

// filter.hpp -- kernels of the filtered k-NN search (vdb_filter_set / vdb_search_filtered; host side: filter.inc; rules:
// filter_plan.hpp).
//
// An installed filter is an allow bitmap over rows (bit r % 32 of word r / 32, the layout of range.hpp) and what is derived from it:
//   install     one pass writes the handle's own copy of the words (tail masked by row number), masked copies of the scans'
//               accumulator inits -- bias_f[r] = allowed ? bias[r] : kPadBias, both windows of bias8_f likewise with kI8PadBias --
//               and counts the admitted rows.  Every MFMA scan reads an init of 0.9e38 or more as the pad marker and never lets the
//               row reach a bin minimum, so the scans filter their candidates without a change: they are handed the copies.
//   exact       every exact stage tests the bit where it forms its per-row `valid` flag (row_allowed, refine.hpp).
//   sparse      selective filters: the admitted rows are compacted into an ascending list at install (segment counts, prefix, emit
//               in bit order -- no atomics, as range_seg_prefix_kernel / range_emit_kernel do it) and filter_rows_kernel scores the
//               list alone, query-blocked like refine_full_blocked_kernel.
#pragma once
#include "common.hpp"
#include "filter_plan.hpp"
#include "refine.hpp"
#include "topk.hpp"

namespace vdb {

typedef int filter_int4 __attribute__((ext_vector_type(4)));

struct FilterInstallArgs {
    const uint32_t *words_in;    // the caller's words: filter_words_in(N) of them
    int64_t N, Npad, W_in;       // W_in = filter_words_in(N)
    uint32_t *words;             // [Npad / 32] the handle's copy: bits of rows >= N cleared
    const float *bias;           // [Npad] or nullptr (a handle that builds no bias)
    float *bias_f;
    const int32_t *bias8;        // [2][Npad] or nullptr (no int8 copy)
    int32_t *bias8_f;
    unsigned long long *count;   // [1], zero on entry: += admitted rows, one atomic per workgroup
};

// one thread per 4 consecutive rows (16-byte loads and stores of the inits); the lane that owns the first rows of a word also
// stores the word and counts its bits
__global__ __launch_bounds__(256) void filter_install_kernel(FilterInstallArgs a) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t * 4;
    int cnt = 0;
    if (row < a.Npad) {
        const int64_t w = row >> 5;
        uint32_t word = w < a.W_in ? a.words_in[w] : 0u;
        const int64_t left = a.N - w * kRangeWordBits;                 // filter_word_mask on the device
        word &= left >= kRangeWordBits ? 0xffffffffu : left <= 0 ? 0u : ((1u << (int)left) - 1u);
        if ((row & 31) == 0) {
            a.words[w] = word;
            cnt = __popc(word);
        }
        const uint32_t bits = (word >> (row & 31)) & 15u;
        if (a.bias) {
            float4 b = *reinterpret_cast<const float4 *>(a.bias + row);
            if (!(bits & 1u)) b.x = kPadBias;
            if (!(bits & 2u)) b.y = kPadBias;
            if (!(bits & 4u)) b.z = kPadBias;
            if (!(bits & 8u)) b.w = kPadBias;
            *reinterpret_cast<float4 *>(a.bias_f + row) = b;
        }
        if (a.bias8) {
#pragma unroll
            for (int win = 0; win < 2; ++win) {
                filter_int4 b = *reinterpret_cast<const filter_int4 *>(a.bias8 + (size_t)win * a.Npad + row);
                if (!(bits & 1u)) b.x = kI8PadBias;
                if (!(bits & 2u)) b.y = kI8PadBias;
                if (!(bits & 4u)) b.z = kI8PadBias;
                if (!(bits & 8u)) b.w = kI8PadBias;
                *reinterpret_cast<filter_int4 *>(a.bias8_f + (size_t)win * a.Npad + row) = b;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(a.count, (unsigned long long)total);
    }
}

// ---- the ascending list of admitted rows ---------------------------------------------------------------------------------------
struct FilterListArgs {
    const uint32_t *words;       // [W] the handle's copy (tail clean)
    int64_t W;
    int S;                       // segments of kFilterSegWords words
    int *seg;                    // [S]: admitted rows per segment (count), then their exclusive prefix (prefix)
    int32_t *list;               // [n_allowed]
};

// one wave per segment, one word per lane
__global__ __launch_bounds__(256) void filter_seg_count_kernel(FilterListArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int64_t w = s * kFilterSegWords + lane;
    int cnt = w < a.W ? __popc(a.words[w]) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) a.seg[s] = cnt;
}

// one workgroup: exclusive prefix over the segments, in place (a thread sums a contiguous run, thread 0 the 256 runs)
__global__ __launch_bounds__(256) void filter_seg_prefix_kernel(FilterListArgs a) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int64_t per = ((int64_t)a.S + 255) / 256;
    const int64_t s0 = t * per < a.S ? t * per : a.S, s1 = s0 + per < a.S ? s0 + per : a.S;
    int64_t sum = 0;
    for (int64_t s = s0; s < s1; ++s) sum += a.seg[s];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t s = s0; s < s1; ++s) {
        const int v = a.seg[s];
        a.seg[s] = (int)run;
        run += v;
    }
}

// the count kernel's units once more: the rows of a word are written behind those of the lanes (words) before it
__global__ __launch_bounds__(256) void filter_emit_kernel(FilterListArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int64_t w = s * kFilterSegWords + lane;
    const uint32_t word = w < a.W ? a.words[w] : 0u;
    if (__ballot(word != 0u) == 0ull) return;
    const int n = __popc(word);
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    int64_t out = (int64_t)a.seg[s] + (inc - n);
    for (uint32_t m = word; m; m &= m - 1u) a.list[out++] = (int32_t)(w * kRangeWordBits + (__ffs((int)m) - 1));
}

// ---- sparse route: exact top-k over the listed rows ----------------------------------------------------------------------------
struct FilterRowsArgs {
    RefineCommon c;              // c.Q: the queries padded to D4
    const int32_t *list;         // [n] admitted rows, ascending
    int64_t n;
    int64_t nq;
    int S;                       // splits of the list per query
    int64_t per_split;           // list entries per split, a multiple of 64
    // S == 1 and D != nullptr: final rows; else partial rows [query][S][k] for merge_kernel
    float *D;
    int64_t *I;
    double *pkeys;
    int64_t *pids;
};

// One wave owns QB consecutive queries and one split of the list; every listed row is gathered ONCE for the QB queries, each query
// keeps its own sequential chain (exact_keys, refine.hpp), so the keys are those of row_key bit for bit.  QB == 1: row_key itself.
template <int KPL, int QB>
__global__ __launch_bounds__(256) void filter_rows_kernel(FilterRowsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t waves_total = (int64_t)gridDim.x * 4;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t groups = (a.nq + QB - 1) / QB;
    const int64_t units = groups * a.S;
    for (int64_t u = wave0; u < units; u += waves_total) {
        const int64_t grp = u / a.S;
        const int split = (int)(u - grp * a.S);
        int64_t q[QB];
        const float *qptr[QB];
        WaveTopK<KPL> tk[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            q[j] = grp * QB + j;
            const int64_t qj = q[j] < a.nq ? q[j] : a.nq - 1;          // (padding slots re-score the last query)
            qptr[j] = a.c.Q + (size_t)qj * a.c.D4;
            tk[j].init(a.c.k);
        }
        const int64_t i0 = (int64_t)split * a.per_split;
        int64_t i1 = i0 + a.per_split;
        if (i1 > a.n) i1 = a.n;
        for (int64_t base = i0; base < i1; base += 64) {
            const int64_t i = base + lane;
            const bool valid = i < i1;
            const int64_t row = valid ? (int64_t)a.list[i] : 0;
            uint64_t key[QB];
#pragma unroll
            for (int j = 0; j < QB; ++j) key[j] = ~0ull;
            if (valid) {
                if (QB == 1) {
                    key[0] = row_key<4>(a.c, row, qptr[0]);
                } else if (a.c.X) {
                    exact_keys<QB>(a.c.X + (size_t)row * a.c.D4, qptr, a.c.D4, a.c.metric, key);
                } else {            // int8-only index: the int8 row, once per query (same chains, same keys)
#pragma unroll
                    for (int j = 0; j < QB; ++j)
                        key[j] = exact_key_i8<4>(a.c.X8 + (size_t)row * a.c.x8_pitch, a.c.cx, qptr[j], a.c.D4, a.c.metric);
                }
            }
            const int64_t id = a.c.id_base + row;
#pragma unroll
            for (int j = 0; j < QB; ++j) tk[j].offer(key[j], id, valid);
        }
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            if (q[j] < a.nq) {
                if (a.S == 1 && a.D) {
                    const size_t o = (size_t)q[j] * a.c.k;
                    write_topk<KPL>(tk[j], a.c.metric, a.D + o, a.I + o, nullptr, nullptr);
                } else {
                    const size_t o = (size_t)(q[j] * a.S + split) * a.c.k;
                    write_topk<KPL>(tk[j], a.c.metric, nullptr, nullptr, a.pkeys + o, a.pids + o);
                }
            }
        }
    }
}

}  // namespace vdb

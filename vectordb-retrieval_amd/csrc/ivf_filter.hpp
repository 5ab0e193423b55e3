// ivf_filter.hpp -- install kernels of the filtered k-NN search on IVF-Flat indexes (vdb_ivf_filter_set / vdb_ivf_search_filtered;
// host side: ivf_filter.inc; rules: ivf_filter_plan.hpp).
//
// The caller's allow bitmap is in id order (bit r % 32 of word r / 32 admits the row whose id is id_base + r); the rows of an IVF
// index sit in list order, and the list scans read their accumulator inits over the list-PADDED panel space.  Two passes:
//   rows    one lane per list-order row: gathers the row's bit through ivf_ids (the only irregular access of the install), a wave
//           ballots its 64 rows and two of its lanes store the two list-order words; the admitted rows are counted, one atomic per
//           workgroup.
//   mask    one lane per 4 panel slots: bias_f[i] = allowed ? bias[i] : kPadBias, both windows of bias8_f likewise with kI8PadBias,
//           the bit read from the list-order words the first pass wrote -- consecutive slots are consecutive rows, so every access
//           of this pass is coalesced.
// The list scans then filter their candidates without a change (they read an init of 0.9e38 or more as the pad marker and never let
// the row reach a bin minimum: DESIGN 4.14), and the exact stages test the list-order bit (row_allowed, refine.hpp) through the
// ALLOW instantiations of ivf_scan_kernel / ivf_tail_kernel (ivf.hpp).
#pragma once
#include "common.hpp"
#include "ivf_filter_plan.hpp"

namespace vdb {

typedef int ivf_filter_int4 __attribute__((ext_vector_type(4)));

struct IvfFilterRowsArgs {
    const uint32_t *words_in;    // the caller's words in id order: (N + 31) / 32 of them
    const int64_t *ids;          // [N] ivf_ids: the id of every list-order row
    int64_t N, id_base;
    uint32_t *words;             // [ivf_filter_words(N)] out: list order, bits of rows >= N clear
    unsigned long long *count;   // [1], zero on entry: += admitted rows, one atomic per workgroup
};

__global__ __launch_bounds__(256) void ivf_filter_rows_kernel(IvfFilterRowsArgs a) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (the grid covers whole 64-row units: ivf_filter_words)
    bool on = false;
    if (row < a.N) {
        const int64_t r = a.ids[row] - a.id_base;
        if (r >= 0 && r < a.N) on = (a.words_in[r >> 5] >> (r & 31)) & 1u;
    }
    const unsigned long long m = __ballot(on);
    const int64_t unit = row >> 6;                                        // wave-uniform
    if (unit * kIvfFilterUnitRows < a.N && lane < 2) a.words[unit * 2 + lane] = (uint32_t)(m >> (32 * lane));
    if (lane == 0) part[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(a.count, (unsigned long long)total);
    }
}

struct IvfFilterMaskArgs {
    const uint32_t *words;       // list-order words (ivf_filter_rows_kernel)
    const int32_t *span_row0;    // [pspans] first list-order row of every panel span
    const int32_t *span_valid;   // [pspans] rows of it that exist
    int64_t panel_rows;          // pspans * span_rows
    int span_rows;               // a multiple of 4
    const float *bias;           // [panel_rows]
    float *bias_f;
    const int32_t *bias8;        // [2][panel_rows] or nullptr (no int8 copy of the panel space)
    int32_t *bias8_f;
};

__global__ __launch_bounds__(256) void ivf_filter_mask_kernel(IvfFilterMaskArgs a) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;      // 4 slots of one span
    if (i >= a.panel_rows) return;
    const int64_t span = i / a.span_rows;
    const int local = (int)(i - span * a.span_rows);
    const int valid = a.span_valid[span];
    const int64_t row = (int64_t)a.span_row0[span] + local;
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (local + j < valid) bits |= ((a.words[(row + j) >> 5] >> ((row + j) & 31)) & 1u) << j;
    float4 b = *reinterpret_cast<const float4 *>(a.bias + i);
    if (!(bits & 1u)) b.x = kPadBias;
    if (!(bits & 2u)) b.y = kPadBias;
    if (!(bits & 4u)) b.z = kPadBias;
    if (!(bits & 8u)) b.w = kPadBias;
    *reinterpret_cast<float4 *>(a.bias_f + i) = b;
    if (a.bias8) {
#pragma unroll
        for (int win = 0; win < 2; ++win) {
            ivf_filter_int4 c = *reinterpret_cast<const ivf_filter_int4 *>(a.bias8 + (size_t)win * a.panel_rows + i);
            if (!(bits & 1u)) c.x = kI8PadBias;
            if (!(bits & 2u)) c.y = kI8PadBias;
            if (!(bits & 4u)) c.z = kI8PadBias;
            if (!(bits & 8u)) c.w = kI8PadBias;
            *reinterpret_cast<ivf_filter_int4 *>(a.bias8_f + (size_t)win * a.panel_rows + i) = c;
        }
    }
}

}  // namespace vdb

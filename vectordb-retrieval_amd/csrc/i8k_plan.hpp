// i8k_plan.hpp -- the int8 K-loop scan (scan16_i8.hpp; option "i8_kloop"; byte-valued corpora of D > 128): the key format of a
// handle and the searches the kernel serves.  Plain host C++ (no HIP header, no handle): tests/host/i8k_plan_main.cpp prints
// what the rules give and tests/test_i8k_plan_host.py checks them against brute force.
//
// The key.  A = x - cx, B = cq - q, the accumulator starts from floor(bias / 2) + offset (L2: bias = ||x||^2 - 2 cq sum x; IP:
// the accumulator starts from -cq sum x + offset), so t' = offset + floor(T / 2) with T = sum over the dimensions of
//   L2:  x^2 - 2 x q + 2 cx (q - cq)          IP:  2 (-x q + cx (q - cq))
// -- per dimension a convex quadratic in x and linear in q, so its extremes over a byte window lie at the window's ends (the
// minimum over x also at x = q).  The D <= 128 scan packs (t' << 6) | quad id with the constant offset 2^24 and padding rows at
// 30 000 000: 25 bits of t'.  At D = 768 the range of floor(T / 2) is 50 M wide, so the key is per handle: (offset, shift) from
// these worst-case extremes over Dpad dimensions -- not from the data -- with
//   every real t' in [1, pad),  pad = kI8kPadKey << shift < 2^31  (the accumulator init of padding rows, whose panels are zero),
//   stored key = ((t' >> shift) << 6) | quad id  <  the bits of +inf,   shift the smallest that fits.
// One (offset, shift) serves both QUERY windows of a handle (bias8 holds an accumulator init per query window, the corpus window
// is the handle's): the extremes are taken over both.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace vdb {

constexpr int kI8kPadKey = 30000000;          // (t' >> shift) of a padding row = kI8PadBias of the D <= 128 scan (common.hpp)
constexpr unsigned kI8kInf = 0x7f800000u;     // = kI8Inf
constexpr int kI8kMaxDim = 4096;

struct I8KeyRule {
    int64_t offset = 0;     // added to floor(bias / 2): the smallest real t' is 1
    int shift = 0;          // stored key = ((t' >> shift) << 6) | quad id
    int64_t pad = 0;        // accumulator init of padding rows = kI8kPadKey << shift
    int64_t lo = 0, hi = 0; // worst-case extremes of floor(T / 2)
};

// T's term of one dimension
inline int64_t i8k_term(int metric, int x, int q, int cx, int cq) {
    return metric == 0 ? (int64_t)x * x - 2 * (int64_t)x * q + 2 * (int64_t)cx * (q - cq) : 2 * (-(int64_t)x * q + (int64_t)cx * (q - cq));
}

inline int64_t i8k_floor_half(int64_t v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); }

// cx: the corpus window of the handle (128 = u8 values 0..255, 0 = s8 values -128..127); dpad: D padded to 64
inline I8KeyRule i8k_key_rule(int dpad, int cx, int metric) {
    const int xlo = cx == 128 ? 0 : -128, xhi = xlo + 255;
    int64_t tmin = INT64_MAX, tmax = INT64_MIN;
    for (int w = 0; w < 2; ++w) {             // query window: u8 (cq = 127), s8 (cq = -1)
        const int cq = w == 0 ? 127 : -1, qlo = w == 0 ? 0 : -128, qhi = qlo + 255;
        for (int q : {qlo, qhi})
            for (int x : {xlo, xhi, std::min(xhi, std::max(xlo, q))}) {
                const int64_t t = i8k_term(metric, x, q, cx, cq);
                tmin = std::min(tmin, t);
                tmax = std::max(tmax, t);
            }
    }
    I8KeyRule r;
    r.lo = i8k_floor_half(tmin * dpad);
    r.hi = i8k_floor_half(tmax * dpad);
    r.offset = 1 - r.lo;
    while (r.shift < 6 && r.hi + r.offset >= ((int64_t)kI8kPadKey << r.shift)) ++r.shift;
    r.pad = (int64_t)kI8kPadKey << r.shift;
    return r;
}
// (dpad <= kI8kMaxDim: the u8 corpus window spans 65 025 (IP) or 65 153 (L2, both query windows) per dimension = 267 M at 4096
//  dimensions and takes shift 4; D = 768 takes shift 1, D <= 448 shift 0; pad <= 1.92e9 < 2^31 for every shift <= 6)
inline bool i8k_key_ok(const I8KeyRule &r) {
    return r.lo + r.offset >= 1 && r.hi + r.offset < r.pad && r.pad < ((int64_t)1 << 31) &&
           ((uint64_t)(r.pad >> r.shift) << 6 | 63u) < kI8kInf;
}

// ---- the build rule: which handles get the int8 K-loop copy at an add ------------------------------------------------------------
// (flat: a plain flat handle -- IVF, PQ, LSH, k-NN-graph and multi-device handles are out of scope)
inline bool i8k_build(int opt_i8_kloop, bool flat, bool tile16, bool byte_valued, bool panels_streamed, int dim) {
    return opt_i8_kloop != 0 && flat && tile16 && byte_valued && !panels_streamed && dim <= kI8kMaxDim;
}

// ---- the launch rule: which searches the kernel serves -------------------------------------------------------------------------
// a handle with the copy | option "panel_dtype" = 0 | the standard 256-row-bin geometry (no direct bins) | resident panels |
// an unfiltered vdb_search / vdb_search_device.  Everything else runs as without the option.
inline bool i8k_serves(bool has_copy, int panel_dtype, int direct_rows, bool panels_streamed, bool filtered) {
    return has_copy && panel_dtype == 0 && direct_rows == 0 && !panels_streamed && !filtered;
}

// K-steps (64 dims) between workgroup barriers; the LDS ring holds 2 x that many 8-KiB stages
constexpr int kI8kBarrierSteps = 2;

}  // namespace vdb

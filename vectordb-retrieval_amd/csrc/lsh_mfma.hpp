// lsh_mfma.hpp -- the sign-LSH Hamming scan on v_mfma_i32_16x16x64_i8 (gfx950 only; option "lsh_mfma").  Host side: lsh.inc; tile
// sizes, LDS bytes and grid: lsh_mfma_plan.hpp.
//
// Same contract as lsh_scan_kernel<MODE, WP> (lsh.hpp) over the same LshSelArgs, and the same integers: with the row bits as 0 / 1
// bytes a and the query bits as +-1 bytes b (+1 for a set bit),  sum a b = n11 - n10  and  popc(q) = n11 + n01,  so
//     hamming = n10 + n01 = popc(q) - sum a b,
// exact in the int32 accumulator.  The test d <= t is  acc >= popc(q) - t,  one constant per query.  Zero bytes of a (padding
// words, the upper half step of a 32-bit code, rows >= n) add nothing whatever b holds.
//
// Operands.  Byte k of a K-step is code bit 64 s + k.  A 16x16x64 fragment gives lane (i = lane & 15, g = lane >> 4) the 16 bytes
// k = 16 g .. 16 g + 15 of row (A) or query (B) i: the 16-bit piece g of the step's two code words.
//   A: a wave loads the words of its rt tiles of 16 rows once per pass and expands every piece into 4 VGPRs of 0 / 1 bytes
//      (nibble x 0x00204081 & 0x01010101); the fragments stay in registers for the whole query tile.
//   B: lsh_mfma_qop_kernel expands the query codes of a chunk, once, into the workspace in fragment order
//      [column block of 16 queries][K-step][lane][16 bytes], and writes popc(q); a scan workgroup copies the blocks of its query
//      tile into LDS as they are, so a B fragment is one conflict-free 16-byte LDS read per lane, reused over the rt row tiles.
// Accumulator: lane (i, g) holds rows 4 g .. 4 g + 3 of the tile for query i of the column block -- a lane owns one column, so the
// epilogue of a column block is a maximum over the lane's 4 rt sums and one compare against the query's constant; only a hit takes
// the branch (for the whole wave), which appends exactly as lsh_scan_kernel does.
#pragma once
#include "common.hpp"
#include "lsh_mfma_plan.hpp"
#include "lsh_select.hpp"
#include "scan_i8.hpp"

namespace vdb {

constexpr int kLshMfmaNever = 0x7fffffff;      // compare constant of a query that takes no part (no sum reaches it)

// 4 code bits -> 4 bytes of 0 / 1 (bit j in byte j): the shifts by 0, 7, 14 and 21 do not overlap
__device__ __forceinline__ uint32_t lsh_mfma_bytes01(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

// the 16-bit piece `g` of K-step `s` of a code of `wp` words (zero past the code)
__device__ __forceinline__ uint32_t lsh_mfma_piece(const uint32_t *__restrict__ code, int wp, int s, int g) {
    const int w = 2 * s + (g >> 1);
    return w < wp ? (code[w] >> (16 * (g & 1))) & 0xffffu : 0u;
}

// The B operand and popc of the a.nq query codes of a chunk: one thread per (column block, K-step, lane).  Queries past a.nq in the
// last column block get zero bytes (their compare constant keeps them out anyway).
__global__ __launch_bounds__(256) void lsh_mfma_qop_kernel(LshSelArgs a, int ksteps, int4v *__restrict__ qop, int *__restrict__ qpopc) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(item & 63), s = (int)((item >> 6) % ksteps);
    const int64_t q = (item >> 6) / ksteps * 16 + (lane & 15);
    if (item >= (a.nq + 15) / 16 * ksteps * 64) return;
    int4v v = {0, 0, 0, 0};
    if (q < a.nq) {
        const uint32_t *code = a.qcodes + (size_t)q * a.kw;
        const uint32_t piece = lsh_mfma_piece(code, a.kw, s, lane >> 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t b01 = lsh_mfma_bytes01((piece >> (4 * e)) & 15u);
            v[e] = (int)(b01 | ((b01 ^ 0x01010101u) * 0xffu));        // 1 -> +1, 0 -> -1
        }
        if (s == 0 && lane < 16) {
            int pc = 0;
            for (int w = 0; w < a.kw; ++w) pc += __popc(code[w]);
            qpopc[q] = pc;
        }
    }
    qop[item] = v;
}

// MODE 0: count the pairs with d <= thi[q] into hist AND append them to the query's list (what fits).  MODE 1: append the pairs
// with d <= tq[q]; a workgroup none of whose queries asks for it returns before it loads a row, and a column block none of whose
// queries does is skipped.  Grid: (row tiles of lsh_mfma_row_tile(WP) rows, query tiles of a.qtile); dynamic LDS lsh_mfma_lds_bytes(WP).
template <int MODE, int WP>
__global__ __launch_bounds__(64 * kLshMfmaWaves) void lsh_mfma_scan_kernel(LshSelArgs a) {
    constexpr int KS = lsh_mfma_ksteps(WP), RT = lsh_mfma_row_tiles(WP), QT = lsh_mfma_qtile(WP), THREADS = 64 * kLshMfmaWaves;
    static_assert(QT % 16 == 0 && QT <= THREADS, "one thread per query of the tile, whole column blocks");
    extern __shared__ __attribute__((aligned(16))) unsigned char lsh_mfma_lds[];
    int4v *bop = reinterpret_cast<int4v *>(lsh_mfma_lds);                            // [column block][KS][64]
    int *kq = reinterpret_cast<int *>(lsh_mfma_lds + (size_t)QT * lsh_mfma_qbytes(WP));   // [QT]: popc(q) - t, or kLshMfmaNever
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.y * QT;
    const int nqt = (int)(a.nq - q0 < QT ? a.nq - q0 : QT), ncb = (nqt + 15) >> 4;
    int mine = -1;
    if (tid < nqt) mine = (MODE == 0 ? a.thi : a.tq)[q0 + tid];
    if (MODE == 1 && !__syncthreads_or(mine >= 0)) return;
    if (tid < QT) kq[tid] = mine >= 0 ? a.qpopc[q0 + tid] - mine : kLshMfmaNever;
    {
        const int4v *src = reinterpret_cast<const int4v *>(a.qop) + (size_t)(q0 >> 4) * KS * 64;
        for (int i = tid; i < ncb * KS * 64; i += THREADS) bop[i] = src[i];
    }
    __syncthreads();
    const int i16 = lane & 15, g = lane >> 4;
    const int64_t wg_row0 = (int64_t)blockIdx.x * lsh_mfma_row_tile(WP);
#pragma unroll 1
    for (int p = 0; p < kLshMfmaPasses; ++p) {
        const int64_t base = wg_row0 + (int64_t)p * lsh_mfma_rows_per_pass(WP) + wave * (RT * 16);
        if (base >= a.n) break;                                   // (wave-uniform; no barrier below)
        int4v fa[RT][KS];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int64_t row = base + t * 16 + i16;
            const bool valid = row < a.n;
            const uint32_t *code = a.codes + (size_t)(valid ? row : 0) * WP;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const uint32_t piece = valid ? lsh_mfma_piece(code, WP, s, g) : 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) fa[t][s][e] = (int)lsh_mfma_bytes01((piece >> (4 * e)) & 15u);
            }
        }
#pragma unroll 1
        for (int cb = 0; cb < ncb; ++cb) {
            const int k = kq[cb * 16 + i16];
            if (__ballot(k != kLshMfmaNever) == 0) continue;      // none of the block's queries takes part
            int4v acc[RT];
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t] = int4v{0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int4v b = bop[(cb * KS + s) * 64 + lane];
#pragma unroll
                for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[t][s], b, acc[t], 0, 0, 0);
            }
            int m[RT], mx = -kLshMfmaNever;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                m[t] = max(max(acc[t][0], acc[t][1]), max(acc[t][2], acc[t][3]));
                mx = max(mx, m[t]);
            }
            if (mx >= k) {                                        // the rare hit: d = popc(q) - acc <= t
                const int64_t gq = q0 + cb * 16 + i16;
                const int pq = a.qpopc[gq];
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    if (m[t] < k) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t row = base + t * 16 + 4 * g + r;
                        if (acc[t][r] < k || row >= a.n) continue;
                        const int d = pq - acc[t][r];
                        if (MODE == 0) atomicAdd(&a.hist[(size_t)gq * a.hb + d], 1);
                        const int idx = atomicAdd(&a.cnt[gq], 1);
                        if (idx < a.cap) a.list[(size_t)gq * a.cap + idx] = ((unsigned long long)d << 32) | (unsigned long long)row;
                    }
                }
            }
        }
    }
}

}  // namespace vdb

// lsh_mfma_plan.hpp -- the int8 MFMA form of the sign-LSH Hamming scan (lsh_mfma.hpp; option "lsh_mfma"): tile sizes, LDS bytes and
// grid per stored code width.  Plain host C++, so tests/host/lsh_mfma_plan_main.cpp prints what the rules give.
//
// One K-step of v_mfma_i32_16x16x64_i8 is 64 code bits = two code words; a 32-bit code (wp = 1) runs half a step on zeros.  A wave
// keeps `rt` tiles of 16 rows as expanded A fragments in registers, 4 VGPRs per tile and K-step, and reuses every B fragment (one
// 16-byte LDS read per lane) over them; rt * ksteps <= 32 bounds the fragments at 128 VGPRs:
//
//   bits   wp  ksteps  rt  A VGPRs  rows per pass  qtile  LDS bytes
//     32    1       1   8       32           1024    256     17 408
//     64    2       1   8       32           1024    256     17 408
//    128    4       2   8       64           1024    256     33 792
//    256    8       4   4       64            512    256     66 560
//    512   16       8   2       64            256    128     66 048
//   1024   32      16   2      128            256     64     65 792
//
// A workgroup of 8 waves stages the +-1 operand of its query tile (qtile x 64 ksteps bytes, at most 64 KiB) and one compare constant
// per query (4 bytes) in LDS once, then walks kLshMfmaPasses row passes against it.  The limit is 65 KiB of dynamic LDS per workgroup
// (MODE 1 adds the 256 static bytes of its workgroup vote): two workgroups would fit the 160 KiB of a CU at every width; the registers
// allow one at most widths.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vdb {

constexpr int kLshMfmaWaves = 8;                     // waves per workgroup (512 threads)
constexpr int kLshMfmaPasses = 4;                    // row passes a workgroup walks against one staged query tile
constexpr int kLshMfmaOperandLds = 64 * 1024;        // bytes of query operand a workgroup stages
constexpr size_t kLshMfmaLdsLimit = 65 * 1024;       // ... + the compare constants

constexpr int lsh_mfma_ksteps(int wp) { return (wp + 1) / 2; }
constexpr int lsh_mfma_row_tiles(int wp) { return lsh_mfma_ksteps(wp) <= 2 ? 8 : lsh_mfma_ksteps(wp) <= 4 ? 4 : 2; }
constexpr int lsh_mfma_rows_per_pass(int wp) { return kLshMfmaWaves * lsh_mfma_row_tiles(wp) * 16; }
constexpr int lsh_mfma_row_tile(int wp) { return kLshMfmaPasses * lsh_mfma_rows_per_pass(wp); }   // rows per workgroup
constexpr int lsh_mfma_qbytes(int wp) { return 64 * lsh_mfma_ksteps(wp); }                         // operand bytes per query
constexpr int lsh_mfma_qtile(int wp) {
    return kLshMfmaOperandLds / lsh_mfma_qbytes(wp) < 256 ? kLshMfmaOperandLds / lsh_mfma_qbytes(wp) : 256;
}
constexpr size_t lsh_mfma_lds_bytes(int wp) { return (size_t)lsh_mfma_qtile(wp) * (lsh_mfma_qbytes(wp) + sizeof(int)); }
// bytes of the operand of nq queries in the workspace: whole 16-query column blocks
constexpr size_t lsh_mfma_operand_bytes(int wp, int64_t nq) { return (size_t)((nq + 15) / 16 * 16) * lsh_mfma_qbytes(wp); }

struct LshMfmaGrid { unsigned x, y; };
constexpr LshMfmaGrid lsh_mfma_grid(int wp, int64_t n, int64_t nq) {
    return {(unsigned)((n + lsh_mfma_row_tile(wp) - 1) / lsh_mfma_row_tile(wp)), (unsigned)((nq + lsh_mfma_qtile(wp) - 1) / lsh_mfma_qtile(wp))};
}

}  // namespace vdb

// ivf_i8_plan.hpp -- the rules of an IVF-I8 index (vdb_ivf_set_codec 3; ivf_i8.hpp, ivf_i8.inc): which byte window
// a corpus is stored under, the device bytes the kind keeps, and the size of the per-batch fp16 slab.  No HIP:
// tests/host/ivf_i8_plan_main.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

namespace vdb {

// The window.  A row is stored as byte = x - cx and decoded as x = byte + cx, exactly.  `vmin` / `vmax`: the smallest and largest
// value of the WHOLE corpus (the rows the handle holds and the rows of the add), `all_integer`: every value is a finite integer
// (the flags of corpus_stats_kernel, the test the flat int8 copies are admitted by).  128: every value in 0..255 (checked first:
// a corpus inside 0..127 fits both windows and takes this one, as the flat index does); 0: every value in -128..127; -1: the
// corpus is not byte-valued and the add is refused.
inline int ivf_i8_window(int vmin, int vmax, bool all_integer) {
    if (!all_integer || vmin > vmax) return -1;
    if (vmin >= 0 && vmax <= 255) return 128;
    if (vmin >= -128 && vmax <= 127) return 0;
    return -1;
}

// bytes of an int8 row (rows8) and 32-dim k-steps of the int8 panels: D <= 64 -> 64 bytes, 2 k-steps; D <= 128 -> 128 bytes, 4
inline int ivf_i8_ksteps(int dim) { return dim <= 64 ? 2 : 4; }
inline int ivf_i8_pitch(int dim) { return ivf_i8_ksteps(dim) * 32; }

// Device bytes an IVF-I8 index of N rows keeps for its rows, `panel_rows` = pspans * 256 slots of the list-padded panel space:
//   per row        rows8 (pitch) + rowstat8 {sum x^2, sum x} (8) + ivf_ids (8)
//   per panel row  panels8 (pitch) + bias8, both query windows (8) + the fp16 scan's bias (4)
//   per span       span_row0 + span_valid (8)
// every one of them sized exactly.  Not counted: what depends on nlist alone (the centroids and their coarse index, the CSR
// offsets, list_pspan0) and the per-search workspace.  128 dims: 144 B per row + 140 B per panel row, ~0.57 x the float32 rows
// when the lists are long; an IVF-Flat index of the same rows keeps 660 B + 396 B (+ 1/8 growth slack).
inline int64_t ivf_i8_bytes(int64_t N, int64_t panel_rows, int dim) {
    const int64_t pitch = ivf_i8_pitch(dim);
    return N * (pitch + 8 + 8) + panel_rows * (pitch + 8 + 4) + panel_rows / 256 * 8;
}

// bytes of the fp16 panels of the whole panel space, made per batch by ivf_panels_from_i8_kernel for the batches the int8 scan
// cannot serve: 2 bytes per dimension (padded to 64 or 128) per panel row.  Workspace; never allocated under "ivf_i8_scratch" = 0.
inline int64_t ivf_i8_slab_bytes(int64_t panel_rows, int dim) { return panel_rows * ivf_i8_pitch(dim) * 2; }

}  // namespace vdb

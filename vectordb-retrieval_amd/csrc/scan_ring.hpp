// scan_ring.hpp -- the stage ring of the int8 x16 batch loop (scan_i8x16_batch_loop, scan_i8x16.hpp) as plain rules.
//
// A wrong ring is a hang or a race, not a wrong number, so what the kernel does per stage is decided here, in constexpr / inline
// C++ that the kernel and a host program (tests/host/scan_ring_main.cpp) both include.  No HIP, no device code.
//
// The ring has R buffers; stage s lives in buffer s % R.  One workgroup barrier per stage, each behind a FULL wait of the wave on
// its own memory operations, plus one barrier that ends the prologue.  Barriers are numbered by the stage they end; the prologue's
// is barrier -1.
//   * prologue: stages 0 .. min(nstages, R - 1) - 1 are issued, then barrier -1.
//   * during stage s: stage s + R - 1 is issued (when there is one) into the buffer that stage s - 1 read -- every wave finished
//     those reads before barrier s - 1, which this wave has passed.  The wave's pieces are a whole stage old at barrier s, so
//     barrier s certifies stage s + R - 1: it may be read by any wave at any time after it.
//   * the last step of stage s reads tile 0 of stage s + 1 (when there is one) ahead of barrier s.  Stage s + 1 was certified by
//     barrier s + 1 - (R - 1) <= s - 1 for R >= 3: a ring of 2 cannot read ahead.
//   * a wave whose query columns are all padding computes nothing, but issues the same pieces and takes the same barriers.
#pragma once

namespace vdb {

// ring depth of the batch forms of scan_i8x16_body.  Their plan keys say RING = 2 ("no deep ring", scan_plan.hpp); the number of
// LDS buffers behind that key is this constant.
constexpr int kX16BatchRing = 3;

// the batch forms: 8 waves, plan ring 2, rolled stages (ST * CB > 16: 8-tile stages with CB = 8 or 4, 4-tile stages with CB = 8)
constexpr bool x16_batch_form(int st_tiles, int cb, int nwaves, int plan_ring) {
    return nwaves == 8 && plan_ring == 2 && st_tiles * cb > 16;
}
// LDS buffers of a form
constexpr int x16_ring_buffers(int st_tiles, int cb, int nwaves, int plan_ring) {
    return x16_batch_form(st_tiles, cb, nwaves, plan_ring) ? kX16BatchRing : plan_ring;
}
// bytes of one stage: ST tiles of 2 KS2 fragments of 1 KiB, and 32 biases per tile
constexpr int x16_stage_bytes(int ks2, int st_tiles) { return st_tiles * 2 * ks2 * 64 * 16 + st_tiles * 32 * 4; }
constexpr int x16_lds_bytes(int ks2, int st_tiles, int cb, int nwaves, int plan_ring) {
    return x16_ring_buffers(st_tiles, cb, nwaves, plan_ring) * x16_stage_bytes(ks2, st_tiles);
}

constexpr int ring_buffer(int s, int R) { return s % R; }
// stages issued before barrier -1
constexpr int ring_prologue_stages(int nstages, int R) { return nstages < R - 1 ? nstages : R - 1; }
// the stage issued during stage s, and whether there is one
constexpr int ring_issue_stage(int s, int R) { return s + R - 1; }
constexpr bool ring_issues(int s, int nstages, int R) { return s + R - 1 < nstages; }
// the barrier that certifies stage s (-1: the prologue's)
constexpr int ring_certifier(int s, int R) { return s < R - 1 ? -1 : s - (R - 1); }
// whether the last step of stage s reads tile 0 of stage s + 1; if not it reads tile 0 of its own stage again (no branch in the loop)
constexpr bool ring_reads_ahead(int s, int nstages) { return s + 1 < nstages; }
// barriers a wave takes, computing or padded: the prologue's and one per stage
constexpr int ring_barriers(int nstages) { return nstages + 1; }

}  // namespace vdb

// The stage ring of the int8 x16 batch loop (csrc/scan_ring.hpp) as a host program: tests/test_scan_ring_host.py checks its output.
// For nstages = 1 .. 12 it walks what a computing wave and a fully padded wave do, in the order scan_i8x16_body and
// scan_i8x16_batch_loop do it and decided by the same functions, and prints the walk as events:
//   ["I", stage, buffer]   the wave issues its share of the LDS-DMA of a stage
//   ["R", stage, buffer]   the wave reads tiles of a stage from LDS
//   ["B", barrier]         full wait on the wave's own memory operations, then the workgroup barrier (-1: the prologue's)
// Then one line with the LDS bytes of every form.  No HIP, no GPU.
#include <stdio.h>

#include "../../vectordb-retrieval_amd/csrc/scan_ring.hpp"

using namespace vdb;

static void walk(int nstages, bool computing) {
    constexpr int R = kX16BatchRing;
    const char *sep = "";
    auto ev3 = [&](const char *k, int a, int b) { printf("%s[\"%s\", %d, %d]", sep, k, a, b), sep = ", "; };
    auto bar = [&](int b) { printf("%s[\"B\", %d]", sep, b), sep = ", "; };
    printf("[");
    for (int s = 0; s < R - 1; ++s)
        if (s < ring_prologue_stages(nstages, R)) ev3("I", s, ring_buffer(s, R));
    bar(-1);
    if (computing) ev3("R", 0, ring_buffer(0, R));                       // tile 0 of stage 0, ahead of the loop
    for (int s = 0; s < nstages; ++s) {
        if (computing) ev3("R", s, ring_buffer(s, R));                   // step 0 reads tile 1, ...
        if (ring_issues(s, nstages, R)) ev3("I", ring_issue_stage(s, R), ring_buffer(ring_issue_stage(s, R), R));   // behind step 0
        if (computing) {
            ev3("R", s, ring_buffer(s, R));                              // ... steps 1 .. ST - 2 the tiles up to ST - 1,
            const int nx = ring_reads_ahead(s, nstages) ? s + 1 : s;     // the last step tile 0 of the next stage
            ev3("R", nx, ring_buffer(nx, R));
        }
        bar(s);
    }
    printf("]");
}

int main() {
    for (int n = 1; n <= 12; ++n) {
        printf("{\"nstages\": %d, \"ring\": %d, \"barriers\": %d, \"certifier\": [", n, kX16BatchRing, ring_barriers(n));
        for (int s = 0; s < n; ++s) printf("%s%d", s ? ", " : "", ring_certifier(s, kX16BatchRing));
        printf("], \"computing\": ");
        walk(n, true);
        printf(", \"padded\": ");
        walk(n, false);
        printf("}\n");
    }
    // every form the kernel tables hold: KS2 1 / 2, ST 4 / 8, CB 4 / 8, waves 1 / 2 / 4 / 8, plan rings 2 / 4 / 8
    printf("{\"forms\": [");
    const char *sep = "";
    for (int ks2 = 1; ks2 <= 2; ++ks2)
        for (int st = 4; st <= 8; st += 4)
            for (int cb = 4; cb <= 8; cb += 4)
                for (int nw = 1; nw <= 8; nw *= 2)
                    for (int ring = 2; ring <= 8; ring *= 2) {
                        printf("%s{\"ks2\": %d, \"st\": %d, \"cb\": %d, \"nwaves\": %d, \"ring\": %d, \"batch\": %d, \"buffers\": %d, "
                               "\"stage_bytes\": %d, \"lds_bytes\": %d}",
                               sep, ks2, st, cb, nw, ring, (int)x16_batch_form(st, cb, nw, ring), x16_ring_buffers(st, cb, nw, ring),
                               x16_stage_bytes(ks2, st), x16_lds_bytes(ks2, st, cb, nw, ring));
                        sep = ", ";
                    }
    printf("]}\n");
    return 0;
}

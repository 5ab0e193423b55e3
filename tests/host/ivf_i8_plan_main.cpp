// The rules of an IVF-I8 index (csrc/ivf_i8_plan.hpp) as a host program: tests/test_ivf_i8_host.py compares its output with a
// NumPy restatement.  Input: one case per line, "vmin vmax all_integer N panel_rows dim".  Output: one JSON object per case -- the
// byte window, the row pitch and k-steps, the resident bytes of the kind and the bytes of the per-batch fp16 slab.
#include <stdio.h>

#include <cinttypes>

#include "../../vectordb-retrieval_amd/csrc/ivf_i8_plan.hpp"

using namespace vdb;

int main() {
    int vmin, vmax, all_integer, dim;
    long long N, panel_rows;
    while (scanf("%d %d %d %lld %lld %d", &vmin, &vmax, &all_integer, &N, &panel_rows, &dim) == 6)
        printf("{\"cx\": %d, \"pitch\": %d, \"ksteps\": %d, \"bytes\": %" PRId64 ", \"slab\": %" PRId64 "}\n", ivf_i8_window(vmin, vmax, all_integer != 0),
               ivf_i8_pitch(dim), ivf_i8_ksteps(dim), ivf_i8_bytes(N, panel_rows, dim), ivf_i8_slab_bytes(panel_rows, dim));
    return 0;
}

// lsh_mfma_plan_main.cpp -- prints what the rules of csrc/lsh_mfma_plan.hpp decide, without HIP or a GPU.  One line per input line:
//   plan <wp> <n> <nq> -> JSON: K-steps, row tiles per wave, rows per pass and per workgroup, query tile, LDS bytes and limit,
//                         operand bytes of nq queries, grid
#include <stdio.h>

#include "../../vectordb-retrieval_amd/csrc/lsh_mfma_plan.hpp"

using namespace vdb;

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int wp;
        long long n, nq;
        if (sscanf(line, "plan %d %lld %lld", &wp, &n, &nq) != 3) continue;
        const LshMfmaGrid g = lsh_mfma_grid(wp, n, nq);
        printf("{\"ksteps\":%d,\"rt\":%d,\"waves\":%d,\"rows_pass\":%d,\"row_tile\":%d,\"qtile\":%d,\"lds\":%llu,\"lds_limit\":%llu,\"operand\":%llu,"
               "\"grid\":[%u,%u]}\n",
               lsh_mfma_ksteps(wp), lsh_mfma_row_tiles(wp), kLshMfmaWaves, lsh_mfma_rows_per_pass(wp), lsh_mfma_row_tile(wp), lsh_mfma_qtile(wp),
               (unsigned long long)lsh_mfma_lds_bytes(wp), (unsigned long long)kLshMfmaLdsLimit, (unsigned long long)lsh_mfma_operand_bytes(wp, nq),
               g.x, g.y);
    }
    return 0;
}

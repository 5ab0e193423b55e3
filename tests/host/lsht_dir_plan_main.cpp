// lsht_dir_plan_main.cpp -- prints what the rules of csrc/lsht_dir_plan.hpp decide, without HIP or a GPU.  One line per input line:
//   plan <T> <kw> <n> <visits> <nq> -> JSON: slots, directory and temporary bytes, whether n fits, entries per query, splits, the rule,
//                                 and what options 0 / 1 / 2 route to
//   hash <W> <word> ...        -> JSON: the slot hash of one table key of W words
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../vectordb-retrieval_amd/csrc/lsht_dir_plan.hpp"

using namespace vdb;

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        int T, kw;
        long long n, nq;
        unsigned long long visits;
        if (sscanf(line, "plan %d %d %lld %llu %lld", &T, &kw, &n, &visits, &nq) == 5) {
            printf("{\"slots\":%lld,\"bytes\":%llu,\"tmp_bytes\":%llu,\"fits\":%d,\"entries\":%.6f,\"splits\":%d,\"rule\":%d,\"use\":[%d,%d,%d],"
                   "\"gather_cost\":%g,\"gather_cost_derived\":%g,\"word_cost\":%g}\n",
                   (long long)lsht_dir_slots(n), (unsigned long long)lsht_dir_bytes(T, n), (unsigned long long)lsht_dir_tmp_bytes(T, n),
                   (int)lsht_dir_fits(n), lsht_dir_entries_per_query(visits, n), lsht_dir_splits(visits, n), (int)lsht_dir_rule(visits, n, kw, nq),
                   (int)lsht_dir_use(0, visits, n, kw, nq), (int)lsht_dir_use(1, visits, n, kw, nq), (int)lsht_dir_use(2, visits, n, kw, nq),
                   lsht_dir_gather_cost(nq), kLshtDirGatherCostDerived, kLshtDirWordCost);
        } else if (strncmp(line, "hash ", 5) == 0) {
            char *p = line + 5;
            const int W = (int)strtol(p, &p, 10);
            uint32_t words[64] = {0};
            for (int w = 0; w < W && w < 64; ++w) words[w] = (uint32_t)strtoul(p, &p, 10);
            printf("{\"hash\":%u}\n", lsht_dir_hash(words, W < 64 ? W : 64));
        }
    }
    return 0;
}

// ivf_pq_kloop_plan_main.cpp -- prints what the rules of csrc/ivf_pq_kloop_plan.hpp decide, without HIP or a GPU.  One line per input line:
//   builds <option> <codec> <D> <M>                         -> 0 / 1   (ksteps = 4 ceil(D / 64), dsub = D / M)
//   serves <option> <codec> <built> <kloop_geom> <filtered> -> 0 / 1
//   space <M> <dsub>                                        -> JSON: P, Kp, nk and the dimension of every operand position
//   plan <M> <tps> <kgroup>                                 -> JSON: the launch of a two-list handle, its LDS bytes, whether it is instantiated
#include <stdio.h>

#include "../../vectordb-retrieval_amd/csrc/ivf_pq_kloop_plan.hpp"

using namespace vdb;

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int a[5];
        if (sscanf(line, "builds %d %d %d %d", &a[0], &a[1], &a[2], &a[3]) == 4) {
            printf("%d\n", ivf_pqk_builds(a[0], a[1], 4 * ((a[2] + 63) / 64), a[2], a[3], a[2] / a[3]) ? 1 : 0);
        } else if (sscanf(line, "serves %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5) {
            printf("%d\n", ivf_pqk_serves(a[0], a[1], a[2] != 0, a[3] != 0, a[4] != 0) ? 1 : 0);
        } else if (sscanf(line, "space %d %d", &a[0], &a[1]) == 2) {
            const int nk = ivf_pqk_nk(a[0], a[1]);
            printf("{\"P\":%d,\"Kp\":%d,\"nk\":%d,\"dim\":[", ivf_pqk_p(a[1]), ivf_pqk_kp(a[0], a[1]), nk);
            for (int p = 0; p < 64 * nk; ++p) printf("%s%d", p ? "," : "", ivf_pqk_operand_dim(p, a[0], a[1]));
            printf("]}\n");
        } else if (sscanf(line, "plan %d %d %d", &a[0], &a[1], &a[2]) == 3) {
            Options opt;
            IvfIndexShape s;
            s.N = 23200; s.nlist = 2; s.tps = a[1]; s.span_rows = 16 * a[1];
            s.pspans = 2 * ((11600 + s.span_rows - 1) / s.span_rows); s.max_pspans = (int)s.pspans / 2;
            s.ksteps = 12; s.tile16 = true; s.mfma_ok = true;
            IvfGeom g;
            g.ok = g.kloop = true; g.group = kIvfKloopGroup; g.max_items = 4;
            const IvfLaunch p = plan_ivf_pqk(s, opt, g, a[2], a[0]);
            bool listed = false;
            for (const ScanKey &r : kKeysIvfPqk) listed = listed || r == p.key;
            printf("{\"family\":\"%s\",\"targs\":[%d,%d,%d,%d],\"block\":%u,\"lds\":%llu,\"budget\":%llu,\"listed\":%s}\n",
                   kScanFamilyNames[(int)p.family], p.key.t[0], p.key.t[1], p.key.t[2], p.key.t[3], p.block,
                   (unsigned long long)ivf_pqk_lds_bytes(p.key.t[1], p.key.t[3]), (unsigned long long)kPqkLdsBudget, listed ? "true" : "false");
        }
    }
    return 0;
}

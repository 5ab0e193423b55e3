// pq_kloop_plan_main.cpp -- prints what the rules of csrc/pq_kloop_plan.hpp decide, without HIP or a GPU.  One line per input line:
//   serves <option> <pq> <D> <M> <scan_path> <direct_rows> <adc> <filtered> -> 0 / 1   (ksteps = 4 ceil(D / 64), dsub = D / M)
//   lds <M>                                     -> JSON: code pitch, ring depth, LDS bytes, workgroups per CU the LDS allows
//   plan <M> <nq> <small_batch> <qgroup>        -> JSON: the launch over 11 chunks next to the flat K-loop scan's, whether it is instantiated
//   space <M> <dsub>                            -> JSON: P, Kp, nk and the dimension of every operand position
#include <stdio.h>

#include "../../vectordb-retrieval_amd/csrc/pq_kloop_plan.hpp"

using namespace vdb;

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int a[8];
        if (sscanf(line, "serves %d %d %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) == 8) {
            printf("%d\n", pq_kloop_serves(a[0], a[1] != 0, 4 * ((a[2] + 63) / 64), a[3], a[2] / a[3], a[4] != 0, a[5], a[6] != 0, a[7] != 0) ? 1 : 0);
        } else if (sscanf(line, "lds %d", &a[0]) == 1) {
            const int cp = pq_kloop_code_pitch(a[0]), bs = pq_kloop_ring_bs(a[0]);
            printf("{\"cp\":%d,\"bs\":%d,\"lds\":%llu,\"wgs\":%d}\n", cp, bs, (unsigned long long)pq_kloop_lds_bytes(bs, cp), pq_kloop_wgs_per_cu_lds(a[0]));
        } else if (sscanf(line, "plan %d %d %d %d", &a[0], &a[1], &a[2], &a[3]) == 4) {
            Options opt;
            opt.small_batch = a[2];
            opt.kloop_qgroup = a[3];
            ScanIndexShape s;
            s.ksteps = 12; s.tile16 = true; s.pq = true; s.Npad = 21 * 1024;
            const int64_t Qpad = (a[1] + 511) / 512 * 512;
            const ScanLaunch p = plan_pq_kloop(s, opt, 11, Qpad, a[1], a[0]), f = plan_f16(s, opt, 11, Qpad, a[1], 0, 8);
            bool listed = false;
            for (const ScanKey &r : kKeysPqKloop) listed = listed || r == p.key;
            printf("{\"family\":\"%s\",\"targs\":[%d,%d,%d],\"grid\":%u,\"block\":%u,\"nqtiles\":%d,\"qgroup\":%d,\"f16\":[%u,%u,%d,%d],\"listed\":%s}\n",
                   kScanFamilyNames[(int)p.family], p.key.t[0], p.key.t[1], p.key.t[2], p.grid, p.block, p.nqtiles, p.qgroup, f.grid, f.block,
                   f.nqtiles, f.qgroup, listed ? "true" : "false");
        } else if (sscanf(line, "space %d %d", &a[0], &a[1]) == 2) {
            const int nk = ivf_pqk_nk(a[0], a[1]);
            printf("{\"P\":%d,\"Kp\":%d,\"nk\":%d,\"dim\":[", ivf_pqk_p(a[1]), ivf_pqk_kp(a[0], a[1]), nk);
            for (int p = 0; p < 64 * nk; ++p) printf("%s%d", p ? "," : "", ivf_pqk_operand_dim(p, a[0], a[1]));
            printf("]}\n");
        }
    }
    return 0;
}

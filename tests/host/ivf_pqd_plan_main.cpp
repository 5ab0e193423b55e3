// ivf_pqd_plan_main.cpp -- prints what the rules of csrc/ivf_pq_direct_plan.hpp decide, without HIP or a GPU.  One line per input line:
//   serve <option> <codec> <geom_ok> <kloop> <filtered>           -> 0 / 1
//   lds <D> <M> <ksteps>                                          -> JSON: code pitch, table / stage / codes / total bytes, workgroups per CU
//   plan <N> <nlist> <pspans> <max_pspans> <d> <k> <nq> <nprobe> <ivf_nw> <ivf_bt> <ivf_part>
//                                                                 -> JSON: the launch beside the fp16 items-mode launch
//   keys                                                          -> JSON: every instantiation of ivf_pq_scan_kernel
#include <stdio.h>
#include <string.h>
#include "../../vectordb-retrieval_amd/csrc/ivf_pq_direct_plan.hpp"

using namespace vdb;

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int a[5];
        long long N, pspans, nq;
        int nlist, max_pspans, d, k, nprobe, nw, bt, part;
        if (sscanf(line, "serve %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5) {
            printf("%d\n", ivf_pqd_serves(a[0], a[1], a[2] != 0, a[3] != 0, a[4] != 0) ? 1 : 0);
        } else if (sscanf(line, "lds %d %d %d", &a[0], &a[1], &a[2]) == 3) {
            printf("{\"pitch\":%d,\"table\":%llu,\"stage\":%llu,\"codes\":%llu,\"total\":%llu,\"wgs\":%d}\n", ivf_pqd_code_pitch(a[1]),
                   (unsigned long long)ivf_pqd_table_bytes(a[0]), (unsigned long long)ivf_pqd_stage_bytes(a[2]),
                   (unsigned long long)ivf_pqd_codes_bytes(a[1]), (unsigned long long)ivf_pqd_lds_bytes(a[0], a[1], a[2]),
                   ivf_pqd_wgs_per_cu(a[0], a[1], a[2]));
        } else if (sscanf(line, "plan %lld %d %lld %d %d %d %lld %d %d %d %d", &N, &nlist, &pspans, &max_pspans, &d, &k, &nq, &nprobe, &nw, &bt,
                          &part) == 11) {
            Options opt;
            opt.ivf_nw = nw; opt.ivf_bt = bt; opt.ivf_part = part;
            IvfIndexShape s;
            s.N = N; s.nlist = nlist; s.pspans = pspans; s.max_pspans = max_pspans;
            s.ksteps = d <= 64 ? 4 : 8; s.span_rows = kIvfSpanRows; s.mfma_ok = true;
            const IvfGeom g = ivf_geometry(s, opt, nq, k, nprobe);
            if (!g.ok) { printf("{\"ok\":false}\n"); continue; }
            const IvfLaunch p = plan_ivf_pqd(s, opt, g), f = plan_ivf_f16(s, opt, g);
            bool listed = false;
            for (const ScanKey &r : kKeysIvfPqd) listed = listed || r == p.key;
            printf("{\"ok\":true,\"family\":\"%s\",\"targs\":[%d,%d,%d],\"f16_targs\":[%d,%d,%d],\"grid\":[%u,%u,%u],\"f16_grid\":[%u,%u,%u],"
                   "\"part_spans\":[%d,%d],\"listed\":%s}\n",
                   kScanFamilyNames[(int)p.family], p.key.t[0], p.key.t[1], p.key.t[2], f.key.t[0], f.key.t[1], f.key.t[4], p.grid_x, p.grid_y,
                   p.block, f.grid_x, f.grid_y, f.block, p.part_spans, f.part_spans, listed ? "true" : "false");
        } else if (!strncmp(line, "keys", 4)) {
            printf("[");
            for (size_t i = 0; i < sizeof kKeysIvfPqd / sizeof kKeysIvfPqd[0]; ++i)
                printf("%s[%d,%d,%d]", i ? "," : "", kKeysIvfPqd[i].t[0], kKeysIvfPqd[i].t[1], kKeysIvfPqd[i].t[2]);
            printf("]\n");
        }
    }
    return 0;
}

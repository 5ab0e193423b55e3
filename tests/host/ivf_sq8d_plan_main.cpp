// ivf_sq8d_plan_main.cpp -- prints what the rules of csrc/ivf_sq8d_plan.hpp decide, without HIP or a GPU.  One line per input line:
//   serve <option> <codec> <geom_ok> <kloop> <D4> <filtered>      -> 0 / 1
//   chunks <D> <D4> <ksteps>                                      -> JSON: base of every chunk, and the dimension of every operand element
//   plan <N> <nlist> <pspans> <max_pspans> <d> <k> <nq> <nprobe> <ivf_nw> <ivf_bt> <ivf_part>
//                                                                 -> JSON: the launch beside the fp16 items-mode launch, LDS bytes
//   keys                                                          -> JSON: every instantiation of ivf_sq8_scan_kernel
#include <stdio.h>
#include <string.h>

#include "../../vectordb-retrieval_amd/csrc/ivf_sq8d_plan.hpp"

using namespace vdb;

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int a[6];
        long long N, pspans, nq;
        int nlist, max_pspans, d, k, nprobe, nw, bt, part;
        if (sscanf(line, "serve %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 6) {
            printf("%d\n", ivf_sq8d_serves(a[0], a[1], a[2] != 0, a[3] != 0, a[4], a[5] != 0) ? 1 : 0);
        } else if (sscanf(line, "chunks %d %d %d", &a[0], &a[1], &a[2]) == 3) {
            printf("{\"base\":[");
            for (int c = 0; c < a[2]; ++c) printf("%s%d", c ? "," : "", ivf_sq8d_chunk_base(c, a[1]));
            printf("],\"dim\":[");
            for (int e = 0; e < 16 * a[2]; ++e) printf("%s%d", e ? "," : "", ivf_sq8d_chunk_dim(e / 16, e % 16, a[0], a[1]));
            printf("]}\n");
        } else if (sscanf(line, "plan %lld %d %lld %d %d %d %lld %d %d %d %d", &N, &nlist, &pspans, &max_pspans, &d, &k, &nq, &nprobe, &nw, &bt,
                          &part) == 11) {
            Options opt;
            opt.ivf_nw = nw; opt.ivf_bt = bt; opt.ivf_part = part;
            IvfIndexShape s;
            s.N = N; s.nlist = nlist; s.pspans = pspans; s.max_pspans = max_pspans;
            s.ksteps = d <= 64 ? 4 : 8; s.span_rows = kIvfSpanRows; s.mfma_ok = true;
            const IvfGeom g = ivf_geometry(s, opt, nq, k, nprobe);
            if (!g.ok) { printf("{\"ok\":false}\n"); continue; }
            const IvfLaunch p = plan_ivf_sq8d(s, opt, g), f = plan_ivf_f16(s, opt, g);
            bool listed = false;
            for (const ScanKey &r : kKeysIvfSq8d) listed = listed || r == p.key;
            printf("{\"ok\":true,\"family\":\"%s\",\"targs\":[%d,%d,%d],\"f16_targs\":[%d,%d,%d],\"grid\":[%u,%u,%u],\"f16_grid\":[%u,%u,%u],"
                   "\"part_spans\":[%d,%d],\"lds\":%llu,\"listed\":%s}\n",
                   kScanFamilyNames[(int)p.family], p.key.t[0], p.key.t[1], p.key.t[2], f.key.t[0], f.key.t[1], f.key.t[4], p.grid_x, p.grid_y,
                   p.block, f.grid_x, f.grid_y, f.block, p.part_spans, f.part_spans, (unsigned long long)ivf_sq8d_lds_bytes(p.key.t[0]),
                   listed ? "true" : "false");
        } else if (!strncmp(line, "keys", 4)) {
            printf("[");
            for (size_t i = 0; i < sizeof kKeysIvfSq8d / sizeof kKeysIvfSq8d[0]; ++i)
                printf("%s[%d,%d,%d]", i ? "," : "", kKeysIvfSq8d[i].t[0], kKeysIvfSq8d[i].t[1], kKeysIvfSq8d[i].t[2]);
            printf("]\n");
        }
    }
    return 0;
}

// The rules of the int8 K-loop list scan (csrc/ivf_i8k_plan.hpp) as a host program: tests/test_ivf_i8k_plan_host.py checks its output.
// Input, one case per line:  "build option codec tile16 byte_valued dim" | "serve has_copy panel_dtype ivf_tile filtered list_major" |
// "plan N nlist pspans max_pspans d k nq nprobe ivf_tps ivf_group ivf_part" (a batch the launch rule admits: the int8 launch next to
// the fp16 one) | "keys" (every instantiation).
#include <stdio.h>
#include <string.h>

#include "../../vectordb-retrieval_amd/csrc/ivf_i8k_plan.hpp"

using namespace vdb;

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "build")) {
            int o, codec, t16, bv, dim;
            if (scanf("%d %d %d %d %d", &o, &codec, &t16, &bv, &dim) != 5) return 1;
            printf("%d\n", ivf_i8k_build(o, codec, t16 != 0, bv != 0, dim) ? 1 : 0);
        } else if (!strcmp(what, "serve")) {
            int has, pd, tile, filtered, lm;
            if (scanf("%d %d %d %d %d", &has, &pd, &tile, &filtered, &lm) != 5) return 1;
            printf("%d\n", ivf_i8k_serves(has != 0, pd, tile, filtered != 0, lm != 0) ? 1 : 0);
        } else if (!strcmp(what, "plan")) {
            long long N, pspans, nq;
            int nlist, max_pspans, d, k, nprobe;
            Options opt;
            if (scanf("%lld %d %lld %d %d %d %lld %d %d %d %d", &N, &nlist, &pspans, &max_pspans, &d, &k, &nq, &nprobe, &opt.ivf_tps,
                      &opt.ivf_group, &opt.ivf_part) != 11)
                return 1;
            IvfIndexShape s;
            s.mfma_ok = true; s.tile16 = true; s.nlist = nlist; s.N = N; s.pspans = pspans; s.max_pspans = max_pspans;
            s.ksteps = (d + 63) / 64 * 4;
            s.tps = ivf_tps_of(opt, N, nlist);
            s.span_rows = s.tps * 16;
            const IvfGeom g = ivf_geometry(s, opt, nq, k, nprobe);
            if (!g.ok || !g.kloop) {
                printf("{\"ok\":false}\n");
                continue;
            }
            const IvfCaps c = ivf_caps(s, opt, g, k);
            const IvfLaunch f = plan_ivf_kloop(s, opt, g, c.kgroup), p = plan_ivf_kloop_i8(s, opt, g, c.kgroup);
            bool listed = false;
            for (const ScanKey &r : kKeysIvfKloopI8) listed = listed || r == p.key;
            printf("{\"ok\":true,\"family\":\"%s\",\"targs\":[%d,%d,%d],\"listed\":%s,\"grid\":[%u,%u,%u,%d],\"f16_grid\":[%u,%u,%u,%d],\"kgroup\":%d}\n",
                   kScanFamilyNames[(int)p.family], p.key.t[0], p.key.t[1], p.key.t[2], listed ? "true" : "false", p.grid_x, p.grid_y, p.block,
                   p.part_spans, f.grid_x, f.grid_y, f.block, f.part_spans, c.kgroup);
        } else if (!strcmp(what, "keys")) {
            printf("[");
            for (size_t i = 0; i < sizeof(kKeysIvfKloopI8) / sizeof(kKeysIvfKloopI8[0]); ++i)
                printf("%s[%d,%d,%d]", i ? "," : "", kKeysIvfKloopI8[i].t[0], kKeysIvfKloopI8[i].t[1], kKeysIvfKloopI8[i].t[2]);
            printf("]\n");
        } else {
            return 1;
        }
    }
    return 0;
}

// The sizing and routing rules of a filtered search on an IVF-Flat index (csrc/ivf_filter_plan.hpp) as a host program:
// tests/test_ivf_filter_plan_host.py compares its output with a Python restatement.  Input: one case per line,
// "N nlist pspans max_pspans d k nq nprobe n_allowed force_path i8".  Output: one JSON object per case -- the unfiltered
// ivf_geometry, the filtered one, the rule on its own and the bytes of an install.
#include <stdio.h>

#include <cinttypes>

#include "../../vectordb-retrieval_amd/csrc/ivf_filter_plan.hpp"

using namespace vdb;

int main() {
    long long N, pspans, nq, n_allowed;
    int nlist, max_pspans, d, k, nprobe, force, i8;
    while (scanf("%lld %d %lld %d %d %d %lld %d %lld %d %d", &N, &nlist, &pspans, &max_pspans, &d, &k, &nq, &nprobe, &n_allowed, &force, &i8) == 11) {
        Options opt;
        opt.force_path = force;
        IvfIndexShape s;                    // (as ivf_build_panel_space derives it: tests/host/ivf_plan_main.cpp)
        s.N = N; s.nlist = nlist; s.pspans = pspans; s.max_pspans = max_pspans;
        s.ksteps = d <= 64 ? 4 : (d <= 128 ? 8 : (d + 63) / 64 * 4);
        s.i8_ks = d <= 64 ? 2 : 4;
        s.tile16 = s.ksteps > kMaxKSteps;
        s.tps = s.tile16 ? ivf_tps_of(opt, N, nlist) : 0;
        s.span_rows = s.tile16 ? s.tps * 16 : kIvfSpanRows;
        s.mfma_ok = N > 0 && pspans > 0;
        s.has_i8 = s.mfma_ok && i8 && !s.tile16;
        const IvfGeom g = ivf_geometry(s, opt, nq, k, nprobe);
        const IvfGeom f = ivf_filter_geometry(s, opt, nq, k, nprobe, n_allowed);
        const bool same = g.ok == f.ok && (!g.ok || (g.bt == f.bt && g.nw == f.nw && g.bins_per_span == f.bins_per_span && g.max_bins == f.max_bins &&
                                                    g.cnt_words == f.cnt_words && g.bin_bytes == f.bin_bytes));
        const int64_t panel_rows = pspans * s.span_rows;
        printf("{\"span_rows\": %d, \"ok\": %d, \"bins_per_span\": %d, \"filtered_ok\": %d, \"same\": %d, \"declines\": %d, \"words\": %" PRId64
               ", \"bytes\": %" PRId64 "}\n",
               s.span_rows, (int)g.ok, g.bins_per_span, (int)f.ok, (int)same, g.ok ? (int)ivf_filter_declines(s, g, k, nprobe, n_allowed) : -1,
               ivf_filter_words(N), ivf_filter_bytes(N, panel_rows, s.mfma_ok, s.has_i8));
    }
    return 0;
}

// ivf_plan_main.cpp -- prints what the rules of csrc/ivf_plan.hpp decide for a batch of an IVF search, without HIP or a GPU.
//
//   ivf_plan --keys       one JSON line per kernel family of the list scans: every instantiation the library holds
//   ivf_plan < cases      one JSON line per case
// A case is `N nlist pspans max_pspans d k nq nprobe` followed by `name=value` pairs: options of vdb_set_option that the rules read,
// and what an add derives from the corpus -- i8_ok (byte-valued rows), codec (0 Flat, 1 SQ8, 2 PQ: a coded index keeps no int8 copy),
// mfma_ok (0: no panel space, e.g. non-finite rows).  pspans / max_pspans are the panel spans of all lists / of the longest list, in
// spans of the `span_rows` this program prints.  The index shape follows build_derived (vdbhip.hip) and ivf_build_panel_space
// (ivf.inc), restated in shape_of below.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../vectordb-retrieval_amd/csrc/ivf_plan.hpp"

using namespace vdb;

namespace {

struct Named {
    const char *name;
    int Options::*m;
};
constexpr Named kNamed[] = {
    {"force_path", &Options::force_path}, {"ivf_min_batch", &Options::ivf_min_batch}, {"list_cap", &Options::list_cap},
    {"panel_dtype", &Options::panel_dtype}, {"i8_ring", &Options::i8_ring}, {"ivf_bt", &Options::ivf_bt},
    {"ivf_part", &Options::ivf_part}, {"ivf_tps", &Options::ivf_tps}, {"ivf_tile", &Options::ivf_tile},
    {"ivf_i8_group", &Options::ivf_i8_group}, {"ivf_group", &Options::ivf_group}, {"ivf_nw", &Options::ivf_nw},
};

struct Corpus {
    int i8_ok = 0, codec = 0, mfma_ok = 1;
};

IvfIndexShape shape_of(int64_t N, int nlist, int64_t pspans, int max_pspans, int d, const Options &opt, const Corpus &c) {
    IvfIndexShape s;
    s.N = N; s.nlist = nlist; s.pspans = pspans; s.max_pspans = max_pspans;
    s.ksteps = d <= 64 ? 4 : (d <= 128 ? 8 : (d + 63) / 64 * 4);
    s.i8_ks = d <= 64 ? 2 : 4;
    s.tile16 = s.ksteps > kMaxKSteps;
    s.tps = s.tile16 ? ivf_tps_of(opt, N, nlist) : 0;
    s.span_rows = s.tile16 ? s.tps * 16 : kIvfSpanRows;
    s.mfma_ok = c.mfma_ok && N > 0 && d <= 4096 && pspans > 0;
    s.has_i8 = s.mfma_ok && c.i8_ok && !s.tile16 && c.codec == 0;
    return s;
}

template <size_t N>
bool listed(const ScanKey (&keys)[N], const ScanKey &k) {
    for (const ScanKey &r : keys)
        if (r == k) return true;
    return false;
}

bool listed(const IvfLaunch &p) {
    switch (p.family) {
        case ScanFamily::scan: return listed(kKeysIvfScan, p.key);
        case ScanFamily::scan_i8: return listed(kKeysIvfScanI8, p.key);
        case ScanFamily::ivf_kloop: return listed(kKeysIvfKloop, p.key);
        default: return false;
    }
}

std::string key_json(ScanFamily f, const ScanKey &k) {
    std::string s = "[";
    for (int i = 0; i < kScanFamilyArgs[(int)f]; ++i) s += (i ? "," : "") + std::to_string(k.t[i]);
    return s + "]";
}

std::string launch_json(const IvfLaunch &p) {
    char buf[256];
    snprintf(buf, sizeof buf, "{\"family\":\"%s\",\"targs\":%s,\"grid_x\":%u,\"grid_y\":%u,\"block\":%u,\"part_spans\":%d,\"listed\":%s}",
             kScanFamilyNames[(int)p.family], key_json(p.family, p.key).c_str(), p.grid_x, p.grid_y, p.block, p.part_spans,
             listed(p) ? "true" : "false");
    return buf;
}

template <size_t N>
void print_keys(ScanFamily f, const ScanKey (&keys)[N]) {
    printf("{\"family\":\"%s\",\"keys\":[", kScanFamilyNames[(int)f]);
    for (size_t i = 0; i < N; ++i) printf("%s%s", i ? "," : "", key_json(f, keys[i]).c_str());
    printf("]}\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--keys")) {
        print_keys(ScanFamily::scan, kKeysIvfScan);
        print_keys(ScanFamily::scan_i8, kKeysIvfScanI8);
        print_keys(ScanFamily::ivf_kloop, kKeysIvfKloop);
        return 0;
    }
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        long long N = 0, pspans = 0, nq = 0;
        int nlist = 0, max_pspans = 0, d = 0, k = 0, nprobe = 0, used = 0;
        if (sscanf(line, "%lld %d %lld %d %d %d %lld %d%n", &N, &nlist, &pspans, &max_pspans, &d, &k, &nq, &nprobe, &used) < 8) continue;
        Options opt;
        Corpus c;
        for (char *tok = strtok(line + used, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
            char *eq = strchr(tok, '=');
            if (!eq) { fprintf(stderr, "ivf_plan: '%s' is not name=value\n", tok); return 2; }
            *eq = 0;
            const int v = atoi(eq + 1);
            bool known = true;
            if (!strcmp(tok, "i8_ok")) c.i8_ok = v;
            else if (!strcmp(tok, "codec")) c.codec = v;
            else if (!strcmp(tok, "mfma_ok")) c.mfma_ok = v;
            else {
                known = false;
                for (const Named &n : kNamed)
                    if (!strcmp(tok, n.name)) { opt.*n.m = v; known = true; }
            }
            if (!known) { fprintf(stderr, "ivf_plan: unknown name '%s'\n", tok); return 2; }
        }
        const IvfIndexShape s = shape_of(N, nlist, pspans, max_pspans, d, opt, c);
        const IvfGeom g = ivf_geometry(s, opt, nq, k, nprobe);
        printf("{\"tile16\":%d,\"tps\":%d,\"span_rows\":%d,\"ok\":%s", s.tile16 ? 1 : 0, s.tps, s.span_rows, g.ok ? "true" : "false");
        if (!g.ok) {
            printf(",\"exact\":{\"S\":%lld}}\n", (long long)ivf_exact_splits(N, nlist, nprobe, nq, k));
            continue;
        }
        const IvfCaps cp = ivf_caps(s, opt, g, k);
        const IvfSelectCaps se = ivf_select_caps(s, g, cp, k, nprobe);
        printf(",\"kloop\":%s,\"bt\":%d,\"bps\":%d,\"bins_per_span\":%d,\"bin_rows\":%d,\"nw\":%d,\"group\":%d,\"run_groups\":%d,\"pairs\":%lld,"
               "\"max_items\":%lld,\"max_slots\":%lld,\"max_bins\":%lld,\"bin_bytes\":%llu,\"cnt_words\":%llu",
               g.kloop ? "true" : "false", g.bt, g.bps, g.bins_per_span, g.bin_rows, g.nw, g.group, g.run_groups, (long long)g.pairs,
               (long long)g.max_items, (long long)g.max_slots, (long long)g.max_bins, (unsigned long long)g.bin_bytes,
               (unsigned long long)g.cnt_words);
        printf(",\"caps\":{\"use_i8\":%s,\"small_ppb\":%s,\"kgroup\":%d,\"cand_cap\":%d,\"rescan_cap\":%d,\"ppb\":%d,\"pblocks\":%u,\"hist_bytes\":%llu}",
               cp.use_i8 ? "true" : "false", cp.small_ppb ? "true" : "false", cp.kgroup, cp.cand_cap, cp.rescan_cap, cp.ppb, cp.pblocks,
               (unsigned long long)cp.hist_bytes);
        printf(",\"select\":{\"max_entries\":%d,\"probe_cap\":%d,\"vals_entries\":%d,\"act_cap\":%d,\"nm\":%d}", se.max_entries, se.probe_cap,
               se.vals_entries, se.act_cap, se.nm);
        if (g.kloop) printf(",\"f16\":null,\"i8\":null,\"kloop_launch\":%s", launch_json(plan_ivf_kloop(s, opt, g, cp.kgroup)).c_str());
        else printf(",\"f16\":%s,\"i8\":%s,\"kloop_launch\":null", launch_json(plan_ivf_f16(s, opt, g)).c_str(),
                    cp.use_i8 ? launch_json(plan_ivf_i8(s, opt, g)).c_str() : "null");
        printf(",\"exact\":null}\n");
    }
    return 0;
}

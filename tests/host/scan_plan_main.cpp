// scan_plan_main.cpp -- prints what the launch rules of csrc/scan_plan.hpp decide, without HIP or a GPU.
//
//   scan_plan --keys       one JSON line per kernel family: every instantiation the library holds
//   scan_plan < cases      one JSON line per case
// A case is `Npad d k nq` followed by `name=value` pairs: options of vdb_set_option that the rules read, and what an add derives
// from the corpus -- i8_ok (byte-valued rows: an int8 copy exists), pq (a PQ<M> index), n_cus.  Npad is the padded row count the
// add computed.  The index shape follows build_derived / build_int8_only / pq_add (vdbhip.hip, pq.inc), restated in shape_of below.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../vectordb-retrieval_amd/csrc/scan_plan.hpp"

using namespace vdb;

namespace {

struct Named {
    const char *name;
    int Options::*m;
};
constexpr Named kNamed[] = {
    {"spans_per_chunk", &Options::spans_per_chunk}, {"small_batch", &Options::small_batch}, {"i8_variant", &Options::i8_variant},
    {"i8_group", &Options::i8_group}, {"f16_group", &Options::f16_group}, {"flat_shape", &Options::flat_shape},
    {"scan_pair", &Options::scan_pair}, {"f16_wide", &Options::f16_wide}, {"f16_stage_tiles", &Options::f16_stage_tiles},
    {"i8_nt", &Options::i8_nt}, {"i8_ring", &Options::i8_ring}, {"kloop_qgroup", &Options::kloop_qgroup},
    {"panel_dtype", &Options::panel_dtype}, {"int8_only", &Options::int8_only}, {"stream_panels", &Options::stream_panels},
};

struct Corpus {
    int i8_ok = 0, pq = 0, n_cus = 256;
};

ScanIndexShape shape_of(int64_t Npad, int d, const Options &opt, const Corpus &c) {
    ScanIndexShape s;
    s.Npad = Npad;
    s.n_cus = c.n_cus;
    s.ksteps = d <= 64 ? 4 : (d <= 128 ? 8 : (d + 63) / 64 * 4);
    s.i8_ks = d <= 64 ? 2 : 4;
    s.pq = c.pq != 0;
    const bool x16_wanted = s.ksteps <= kMaxKSteps && opt.flat_shape != 32 && opt.f16_group == 8 && opt.i8_group == 8;
    if (s.pq) {
        s.tile16 = s.ksteps > kMaxKSteps;
        s.x16 = !s.tile16;
        return s;
    }
    s.tile16 = s.ksteps > kMaxKSteps && Npad > 2048;
    s.i8_ok = c.i8_ok && d <= 128 && !s.tile16;
    s.int8_only = opt.int8_only && s.i8_ok;
    s.x16 = x16_wanted && (s.int8_only || Npad > 15360);
    s.panels_streamed = s.tile16 && opt.stream_panels != 0;
    return s;
}

template <size_t N>
bool listed(const ScanKey (&keys)[N], const ScanKey &k) {
    for (const ScanKey &r : keys)
        if (r == k) return true;
    return false;
}

bool listed(const ScanLaunch &p) {
    switch (p.family) {
        case ScanFamily::scan: return listed(kKeysScan, p.key);
        case ScanFamily::scan16_kloop: return listed(kKeysScan16Kloop, p.key);
        case ScanFamily::scan_x16: return listed(kKeysScanX16, p.key);
        case ScanFamily::scan_i8: return listed(kKeysScanI8, p.key);
        case ScanFamily::scan_i8x16: return listed(kKeysScanI8x16, p.key);
        case ScanFamily::scan_pair_x16: return listed(kKeysScanPairX16, p.key);
        default: return false;
    }
}

std::string key_json(ScanFamily f, const ScanKey &k) {
    std::string s = "[";
    for (int i = 0; i < kScanFamilyArgs[(int)f]; ++i) s += (i ? "," : "") + std::to_string(k.t[i]);
    return s + "]";
}

std::string launch_json(const ScanLaunch &p) {
    if (p.family == ScanFamily::none) return "null";
    char buf[256];
    snprintf(buf, sizeof buf, "{\"family\":\"%s\",\"targs\":%s,\"grid\":%u,\"block\":%u,\"nqtiles\":%d,\"nqtiles8\":%d,\"qgroup\":%d,\"listed\":%s}",
             kScanFamilyNames[(int)p.family], key_json(p.family, p.key).c_str(), p.grid, p.block, p.nqtiles, p.nqtiles8, p.qgroup,
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
        print_keys(ScanFamily::scan, kKeysScan);
        print_keys(ScanFamily::scan16_kloop, kKeysScan16Kloop);
        print_keys(ScanFamily::scan_x16, kKeysScanX16);
        print_keys(ScanFamily::scan_i8, kKeysScanI8);
        print_keys(ScanFamily::scan_i8x16, kKeysScanI8x16);
        print_keys(ScanFamily::scan_pair_x16, kKeysScanPairX16);
        return 0;
    }
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        long long Npad = 0, nq = 0;
        int d = 0, k = 0, used = 0;
        if (sscanf(line, "%lld %d %d %lld%n", &Npad, &d, &k, &nq, &used) < 4) continue;
        Options opt;
        Corpus c;
        for (char *tok = strtok(line + used, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
            char *eq = strchr(tok, '=');
            if (!eq) { fprintf(stderr, "scan_plan: '%s' is not name=value\n", tok); return 2; }
            *eq = 0;
            const long long v = atoll(eq + 1);
            bool known = true;
            if (!strcmp(tok, "i8_ok")) c.i8_ok = (int)v;
            else if (!strcmp(tok, "pq")) c.pq = (int)v;
            else if (!strcmp(tok, "n_cus")) c.n_cus = (int)v;
            else if (!strcmp(tok, "stream_slab_rows")) opt.stream_slab_rows = v;
            else {
                known = false;
                for (const Named &n : kNamed)
                    if (!strcmp(tok, n.name)) { opt.*n.m = (int)v; known = true; }
            }
            if (!known) { fprintf(stderr, "scan_plan: unknown name '%s'\n", tok); return 2; }
        }
        const ScanIndexShape s = shape_of(Npad, d, opt, c);
        ScanGeom g = scan_geometry(s, opt, k, nq);
        int direct_rows = 0;
        if (!g.ok) direct_rows = scan_geometry_direct(s, opt, k, g);
        const int64_t Qpad = (nq + 511) / 512 * 512;
        const int nw = nw_small(opt, nq);
        printf("{\"tile16\":%d,\"x16\":%d,\"ok\":%s,\"nspans\":%lld,\"spc\":%d,\"rem\":%d,\"nchunks\":%d,\"vpl\":%d,\"direct_rows\":%d,\"nw_small\":%d",
               s.tile16 ? 1 : 0, s.x16 ? 1 : 0, g.ok ? "true" : "false", (long long)g.nspans, g.spc, g.rem, g.nchunks, g.vpl, direct_rows, nw);
        if (g.ok) {
            const bool i8 = use_i8(s, opt, direct_rows);
            const ScanLaunch pair = plan_pair(s, opt, g.nchunks, Qpad, nq, direct_rows, nw);
            printf(",\"use_i8\":%s,\"pair\":%s,\"pair_candidate\":%s,\"wide\":%s,\"f16_octs\":%s,\"f16\":%s,\"i8\":%s,\"pair_launch\":%s",
                   i8 ? "true" : "false", pair.family != ScanFamily::none ? "true" : "false",
                   pair_candidate(s, opt, direct_rows) ? "true" : "false", wide_tiles(g.nchunks, Qpad) ? "true" : "false",
                   f16_octs(s, opt, direct_rows) ? "true" : "false",
                   launch_json(plan_f16(s, opt, g.nchunks, Qpad, nq, direct_rows, nw)).c_str(),
                   i8 ? launch_json(plan_i8(s, opt, g.nchunks, Qpad, nq, nw)).c_str() : "null", launch_json(pair).c_str());
            if (s.panels_streamed) printf(",\"stream_slab_chunks\":%lld", (long long)stream_slab_chunks(s, opt, g, Qpad));
        }
        printf("}\n");
    }
    return 0;
}

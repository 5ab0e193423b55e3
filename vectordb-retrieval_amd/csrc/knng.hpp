// knng.hpp -- kernels of the k-NN graph index (host side: knng.inc; contract: include/vdbhip.h).
//
//   knng_strip_self_kernel  the partial lists of a self-search block -> local int32 candidates + their sortable float64 keys
//   knng_prune_kernel       HNSW neighbour heuristic over the candidates of a row, rejected candidates kept as fill
//   knng_search_kernel      beam search: one wave per query, the list L, the query and a lossy "seen" filter in LDS
//
// Every distance is the canonical float64 chain of refine.hpp (exact_key / row_key), every order is (key, local row).
#pragma once
#include "common.hpp"
#include "refine.hpp"

namespace vdb {

constexpr int kKnngMinDegree = 4, kKnngMaxDegree = 64, kKnngMaxCand = 128, kKnngMaxEf = 512;
constexpr unsigned kKnngEmpty = 0x7fffffffu;      // id of an empty slot of L (no row has it: ntotal < 2^31 - 1024); its key is all ones
constexpr unsigned kKnngExpanded = 0x80000000u;   // the "expanded" flag of an entry travels in the top bit of its id
constexpr unsigned long long kKnngNoKey = ~0ull;

// LDS operations of ONE wave execute in program order; this keeps the compiler from moving them across the point where
// the lanes of the wave exchange data through LDS (no s_barrier: the waves of a workgroup run independent queries)
__device__ __forceinline__ void knng_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- build: strip ------------------------------------------------------------------------------------------------------------
struct KnngStripArgs {
    const double *pk;          // (nrows, k) keys of vdb_search_partial_device, ascending by (key, id)
    const int64_t *pi;         // (nrows, k) global ids, -1 = missing
    int64_t row0, nrows;       // the block holds the rows [row0, row0 + nrows) as queries
    int k, ncand;              // k = min(ncand + 1, ntotal)
    int64_t id_base;
    int32_t *cand;             // (nrows, ncand) local row numbers, -1 tail
    unsigned long long *ckeys; // (nrows, ncand) sortable keys
};

// one wave per row: drop the entry that is the row itself (or, when duplicates of the row with smaller ids pushed it out of
// its own list, the last entry), close the gap
__global__ __launch_bounds__(256) void knng_strip_self_kernel(KnngStripArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.nrows) return;
    const int64_t self = a.id_base + a.row0 + r;
    const double *pk = a.pk + (size_t)r * a.k;
    const int64_t *pi = a.pi + (size_t)r * a.k;
    int sp = a.k - 1;
    for (int j0 = 0; j0 < a.k; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long m = __ballot(j < a.k && pi[j] == self);
        if (m) {
            sp = j0 + __ffsll(m) - 1;
            break;
        }
    }
    for (int j = lane; j < a.ncand; j += 64) {
        const int src = j < sp ? j : j + 1;
        int32_t c = -1;
        unsigned long long key = kKnngNoKey;
        if (src < a.k) {
            const int64_t id = pi[src];
            if (id >= 0) {
                c = (int32_t)(id - a.id_base);
                key = sortable_u64(pk[src]);
            }
        }
        a.cand[(size_t)r * a.ncand + j] = c;
        a.ckeys[(size_t)r * a.ncand + j] = key;
    }
}

// ---- build: prune ------------------------------------------------------------------------------------------------------------
struct KnngPruneArgs {
    const float *X;            // [N][D4]
    int D4, metric;
    int64_t row0, nrows;
    int ncand, degree;
    const int32_t *cand;
    const unsigned long long *ckeys;
    int32_t *nbrs;             // [N][degree]
};

// one wave per row i.  Candidate e (key(i, e) given) is selected while |S| < degree unless some s in S has key(e, s) < key(i, e):
// lane l < |S| walks the chain of key(e, S[l]) (row e is the query, row S[l] the row), one ballot decides.  The stored row is S,
// then the rejected candidates in candidate order, then -1.
__global__ __launch_bounds__(256) void knng_prune_kernel(KnngPruneArgs a) {
    __shared__ int32_t sel[4][kKnngMaxDegree];
    __shared__ int32_t rej[4][kKnngMaxCand];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + w;
    if (r >= a.nrows) return;
    const int32_t *cand = a.cand + (size_t)r * a.ncand;
    const unsigned long long *ckeys = a.ckeys + (size_t)r * a.ncand;
    int ns = 0, nr = 0;
    for (int c = 0; c < a.ncand; ++c) {
        const int e = __builtin_amdgcn_readfirstlane(cand[c]);
        if (e < 0) break;
        bool reject = ns >= a.degree;
        if (!reject) {
            const unsigned long long ke = ckeys[c];
            bool closer = false;
            if (lane < ns) closer = exact_key<4>(a.X + (size_t)sel[w][lane] * a.D4, a.X + (size_t)e * a.D4, a.D4, a.metric) < ke;
            reject = __ballot(closer) != 0ull;
        }
        if (lane == 0) {
            if (reject) rej[w][nr] = e;
            else sel[w][ns] = e;
        }
        if (reject) ++nr;
        else ++ns;
        knng_wave_sync();
    }
    if (lane < a.degree) {
        int32_t v = -1;
        if (lane < ns) v = sel[w][lane];
        else if (lane - ns < nr) v = rej[w][lane - ns];
        a.nbrs[(size_t)(a.row0 + r) * a.degree + lane] = v;
    }
}

// ---- search ------------------------------------------------------------------------------------------------------------------
struct KnngSearchArgs {
    RefineCommon c;            // the float32 rows; c.Q = the queries padded to D4
    const int32_t *nbrs;
    int degree;
    int64_t nq;
    int k, ef, max_iters;
    const int32_t *entries;    // the entry points: the distinct rows floor(j N / nentry), j < min(nentry, ef, N), ascending (the host lists them)
    int nentries;
    int vbits;                 // log2 slots of the seen filter
    int waves;                 // queries (waves) per workgroup
    int phases;                // 1 entry scoring | 2 traversal | 4 results; all three in one launch unless the call is timed
    unsigned long long *st_keys;   // timed calls: L between the launches, [nq][64 EPL]
    unsigned *st_ids;
    unsigned long long *stat;  // sharded counters: 0 rows scored, 1 queries stopped by max_iters
    float *D;
    int64_t *I;
};

// bytes of LDS one query needs: L (keys, ids), the step's survivors (keys, ids), the query, the filter
__host__ __device__ inline size_t knng_wave_lds(int efp, int D4, int vbits) {
    return (size_t)efp * 12 + 64 * 12 + (size_t)D4 * 4 + ((((size_t)4 << vbits) + 15) & ~(size_t)15);      // (16-byte multiples)
}

__device__ __forceinline__ bool knng_less(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
    return ka < kb || (ka == kb && ia < ib);
}

struct KnngWave {
    unsigned long long *keys;  // L, ascending by (key, id); empty slots (all ones, kKnngEmpty) behind the nL entries
    unsigned *ids;
    unsigned long long *skeys; // the survivors of the current step, one per lane
    unsigned *sids;
    float *q;
    int *filt;
    int nL;                    // entries of L (wave-uniform)
    int scored;                // rows scored so far (wave-uniform)
};

// One set operation L <- best ef of (L u scored): lane `lane` offers row `cand` (-1: nothing); only lanes below `m` may offer one.
// A row the filter remembers was scored before, and a row that is in L now needs no score: both are dropped.  The others are scored and
// everything lands at its rank among (L u survivors); ranks >= ef are dropped.
template <int EPL>
__device__ __forceinline__ void knng_absorb(const KnngSearchArgs &a, KnngWave &s, int lane, int cand, int m) {
    constexpr int EFP = 64 * EPL;
    bool live = cand >= 0;
    if (live) {
        const unsigned slot = ((unsigned)cand * 2654435761u) >> (32 - a.vbits);
        if (s.filt[slot] == cand) live = false;
        else s.filt[slot] = cand;                  // (a collision overwrites: the filter forgets, it never invents)
    }
    if (__ballot(live) == 0ull) return;
    {   // exact de-duplication against the current L
        const uint4 *ids4 = reinterpret_cast<const uint4 *>(s.ids);
        const unsigned cu = (unsigned)cand;
        for (int i = 0; i < (s.nL + 3) / 4; ++i) {
            const uint4 v = ids4[i];
            if ((v.x & kKnngEmpty) == cu || (v.y & kKnngEmpty) == cu || (v.z & kKnngEmpty) == cu || (v.w & kKnngEmpty) == cu) live = false;
        }
    }
    unsigned long long key = kKnngNoKey;
    unsigned id = kKnngEmpty;
    if (live) {
        key = row_key<4>(a.c, cand, s.q);
        id = (unsigned)cand;
    }
    const int ns = __popcll(__ballot(live));
    if (ns == 0) return;
    s.scored += ns;
    s.skeys[lane] = key;
    s.sids[lane] = id;
    knng_wave_sync();
    unsigned long long lk[EPL];
    unsigned li[EPL];
    int add[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        lk[j] = s.keys[j * 64 + lane];
        li[j] = s.ids[j * 64 + lane];
        add[j] = 0;
    }
    int rank = 0;
    if (live) {          // entries of L in front of this survivor: lower bound in the sorted list (at most 10 halvings of 512)
        int lo = 0, hi = s.nL;
        for (int it = 0; it < 10 && lo < hi; ++it) {
            const int mid = (lo + hi) >> 1;
            if (knng_less(s.keys[mid], s.ids[mid] & kKnngEmpty, key, id)) lo = mid + 1;
            else hi = mid;
        }
        rank = lo;
    }
    for (int t = 0; t < m; ++t) {
        const unsigned si = s.sids[t];
        if (si == kKnngEmpty) continue;
        const unsigned long long sk = s.skeys[t];
        rank += (live && knng_less(sk, si, key, id)) ? 1 : 0;
#pragma unroll
        for (int j = 0; j < EPL; ++j) add[j] += knng_less(sk, si, lk[j], li[j] & kKnngEmpty) ? 1 : 0;
    }
    knng_wave_sync();
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int pos = j * 64 + lane + add[j];
        if (add[j] != 0 && pos < a.ef) {
            s.keys[pos] = lk[j];
            s.ids[pos] = li[j];
        }
    }
    if (live && rank < a.ef) {
        s.keys[rank] = key;
        s.ids[rank] = id;
    }
    s.nL = min(a.ef, s.nL + ns);
    knng_wave_sync();
    (void)EFP;
}

template <int EPL>
__global__ __launch_bounds__(256) void knng_search_kernel(KnngSearchArgs a) {
    constexpr int EFP = 64 * EPL;
    extern __shared__ __attribute__((aligned(16))) unsigned char knng_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t q = (int64_t)blockIdx.x * a.waves + wave;
    if (q >= a.nq) return;
    const int D4 = a.c.D4;
    unsigned char *base = knng_smem + (size_t)wave * knng_wave_lds(EFP, D4, a.vbits);
    KnngWave s;
    s.keys = reinterpret_cast<unsigned long long *>(base);
    s.skeys = s.keys + EFP;
    s.ids = reinterpret_cast<unsigned *>(s.skeys + 64);
    s.sids = s.ids + EFP;
    s.q = reinterpret_cast<float *>(s.sids + 64);
    s.filt = reinterpret_cast<int *>(s.q + D4);
    s.nL = 0;
    s.scored = 0;
    for (int i = lane; i < D4; i += 64) s.q[i] = a.c.Q[(size_t)q * D4 + i];
    for (int i = lane; i < (1 << a.vbits); i += 64) s.filt[i] = -1;
    if (a.phases & 1) {
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            s.keys[j * 64 + lane] = kKnngNoKey;
            s.ids[j * 64 + lane] = kKnngEmpty;
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            const unsigned id = a.st_ids[(size_t)q * EFP + j * 64 + lane];
            s.keys[j * 64 + lane] = a.st_keys[(size_t)q * EFP + j * 64 + lane];
            s.ids[j * 64 + lane] = id;
            s.nL += __popcll(__ballot(id != kKnngEmpty));
        }
    }
    knng_wave_sync();

    if (a.phases & 1) {        // entry points, 64 per set operation (at most ef of them: every one is inserted)
        for (int j0 = 0; j0 < a.nentries; j0 += 64) {
            const int j = j0 + lane;
            const int cand = j < a.nentries ? a.entries[j] : -1;
            knng_absorb<EPL>(a, s, lane, cand, 64);
        }
    }

    if (a.phases & 2) {
        int it = 0;
        bool open = true;          // an unexpanded entry may be left
        for (; it < a.max_iters; ++it) {
            int p = -1;
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const int e = j * 64 + lane;
                const unsigned long long mk = __ballot(e < s.nL && !(s.ids[e] & kKnngExpanded));
                if (p < 0 && mk) p = j * 64 + __ffsll(mk) - 1;
            }
            if (p < 0) {
                open = false;
                break;
            }
            const unsigned node = (unsigned)__builtin_amdgcn_readfirstlane((int)s.ids[p]);
            knng_wave_sync();
            if (lane == 0) s.ids[p] = node | kKnngExpanded;
            knng_wave_sync();
            const int cand = lane < a.degree ? a.nbrs[(size_t)node * a.degree + lane] : -1;
            knng_absorb<EPL>(a, s, lane, cand, a.degree);
        }
        if (open) {                // the cap ended the loop: does it matter?
            bool any = false;
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const int e = j * 64 + lane;
                any |= __ballot(e < s.nL && !(s.ids[e] & kKnngExpanded)) != 0ull;
            }
            if (any && lane == 0) stat_add(a.stat, q, 1, 1ull);
        }
    }
    if (lane == 0 && s.scored) stat_add(a.stat, q, 0, (unsigned long long)s.scored);

    if (a.phases & 4) {
        for (int i = lane; i < a.k; i += 64) {
            const bool have = i < s.nL;
            const double kv = unsortable_f64(s.keys[i]);
            float d;
            if (have) d = (float)(a.c.metric == 0 ? kv : -kv);
            else d = (a.c.metric == 0) ? 3.402823466e+38f : -3.402823466e+38f;
            a.D[(size_t)q * a.k + i] = d;
            a.I[(size_t)q * a.k + i] = have ? (int64_t)(s.ids[i] & kKnngEmpty) + a.c.id_base : -1;
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            a.st_keys[(size_t)q * EFP + j * 64 + lane] = s.keys[j * 64 + lane];
            a.st_ids[(size_t)q * EFP + j * 64 + lane] = s.ids[j * 64 + lane];
        }
    }
}

}  // namespace vdb

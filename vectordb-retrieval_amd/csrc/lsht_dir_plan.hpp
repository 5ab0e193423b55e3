// lsht_dir_plan.hpp -- the bucket directory of the hash-table LSH (lsht_dir.hpp; option "lsht_directory"): slot hash, slot count,
// directory bytes, workgroups per query and the rule that routes a call to the lookup or to the vote scan.  Plain host C++ (the hash is
// __host__ __device__ under hipcc), so tests/host/lsht_dir_plan_main.cpp prints what the rules give.
//
// Per table t a CSR over S hash slots: offsets[t][S + 1] and rows[t][N], int32.  slot = lsht_dir_hash(the W key words of table t) &
// (S - 1): rows with equal table keys share a slot, rows with different keys may (the lookup compares the full key).  S is the power
// of two at or above N, at least 1024: a directory of all-distinct keys has about one row per slot.
//
// The rule needs no round trip per call: the build leaves visits = sum over tables and slots of count^2, which is N x the bucket
// entries a query distributed like the rows walks.  A walked entry is a gathered key row; the scan reads every key word of every row,
// coalesced and shared by a tile of queries.  The lookup serves a call of nq queries when
//     visits / N * gather cost(nq) <= N * kw * kLshtDirWordCost             (kw = stored key words per row)
// The gather cost was derived as 16 (one 64-byte request per gathered table key of at most 16 words, against one coalesced word of
// the scan) and then set from the measured break-even (DESIGN 4.12 "Bucket directory"; profiles/r36_bench_lsht_directory.json): the
// vote scan is bound by compares on registers, not by its reads, so a walked entry costs 120 - 300 of its words in batches of 1 and
// 64 queries and 280 - 730 in a batch of 10 000, where the scan shares every key read among 256 queries and the gathers of 10 000
// lookups evict each other.  Hence two weights, split at the scan's query tile; batches between 64 and 10 000 were not measured.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VDB_LSHT_DIR_HD __host__ __device__
#else
#define VDB_LSHT_DIR_HD
#endif

namespace vdb {

constexpr int kLshtDirMinSlots = 1024;               // S >= this (a multiple of the 1024 counts one step of the prefix scan takes)
constexpr int kLshtDirThreads = 256;                 // threads of a lookup workgroup: one bucket entry per thread and step
constexpr int kLshtDirEntriesPerGroup = 4096;        // expected bucket entries per lookup workgroup
constexpr int kLshtDirMaxSplits = 16;                // workgroups per query at most
constexpr double kLshtDirGatherCostDerived = 16.0;   // derived: a 64-byte request per gathered key of <= 16 words
constexpr int kLshtDirSmallBatch = 256;              // queries of one tile of the vote scan: up to here a batch is "small"
constexpr double kLshtDirGatherCostSmall = 180.0;    // in force, measured: batches of at most kLshtDirSmallBatch queries
constexpr double kLshtDirGatherCost = 500.0;         // ... larger batches
constexpr double kLshtDirWordCost = 1.0;             // one key word of one row in the vote scan

// one step per key word, then the finalizer of MurmurHash3
VDB_LSHT_DIR_HD inline uint32_t lsht_dir_mix(uint32_t h, uint32_t word) {
    h = (h ^ word) * 0x9e3779b1u;
    return h ^ (h >> 15);
}
VDB_LSHT_DIR_HD inline uint32_t lsht_dir_finish(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}
VDB_LSHT_DIR_HD inline uint32_t lsht_dir_hash(const uint32_t *words, int W) {
    uint32_t h = 0x811c9dc5u;
    for (int w = 0; w < W; ++w) h = lsht_dir_mix(h, words[w]);
    return lsht_dir_finish(h);
}

// S = max(1024, the power of two at or above n)
inline int64_t lsht_dir_slots(int64_t n) {
    int64_t s = kLshtDirMinSlots;
    while (s < n) s <<= 1;
    return s;
}
// the directory serves n rows: offsets and row numbers are int32, and S has to be one too
inline bool lsht_dir_fits(int64_t n) { return n > 0 && n <= ((int64_t)1 << 30); }
inline size_t lsht_dir_bytes(int T, int64_t n) { return (size_t)T * (size_t)(lsht_dir_slots(n) + 1 + n) * sizeof(int32_t); }
// the build's temporary: one cursor per slot and table, and the 8 bytes of `visits`
inline size_t lsht_dir_tmp_bytes(int T, int64_t n) { return (size_t)T * (size_t)lsht_dir_slots(n) * sizeof(int32_t) + 8; }

// bucket entries a query like the rows walks
inline double lsht_dir_entries_per_query(unsigned long long visits, int64_t n) { return n > 0 ? (double)visits / (double)n : 0.0; }

// workgroups per query: about kLshtDirEntriesPerGroup expected entries each
inline int lsht_dir_splits(unsigned long long visits, int64_t n) {
    const double e = lsht_dir_entries_per_query(visits, n);
    const double s = (e + kLshtDirEntriesPerGroup - 1) / kLshtDirEntriesPerGroup;
    return s < 1.0 ? 1 : s > kLshtDirMaxSplits ? kLshtDirMaxSplits : (int)s;
}

// option "lsht_directory" = 1: does the lookup serve the call?  (2: always; 0: never)
inline double lsht_dir_gather_cost(int64_t nq) { return nq <= kLshtDirSmallBatch ? kLshtDirGatherCostSmall : kLshtDirGatherCost; }
inline bool lsht_dir_rule(unsigned long long visits, int64_t n, int kw, int64_t nq) {
    return lsht_dir_entries_per_query(visits, n) * lsht_dir_gather_cost(nq) <= (double)n * (double)kw * kLshtDirWordCost;
}
inline bool lsht_dir_use(int option, unsigned long long visits, int64_t n, int kw, int64_t nq) {
    return option == 2 || (option == 1 && lsht_dir_rule(visits, n, kw, nq));
}

}  // namespace vdb

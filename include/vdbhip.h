/*
 * vdbhip.h -- C-ABI of libvdbhip.so, the MI355X (gfx950) brute-force / IVF-Flat k-NN backend.
 *
 * This is the drop-in boundary for ONE hot path of Human-Augment-Analytics/vectordb-retrieval:
 * what the reference delegates to `faiss.IndexFlat` / `faiss.IndexIVFFlat` / NumPy on behalf of
 *   src/algorithms/exact_search.py:26-78        ExactSearch.build_index / search / batch_search
 *   src/algorithms/modular.py:121-133, 312-390  BruteForceIndexer.build, LinearSearcher.*
 *   src/algorithms/modular.py:244-309, 418-449, 536-548  FaissFactory/IVFIndexer.build, FaissSearcher.*
 *   src/algorithms/approximate_search.py:28-87  ApproximateSearch (IVFn,Flat keys)
 *   src/benchmark/dataset.py:497-504, 858-964   brute-force ground truth
 * Plain pointers and sizes only; no torch / numpy types.  The reference-side binding (ctypes) is
 * shown in INTEGRATION.md and implemented in vectordb-retrieval_amd/vdbhip/_ffi.py.
 *
 * Conventions (identical to faiss.IndexFlat, i.e. what ExactSearch.batch_search returns,
 * exact_search.py:78):
 *   metric VDB_METRIC_L2 : distances are SQUARED L2, ascending.
 *   metric VDB_METRIC_IP : "distances" are raw inner products, descending.
 *   ids are int64 row numbers (+ id_base of vdb_add); when k > ntotal the tail is padded with
 *   id -1 and distance +FLT_MAX (L2) / -FLT_MAX (IP).
 *   Ties are broken by the smaller id (shard-count invariant).
 * The LinearSearcher / FaissSearcher conventions (sqrt, negated scores, cosine = normalise + IP,
 * +inf padding; modular.py:355-360, 381-385, 545-546) are applied by the Python shim on the (nq,k) output.
 *
 * Exactness contract: the neighbours returned are the exact k nearest under float64 arithmetic
 *   L2: sum_d fma(t,t,.) with t = (double)x[d]-(double)q[d];  IP: sum_d fma((double)q[d],(double)x[d],.)
 * (d ascending), the order key being (value, id).  The fp16 MFMA scan only nominates candidates;
 * every returned neighbour is re-scored in this arithmetic and a rigorous error bound guarantees that
 * no true neighbour was left out (DESIGN.md "exactness guard").
 *
 * Threading: a handle may be used from one host thread at a time.  All calls return a status
 * code; vdb_last_error() gives the message of the last failure on the calling thread.
 */
#ifndef VDBHIP_H
#define VDBHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDB_ABI_VERSION 4

typedef struct vdb_index_s *vdb_handle;

enum vdb_metric { VDB_METRIC_L2 = 0, VDB_METRIC_IP = 1 };

enum vdb_status {
    VDB_OK = 0,
    VDB_ERR_INVALID = 1,     /* bad argument (maps to ValueError at build time, RuntimeError at search time) */
    VDB_ERR_STATE = 2,       /* e.g. search before add: "Index has not been built yet." (exact_search.py:53-54) */
    VDB_ERR_HIP = 3,         /* HIP runtime failure */
    VDB_ERR_NOMEM = 4,
    VDB_ERR_UNSUPPORTED = 5
};

/* which search path served the last call (vdb_stats_t.last_path) */
enum vdb_path { VDB_PATH_NONE = 0, VDB_PATH_EXACT_SCAN = 1, VDB_PATH_MFMA_SCAN = 2, VDB_PATH_IVF = 3, VDB_PATH_LSH = 4, VDB_PATH_KNNG = 5, VDB_PATH_LSHT = 6,
                VDB_PATH_PQ_ADC = 7 /* flat PQ: lookup-table (ADC) scan of the codes, then the select and exact refine of the MFMA scan */,
                VDB_PATH_IVFPQ_ADC = 8 /* IVF-PQ: lookup-table (ADC) scan of the probed lists, then the exact re-score of the rows near the k-th score */,
                VDB_PATH_RANGE = 9 /* vdb_range_search: bitmap prefilter (fp16 MFMA scan, or all rows), exact filter, emit in id order */,
                VDB_PATH_FILTER_ROWS = 10 /* vdb_search_filtered, selective filter: exact top-k over the list of admitted rows alone */,
                VDB_PATH_IVF_RANGE = 11 /* vdb_ivf_range_search: candidate bitmap from the list scans' bin minima (or every probed row), exact filter, emit in list order */ };

typedef struct vdb_stats_s {
    int64_t ntotal;            /* rows indexed */
    int32_t dim;
    int32_t metric;
    int64_t bytes_resident;    /* device bytes owned by the handle (index + workspace) */
    int32_t last_path;         /* enum vdb_path */
    int32_t corpus_fp16_exact; /* 1 if every corpus value is exactly representable in the fp16 scan copy */
    int64_t last_nq;
    int64_t last_candidates;   /* candidate groups (4 consecutive rows each; 8 on the flat int8 scan) re-scored exactly (hash-table LSH: candidates) */
    int64_t last_rescan_bins;  /* 256-row bins re-scanned exactly (collision guard) */
    int64_t last_fallback_queries; /* queries whose work list overflowed -> exhaustive exact scan (LSH, hash-table LSH: exact fallback of the select) */
    float last_scan_ms;        /* mean HIP-event time of the dominant (scan) kernel over the searches recorded since
                                  timing was switched on; 0 if not timed */
    float last_total_ms;       /* same for the whole device pipeline */
    int32_t nlist;             /* IVF: number of inverted lists (0 = flat index) */
    int32_t nprobe;
    int32_t scan_dtype;        /* arithmetic of the last MFMA scan: 0 = fp16 (f32 accumulate), 1 = int8 (i32 accumulate),
                                  2 = fp16 panels converted from the 8-bit codes of an SQ8 or PQ index, or from the int8 panels of an IVF-I8
                                  index for a batch its int8 scan cannot serve (f32 accumulate),
                                  3 = float32 lookup-table sums over the codes of a PQ or IVF-PQ index (last_path = VDB_PATH_PQ_ADC /
                                  VDB_PATH_IVFPQ_ADC; there last_candidates counts ROWS re-scored exactly) */
    int32_t has_i8_copy;       /* 1 if the index holds the int8 scan copy (byte-valued integer corpus, D <= 128) next to the float32
                                  rows and the fp16 copy; 2 if it holds ONLY the int8 copies (option "int8_only", or an IVF-I8 index) */
    int64_t last_rows_scanned; /* IVF: (query, row) pairs scanned by the last search (rows of the probed lists); hash-table LSH: ntotal x the
                                  queries that took the brute-force fallback */
    int64_t upload_blocks;     /* row blocks the last vdb_add / vdb_ivf_add streamed through the pinned staging buffers */
    int64_t graph_replays;     /* searches served by launching the captured hipGraph (option "graph") since the handle was made */
    int32_t ndevices;          /* shards of the handle: 1, or the ndev of vdb_create_multi (sums / maxima over the shards above) */
    int32_t scan_shape;        /* rows of the MFMA tile the flat scan copies (D <= 128) are laid out for: 16 = layout "x16"
                                  (v_mfma_*_16x16x32_f16 / 16x16x64_i8, the default above 15 360 rows), 32 = 32x32x16 / 32x32x32
                                  (option "flat_shape" = 32, small corpora, quads); 0 = no such copy (D > 128, empty index) */
    int64_t bytes_workspace;   /* the part of bytes_resident that is per-search workspace (bin arrays, work lists, staging; PQ: and
                                  the slab of fp16 panels made per search) */
    float last_prep_ms;        /* timing on: mean time from the start of the device pipeline to the start of the dominant kernel
                                  (query statistics / operands; IVF: + coarse search, plan) ... */
    float last_tail_ms;        /* ... and from its end to the end of the pipeline (bin select + exact refine): with last_scan_ms
                                  the three stages of a search, so a caller can name the longest one */
} vdb_stats_t;

/* ---- kinds of handle: which calls each admits --------------------------------------------------------------------------
 * Every handle comes from vdb_create (or vdb_create_multi) and is of exactly ONE kind, decided by what has been done to it:
 *   flat      nothing below                              PQ        codebooks of vdb_pq_train / vdb_pq_set_codebooks
 *   LSH       a projection (vdb_lsh_set_projection)      IVF-Flat  centroids or filed rows, codec 0
 *   knng      a k-NN graph (vdb_knng_build / _set;       IVF-SQ8   vdb_ivf_set_codec 1
 *             an add or vdb_reset makes it flat again)   IVF-PQ    vdb_ivf_set_codec 2
 *   multi     vdb_create_multi (flat or IVF-Flat rows)   IVF-I8    vdb_ivf_set_codec 3
 *                                                        LSHT      hash tables (vdb_lsht_set_tables)
 * A call on a kind it does not serve is refused before it looks at its arguments or touches the handle, with a message that names
 * the call and the kind: U = VDB_ERR_UNSUPPORTED, S = VDB_ERR_STATE.  "+" = admitted (the call's own state and argument checks
 * follow: "no centroids", "not built", ...).
 *                                                       flat  LSH  LSHT  knng  PQ   IVF-Flat  IVF-SQ8  IVF-PQ  multi
 *   vdb_add(_device)                                     +     +    +     +    U      +         U        U       +
 *   vdb_search*, vdb_reserve, vdb_reset, vdb_stats,
 *     vdb_set_option, the get_codebooks / get_projection
 *     / get_tables / vdb_knng_get calls (M, nbits, T,
 *     degree 0 elsewhere)                                +     +    +     +    +      +         +        +       +
 *   vdb_rerank(_device)                                  +     +    +     +    +      +         +        S       +
 *   vdb_range_search(_device), vdb_range_results(_device) +    +    +     +    U      U         U        U       U
 *   vdb_filter_set(_device), vdb_filter_count,
 *     vdb_search_filtered(_device)                       +     +    +     +    U      U         U        U       U
 *   vdb_filter_clear                                     +     +    +     +    +      +         +        +       U
 *   vdb_ivf_filter_set(_device), vdb_ivf_filter_count,
 *     vdb_ivf_search_filtered(_device)                   +     U    U     U    U      +         U        U       U
 *   vdb_ivf_range_search(_device),
 *     vdb_ivf_range_results(_device)                     +     U    U     U    U      +         U        U       U
 *   vdb_ivf_train, vdb_ivf_set_centroids                 +     U    U     U    U      +         +        +       +
 *   vdb_ivf_set_codec 1 | 2 | 3                          +     U    U     U    U      +         +        +       U
 *   every other vdb_ivf_* call, vdb_ivf_set_codec 0      +     +    +     +    U      +         +        +       +
 *   vdb_ivf_sq8_*, vdb_ivf_get_codes                     S     S    S     S    U      S         +        U       U
 *   vdb_ivf_i8_get_rows                                  S     S    S     S    U      S         S        U       U
 *   vdb_ivfpq_train / _set_codebooks / _add_codes /
 *     _get_codes                                         S     S    S     S    U      S         S        +       U
 *   vdb_pq_train, vdb_pq_set_codebooks                   +     U    U     U    +      U         U        U       U
 *   vdb_pq_add, vdb_pq_add_codes, vdb_pq_get_codes       S     S    S     S    +      S         S        U       U
 *   vdb_lsh_set_projection                               +     +    U     U    U      U         U        U       U
 *   vdb_lsh_candidates*, vdb_lsh_search*                 S     +    U     U    U      S         S        U       U
 *   vdb_lsh_get_codes                                    S     +    U     S    U      S         S        U       U
 *   vdb_lsht_set_tables                                  +     U    +     U    U      U         U        U       U
 *   vdb_lsht_candidates*, vdb_lsht_search*,
 *     vdb_lsht_get_keys                                  S     U    +     U    U      U         U        U       U
 *   vdb_knng_build, vdb_knng_set, vdb_knng_search*       +     U    U     +    U      U         U        U       U
 *   vdb_debug_scan_scores                                +     +    +     +    +      +         +        +       U
 *   vdb_debug_pq_adc_scores                              U     U    U     U    +      U         U        U       U
 *   vdb_debug_ivfpq_adc_scores                           U     U    U     U    U      U         U        +       U
 *   options refused (U), in either order of the calls:
 *     "int8_only" = 1, "stream_panels" = 1               -     U    U     U    U      -         U        U       -
 *     "graph" = 1                                        -     -    -     -    U      -         U        U       U
 *     "flat_shape" = 32, "f16_group" = 4, "i8_group" = 4 -     -    -     -    U      -         -        -       -
 * The tenth kind, IVF-I8, in a column of its own (the same rows):
 *                                                       IVF-I8
 *   vdb_add(_device)                                    U
 *   vdb_search*, vdb_reserve, vdb_reset, vdb_stats,
 *     vdb_set_option, the get_codebooks / get_projection
 *     / get_tables / vdb_knng_get calls (M, nbits, T,
 *     degree 0 elsewhere)                               +
 *   vdb_rerank(_device)                                 +
 *   vdb_range_search(_device), vdb_range_results(_deviceU
 *   vdb_filter_set(_device), vdb_filter_count,
 *     vdb_search_filtered(_device)                      U
 *   vdb_filter_clear                                    +
 *   vdb_ivf_filter_set(_device), vdb_ivf_filter_count,
 *     vdb_ivf_search_filtered(_device)                  U
 *   vdb_ivf_range_search(_device),
 *     vdb_ivf_range_results(_device)                    U
 *   vdb_ivf_train, vdb_ivf_set_centroids                +
 *   vdb_ivf_set_codec 1 | 2 | 3                         +
 *   every other vdb_ivf_* call, vdb_ivf_set_codec 0     +
 *   vdb_ivf_sq8_*, vdb_ivf_get_codes                    U
 *   vdb_ivf_i8_get_rows                                 +
 *   vdb_ivfpq_train / _set_codebooks / _add_codes /
 *     _get_codes                                        U
 *   vdb_pq_train, vdb_pq_set_codebooks                  U
 *   vdb_pq_add, vdb_pq_add_codes, vdb_pq_get_codes      U
 *   vdb_lsh_set_projection                              U
 *   vdb_lsh_candidates*, vdb_lsh_search*                U
 *   vdb_lsh_get_codes                                   U
 *   vdb_lsht_set_tables                                 U
 *   vdb_lsht_candidates*, vdb_lsht_search*,
 *     vdb_lsht_get_keys                                 U
 *   vdb_knng_build, vdb_knng_set, vdb_knng_search*      U
 *   vdb_debug_scan_scores                               +
 *   vdb_debug_pq_adc_scores                             U
 *   vdb_debug_ivfpq_adc_scores                          U
 *   options refused (U), in either order of the calls:
 *     "int8_only" = 1, "stream_panels" = 1              U
 *     "graph" = 1                                       U
 *     "flat_shape" = 32, "f16_group" = 4, "i8_group" = 4-
 * "Either order": vdb_set_option refuses the value on a handle of the kind, and the call that makes a handle that kind
 * (vdb_lsh_set_projection, vdb_lsht_set_tables, vdb_knng_build / _set, vdb_pq_train / _set_codebooks, vdb_ivf_set_codec 1 | 2 | 3) refuses a handle on
 * which the option holds the value; LSH, LSHT and knng also while an "int8_only" / "stream_panels" of the last add is in effect.  The
 * LSH, hash-table LSH, k-NN graph, range search and filter calls (but vdb_filter_clear) are refused while option "graph" is 1. */

/* ---- library ---------------------------------------------------------------------------- */
int vdb_abi_version(void);
const char *vdb_last_error(void);
int vdb_device_count(int *count);

/* ---- flat (brute-force) index -- replaces faiss.IndexFlat(d, metric) (exact_search.py:38) -- */
int vdb_create(int dim, int metric, int device, vdb_handle *out);
/* ONE index over several GPUs of the node, driven from ONE process -- the form SURVEY 8b proposed
 * (`vdb_create(dim, metric, const int *devs, int ndev, ...)`), because the reference's harness is a single process that calls
 * build_index once and batch_search per batch (src/experiments/experiment_runner.py:329-331, 428-434) on a plugin made from a
 * `type:` string (src/algorithms/__init__.py:37-47).  The handle is an ordinary vdb_handle:
 *   vdb_add / vdb_add_device / vdb_ivf_add(_assigned)  cut the rows of a call into ndev contiguous blocks, block s -> devices[s]
 *                  (SURVEY 8e); ids stay id_base + insertion order, appends work as on one device;
 *   vdb_search / vdb_ivf_search (+ _device, _partial_device; device pointers = memory of devices[0])  run every shard's partial
 *                  search on its own device, stream and host thread, gather the packed partials into devices[0] by peer copies
 *                  over xGMI and merge them there on (float64 key, global id): the result is bit-identical to the
 *                  single-device index of the same rows, whatever ndev;
 *   vdb_ivf_train  runs k-means once (on devices[0], over the whole training set); every shard files its rows under the same
 *                  centroids and probes the same lists;
 *   vdb_reserve, vdb_stats (sums / maxima over the shards, ndevices), vdb_set_option (forwarded), vdb_reset, vdb_destroy,
 *   vdb_ivf_set_centroids / _get_centroids / _set_nprobe / _get_assignment, vdb_rerank(_device)  work as on one device.
 * Not available on such a handle: the table of kinds above (column "multi").
 * Option "multi_stage_all" = 1 (tests) makes shards on devices[0] take the remote-shard path too (own query copy, packed buffer,
 * peer copy), so a one-GPU box exercises the code a multi-GPU node runs.
 * A device may be listed more than once (several shards on one GPU). */
int vdb_create_multi(int dim, int metric, const int *devices, int ndev, vdb_handle *out);
int vdb_destroy(vdb_handle h);

/* replaces index.add(vectors) (exact_search.py:39; modular.py:124-130 keeps the raw matrix):
 * uploads n rows (row-major float32, host memory) and builds the scan copy.  APPENDS, as faiss.Index.add does: row i of
 * the index (in insertion order over all adds) gets id id_base + i; id_base (row-sharded corpora pass their shard offset)
 * belongs to the index -- every add of one index passes the same value (VDB_ERR_INVALID otherwise), vdb_reset empties the
 * index.  An append re-derives the scan copies from the float32 rows on the device (~0.3 s per 12.5M x 768 rows) and
 * needs room for the old and the grown row buffer side by side while it copies.
 * The rows are streamed in blocks (option "upload_block_mb", default 64 MiB) through two pinned staging buffers, so
 * x_host may be a memory-mapped file far larger than host RAM comfortably holds (dataset.py:376-471, 1001-1052). */
int vdb_add(vdb_handle h, const float *x_host, int64_t n, int64_t id_base);
/* same, rows already in device memory of the handle's GPU */
int vdb_add_device(vdb_handle h, const float *x_dev, int64_t n, int64_t id_base, void *stream);

/* replaces index.reset(): drops every row (flat and IVF; an IVF index keeps its centroids).  A search before the next add
 * fails with VDB_ERR_STATE. */
int vdb_reset(vdb_handle h);

/* replaces index.search(queries, k) (exact_search.py:58,78): host buffers, synchronous.
 * D (nq,k) float32, I (nq,k) int64, caller-allocated. */
int vdb_search(vdb_handle h, const float *q_host, int64_t nq, int k, float *D, int64_t *I);
/* device-resident variant: all pointers are device memory on the handle's GPU; work is enqueued on
 * `stream` (a hipStream_t, NULL = default stream) and NOT synchronised. */
int vdb_search_device(vdb_handle h, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                      void *stream);

/* ---- range search -- replaces faiss.IndexFlat.range_search: EVERY row within `radius` of each query, exactly ---------------
 * The result is defined by what vdb_search returns: of the rows vdb_search with k = ntotal would return for query q, those whose
 * returned distance D satisfies
 *   L2: D < radius  (D = (float)key, key = the canonical float64 squared distance)     IP: D > radius  (D = (float)(-key), the raw score)
 * with ids = id_base + row, in ASCENDING ID (FAISS leaves the order open; this one needs no sort and two runs return the same
 * bytes).  A NaN key passes neither comparison and is never returned; a key of +inf is never returned under L2; under IP a score of
 * +inf is returned with D = +inf.  radius: +-inf is legal, NaN is VDB_ERR_INVALID, an L2 radius <= 0 returns nothing.
 * lims (nq + 1 int64): query q owns entries [lims[q], lims[q + 1]) of D (float32) and I (int64), which the handle keeps on the
 * device until the next range search, vdb_add (one that is not refused: see the filter section below), vdb_reset or vdb_set_option;
 * they count in bytes_resident / bytes_workspace and are freed by vdb_reset and vdb_destroy.  vdb_range_results(_device) copies the result of the LAST range search of the handle out.
 * How: a handle with resident fp16 panels in layout "x16" (D <= 128, above 15 360 rows) or p16 (D > 128, above 2048
 * rows) runs an MFMA scan that sets a bit per (query, row) whose scan score lies within the proven bound of the radius -- a superset
 * of the answer; every other handle (32x32 layout, "int8_only", "stream_panels", a non-finite corpus) and every query whose
 * threshold or scales are not finite takes all rows.  Set bits are then re-scored in the canonical arithmetic, filtered, counted
 * and written in bit order.  The batch runs in query slabs whose bitmap fits option "range_bitmap_mb"; every slab synchronises
 * the stream once (its result count sizes the result buffers).
 * VDB_ERR_STATE: an empty index; vdb_range_results(_device) without a result on the handle.  VDB_ERR_INVALID: nq <= 0, a null pointer,
 * a NaN radius.  VDB_ERR_UNSUPPORTED: the kinds of the table above, and any handle while option "graph" is 1.  A failed allocation
 * is VDB_ERR_NOMEM: the handle keeps its rows and loses only the result.
 * vdb_stats after a call: last_path = VDB_PATH_RANGE, last_nq, last_candidates = (query, row) pairs scored exactly,
 * last_fallback_queries = queries for which every row was a candidate, scan_dtype = 0; with option "timing", last_prep_ms = query
 * statistics, bound and threshold, last_scan_ms = the prefilter (several slabs: from the first scan's start to the last one's end),
 * last_tail_ms = exact filter + emit. */
int vdb_range_search(vdb_handle h, const float *q_host, int64_t nq, float radius, int64_t *lims_host);
/* D float32 (lims[nq]), I int64 (lims[nq]), caller-allocated; may be NULL when lims[nq] == 0 */
int vdb_range_results(vdb_handle h, float *D_host, int64_t *I_host);
/* device pointers on the handle's GPU, work on `stream`; the stream is synchronised (once per slab), *total_host = lims[nq] */
int vdb_range_search_device(vdb_handle h, const float *q_dev, int64_t nq, float radius, int64_t *lims_dev, int64_t *total_host, void *stream);
/* enqueued on `stream`, NOT synchronised */
int vdb_range_results_device(vdb_handle h, float *D_dev, int64_t *I_dev, void *stream);

/* ---- filtered k-NN search -- replaces IndexFlat.search(.., params=SearchParameters(sel=IDSelectorBitmap)): the k nearest rows AMONG
 * the rows an allow bitmap admits, exactly ---------------------------------------------------------------------------------------
 * The filter: bit r % 32 of word r / 32 admits row r (rows in insertion order, so its id is id_base + r) -- the bitmap layout of the
 * range search.  nbits must equal ntotal (VDB_ERR_INVALID otherwise); bits at positions >= nbits of the last word are ignored,
 * whatever they hold.  vdb_filter_set reads (nbits + 31) / 32 words.
 * The result is defined by what vdb_search returns: per query, exactly the rows vdb_search with k = ntotal would return, restricted
 * to the admitted rows and cut to the first k -- the same keys, distances, tie order by (key, id), and the same -1 / +-FLT_MAX padding
 * when fewer than k rows are admitted.  An all-ones filter returns vdb_search's bytes, an all-zero filter all padding.
 * The filter is state of the handle: its own copy of the words, masked copies of the scans' accumulator inits (4 bytes per padded row,
 * 8 more on a handle with an int8 copy), the admitted count, and -- when fewer rows are admitted than max(4160, option
 * "filter_sparse_pairs") -- their ascending list (4 bytes each, + 4 per 2048 rows).  It counts in bytes_resident and is freed by
 * vdb_filter_clear, vdb_reset and vdb_destroy.  vdb_add(_device), vdb_reset, vdb_set_option and any call that changes the kind of the
 * handle DROP the filter: vdb_search_filtered then fails with VDB_ERR_STATE and a message naming the missing filter -- it never answers
 * unfiltered.  (A vdb_add(_device) that is refused -- a null pointer with n > 0, a negative n, another id_base, an append to an
 * "int8_only" index, more than 2^31 rows -- changes nothing: it keeps the filter and the last range result, as a refused vdb_ivf_add
 * does; an empty append, n = 0 with the index's id_base, is an add that passed its checks and drops both.)
 * vdb_search and every other call never look at the filter: their results are the same with or without one.
 * An install runs on its stream and synchronises it once (the admitted count comes back); the searches synchronise nothing.  The
 * caller orders an install behind filtered searches still running on other streams.
 * How: every MFMA scan reads an accumulator init of 0.9e38 or more as the marker of a padding row and never selects it,
 * so a filtered search is the unfiltered one run on the masked copies, with the allow bit tested wherever an exact stage decides
 * that a row is valid (candidate groups are 4 or 8 consecutive rows, the exhaustive fallback walks all of them).  A selective filter
 * takes the sparse route instead (last_path = VDB_PATH_FILTER_ROWS): when n_allowed < 2 k + 64 (the select could not find k live
 * bins) or nq * n_allowed < option "filter_sparse_pairs", the listed rows alone are scored, query-blocked, and merged.  Option
 * "force_path" keeps its meaning: 1 the exact kernels, 2 the scan, both masked.
 * VDB_ERR_STATE: an empty index; a search or vdb_filter_count without a filter.  VDB_ERR_INVALID: nq <= 0, k outside [1, 2048], a null
 * pointer, nbits != ntotal.  VDB_ERR_UNSUPPORTED: the kinds of the table above, and any handle while option "graph" is 1.  A failed
 * allocation is VDB_ERR_NOMEM: the handle keeps its rows and loses only the filter.
 * vdb_stats after a filtered search: last_path = VDB_PATH_MFMA_SCAN (the scan and the dense small-corpus path) or
 * VDB_PATH_EXACT_SCAN as for vdb_search, with last_candidates / last_rescan_bins / last_fallback_queries meaning what they do there;
 * VDB_PATH_FILTER_ROWS on the sparse route, where last_candidates = nq * n_allowed. */
int vdb_filter_set(vdb_handle h, const uint32_t *words_host, int64_t nbits);
/* words in device memory of the handle's GPU; the install runs on `stream`, which is synchronised once */
int vdb_filter_set_device(vdb_handle h, const uint32_t *words_dev, int64_t nbits, void *stream);
int vdb_filter_clear(vdb_handle h);
int vdb_filter_count(vdb_handle h, int64_t *n_allowed);          /* rows the installed filter admits */
int vdb_search_filtered(vdb_handle h, const float *q_host, int64_t nq, int k, float *D, int64_t *I);
/* device pointers on the handle's GPU; enqueued on `stream`, NOT synchronised */
int vdb_search_filtered_device(vdb_handle h, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev, void *stream);

/* ---- filtered k-NN search on IVF-Flat indexes -- replaces IndexIVFFlat.search(.., params=SearchParametersIVF(sel=IDSelectorBitmap)):
 * the k nearest rows AMONG the admitted rows of the probed lists, exactly --------------------------------------------------------
 * (The flat filter calls above keep refusing IVF handles: these are entry points of their own.)
 * The filter is the flat one's: bit r % 32 of word r / 32 admits the row whose id is id_base + r -- row numbers in INSERTION order
 * over all vdb_ivf_add / _add_assigned calls, NOT in list order.  nbits must equal ntotal; bits at positions >= nbits of the last
 * word are ignored, whatever they hold; (nbits + 31) / 32 words are read.
 * The result is defined by vdb_ivf_search: per query it covers the same nprobe lists (the coarse search never looks at the filter, as
 * in FAISS) and returns the k rows smallest under (canonical float64 key, id) among the ADMITTED rows of those lists, with
 * vdb_ivf_search's distances, tie order and -1 / +-FLT_MAX padding.  An all-ones filter returns vdb_ivf_search's bytes, an all-zero
 * filter only padding.  vdb_ivf_search and every other call never look at the filter.
 * The filter is state of the handle and counts in bytes_resident:
 *     bytes = 4 * 2 * ceil(ntotal / 64)            the allow words in list order
 *           + 8                                    the admitted count
 *           + 4 * panel_rows                       masked accumulator inits of the list-padded panel space (panel_rows = its rows:
 *                                                  every list padded to whole spans of 256 rows, D > 128: 256 or 1024), if built
 *           + 8 * panel_rows                       ... and of its int8 copy (byte-valued rows, D <= 128)
 * (ivf_filter_bytes, csrc/ivf_filter_plan.hpp).  vdb_filter_clear, vdb_reset and vdb_destroy free it.  Any vdb_ivf_add*, vdb_add,
 * vdb_reset, vdb_set_option, vdb_ivf_set_centroids, vdb_ivf_train and a change of kind DROP it (an add that is refused -- no
 * centroids, a bad pointer, another id_base, a list id out of range -- changes nothing and keeps it; an empty append drops it);
 * vdb_ivf_set_nprobe does not (nothing in it depends on nprobe).  An install that replaces a filter writes into the same buffers.  A filtered search without a filter is VDB_ERR_STATE with a message naming the missing filter: it never
 * answers unfiltered.  An install synchronises its stream once (the admitted count comes back); the searches synchronise nothing.
 * How: the install permutes the bitmap into list order on the device and writes masked copies of the list scans'
 * accumulator inits (the pad marker of DESIGN 4.14); the list scans run unchanged on the copies and the exact stages (candidate
 * refine, flagged-query fallback, exact list scan) test the list-order bit.  The exact list scan answers a batch instead of the
 * list-major scan when min(bins per query, nprobe * n_allowed / nlist) < 4 k (ivf_filter_declines; never for a filter that admits
 * every row); option "force_path" keeps its meaning (1: exact list scan, 2: list-major scan wherever vdb_ivf_search would take it).
 * VDB_ERR_STATE: no centroids / not built / an empty index; a search or vdb_ivf_filter_count without a filter.  VDB_ERR_INVALID:
 * nq <= 0, k outside [1, 2048], a null pointer, nbits != ntotal.  VDB_ERR_UNSUPPORTED: the kinds of the table above, and any handle
 * while option "graph" is 1.  A failed allocation is VDB_ERR_NOMEM: the handle keeps its rows and loses only the filter.
 * vdb_stats after a filtered search: last_path = VDB_PATH_IVF; last_candidates, last_rescan_bins, last_fallback_queries and
 * last_rows_scanned mean what they mean after vdb_ivf_search.  Not served: IVF-SQ8, IVF-PQ, multi-device and sharded (partial) forms. */
int vdb_ivf_filter_set(vdb_handle h, const uint32_t *words_host, int64_t nbits);
/* words in device memory of the handle's GPU; the install runs on `stream`, which is synchronised once */
int vdb_ivf_filter_set_device(vdb_handle h, const uint32_t *words_dev, int64_t nbits, void *stream);
int vdb_ivf_filter_count(vdb_handle h, int64_t *n_allowed);      /* rows the installed filter admits */
int vdb_ivf_search_filtered(vdb_handle h, const float *q_host, int64_t nq, int k, float *D, int64_t *I);
/* device pointers on the handle's GPU; enqueued on `stream`, NOT synchronised */
int vdb_ivf_search_filtered_device(vdb_handle h, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev, void *stream);

/* ---- range search on IVF-Flat indexes -- replaces faiss.IndexIVFFlat.range_search: EVERY row of the probed lists within `radius` of
 * each query, exactly -----------------------------------------------------------------------------------------------------------
 * (vdb_range_search keeps refusing IVF handles: these are entry points of their own.)
 * Per query the result is what vdb_ivf_search returns with the handle's current nprobe and k = all rows of the probed lists -- the same
 * coarse choice, the same canonical float64 keys, the same returned D -- cut to the rows whose D satisfies D < radius (L2) or
 * D > radius (IP); the ids are the rows' own (id_base + insertion row).  A NaN key passes neither comparison; +-inf radii are legal;
 * an L2 radius <= 0 returns nothing (vdb_range_search's rules, word for word).
 * The rows of a query come in ascending LIST-ORDER row: ascending list number, then ascending id inside a list (an add keeps
 * insertion order inside a list).  No sort is involved; two runs return the same bytes, whichever route served them and whatever
 * the slab size.  lims_host: nq + 1 offsets as for vdb_range_search; the result stays on the device, owned by the handle, until the
 * next range search, any add, vdb_ivf_set_centroids, vdb_ivf_train, vdb_reset or vdb_set_option (vdb_ivf_set_nprobe keeps it: it
 * is already materialised); it counts in bytes_resident / bytes_workspace and is freed by vdb_reset and vdb_destroy.
 * vdb_ivf_range_results(_device) copies the result of the LAST range search out.  An installed IVF filter is ignored and left alone.
 * How: per query slab (option "range_bitmap_mb", at most 16384 queries) the coarse search and the fp16 list scan of
 * vdb_ivf_search run unchanged; every kept bin minimum that can stand for a score <= the query's threshold marks its quad, a bin
 * whose kept minima all pass marks all its rows, in a bitmap [query][list-order row]; the marks are re-scored exactly, counted and
 * emitted by the kernels of vdb_range_search.  The exact route marks every probed row instead (no scan): batches the list-major
 * scan declines, and option "force_path" 1 / 3.  Every slab synchronises `stream` once.
 * VDB_ERR_STATE: no centroids / not built / an empty index; vdb_ivf_range_results(_device) without a result.  VDB_ERR_INVALID:
 * nq <= 0, a null pointer, a NaN radius.  VDB_ERR_UNSUPPORTED: the kinds of the table above, and any handle while option "graph" is 1.
 * vdb_stats after a call: last_path = VDB_PATH_IVF_RANGE, last_nq, last_candidates = (query, row) pairs scored exactly,
 * last_fallback_queries = queries for which every probed row was a candidate; with option "timing", last_scan_ms / last_tail_ms per slab.
 * Not served: IVF-SQ8, IVF-PQ and multi-device handles, the int8 list scan, filtered range search, per-query radii. */
int vdb_ivf_range_search(vdb_handle h, const float *q_host, int64_t nq, float radius, int64_t *lims_host);
int vdb_ivf_range_results(vdb_handle h, float *D_host, int64_t *I_host);
/* device pointers on the handle's GPU; lims_dev: nq + 1 int64; *total_host = lims[nq]; `stream` is synchronised once per slab */
int vdb_ivf_range_search_device(vdb_handle h, const float *q_dev, int64_t nq, float radius, int64_t *lims_dev, int64_t *total_host, void *stream);
int vdb_ivf_range_results_device(vdb_handle h, float *D_dev, int64_t *I_dev, void *stream);

/* ---- row-sharded search (one process per GPU; partials exchanged with an RCCL all-gather) ---- */
/* per-shard partial top-k: float64 order keys (L2: squared distance, IP: -score) and global ids,
 * sorted ascending by (key,id); missing entries have id -1 / key +inf. */
int vdb_search_partial_device(vdb_handle h, const float *q_dev, int64_t nq, int k, double *keys_dev,
                              int64_t *ids_dev, void *stream);
/* merge nparts partial lists laid out (nparts, nq, k) into the final (nq,k) result. */
int vdb_merge_partials_device(int metric, int device, const double *keys_dev, const int64_t *ids_dev, int nparts,
                              int64_t nq, int k, float *D_dev, int64_t *I_dev, void *stream);

/* same merge for ONE packed buffer per part -- what a single RCCL all-gather produces when every rank sends
 * its keys (nq*k doubles) immediately followed by its ids (nq*k int64): layout (nparts, 2, nq, k) 8-byte words. */
int vdb_merge_packed_partials_device(int metric, int device, const void *packed_dev, int nparts, int64_t nq, int k,
                                     float *D_dev, int64_t *I_dev, void *stream);

/* ---- candidate re-scoring -- replaces the per-query NumPy loop of FaissSearcher._batch_search_lsh_rerank
 *      (modular.py:483-532: gather candidate rows by id -> exact L2 / inner product -> top-k) and
 *      LSHSearcher._compute_distances (lsh.py:242-250) ------------------------------------------------ */
/* cand (nq, ncand) int64 row ids (id_base-relative ids as returned by search; -1 = empty slot, ids of one
 * query must be distinct).  Output: the k best candidates of every query, flat conventions and padding.
 * A handle whose rows were filed by vdb_ivf_add(_assigned) (any IVF kind, one device or vdb_create_multi) is refused with
 * VDB_ERR_STATE before any kernel runs: its rows sit in list order (SQ8 and IVF-PQ keep no float32 rows at all), not in id order. */
int vdb_rerank(vdb_handle h, const float *q_host, int64_t nq, const int64_t *cand_host, int ncand, int k, float *D,
               int64_t *I);
int vdb_rerank_device(vdb_handle h, const float *q_dev, int64_t nq, const int64_t *cand_dev, int ncand, int k,
                      float *D_dev, int64_t *I_dev, void *stream);

/* ---- IVF-Flat -- replaces faiss.index_factory(d, "IVF<nlist>,Flat", metric) + train/add/search
 *      (modular.py:277-286, 437-441, 544; approximate_search.py:39-51, 87) ------------------- */
/* k-means (Lloyd) on at most max_points_per_centroid*nlist rows sampled with `seed`; niter iterations.  The result is fixed bit
 * for bit by the arguments (restated in NumPy by tests/kmeans_restatement.py); max_points_per_centroid <= 0 means 256:
 *   sample   ns = min(n, max_points_per_centroid * nlist);  pick = 0 .. n-1;  rng = std::mt19937_64(seed);  for i = 0 ..
 *            min(ns, n - 1) - 1:  j = i + rng() % (n - i), swap pick[i] and pick[j].  The sample is the rows pick[0 .. ns) in that
 *            order (ns == n: still a permutation of the rows, not the identity)
 *   init     the centroids are the first nlist sample rows; niter == 0 returns them
 *   assign   every sample row goes to its nearest centroid under the index metric: the canonical float64 key (above), ties to
 *            the smaller list; inside a list the rows stay in sample order
 *   update   non-empty list c, every d:  acc = 0.0;  acc += (double)x[d] over the rows of the list in order, one rounding per
 *            add;  centroid[c][d] = (float)(acc / (double)count).  An empty list keeps its centroid
 *   IP only  ("spherical")  n2 = sum over the 64-dimension blocks, in ascending order, of the block's sum of
 *            (double)centroid[c][d] * (double)centroid[c][d] (0 for d >= dim), the 64 values of a block added as the butterfly
 *            v[i] += v[i ^ w], w = 32, 16, .., 1;  n2 > 0:  centroid[c][d] *= (float)(1.0 / sqrt(n2)), a float32 product
 *   split    after the update, on the list sizes cnt of this assignment, for l ascending with cnt[l] == 0:  big = the first
 *            list holding the largest cnt;  for every d, c = centroid[big][d], e = +1/1024 (odd d) or -1/1024 (even d):
 *            centroid[l][d] = c * (1.f + e), centroid[big][d] = c * (1.f - e), float32;  cnt[l] = cnt[big] / 2,
 *            cnt[big] -= cnt[l] (the next empty list sees these counts).  Split centroids are not normalised again
 * The centroids after the last iteration are installed; rows filed under earlier centroids are dropped at the next add. */
int vdb_ivf_train(vdb_handle h, int nlist, const float *x_host, int64_t n, int niter, uint64_t seed,
                  int max_points_per_centroid);
/* inject centroids (nlist, dim) instead of training -- used by parity tests and index loading */
int vdb_ivf_set_centroids(vdb_handle h, const float *centroids_host, int nlist);
int vdb_ivf_get_centroids(vdb_handle h, float *centroids_host);
/* assign rows to their nearest centroid and build the inverted lists (CSR, vectors grouped by list).  APPENDS like vdb_add
 * (same id rule); the lists are the ones a single add of all rows builds (rows of a list stay in insertion order). */
int vdb_ivf_add(vdb_handle h, const float *x_host, int64_t n, int64_t id_base);
/* same with the list of every row given (int32 (n), as vdb_ivf_get_assignment returned it for this corpus and these
 * centroids): what loading a persisted index does -- no coarse assignment pass (covertree_v2_2.py:184-282 is the
 * reference's load protocol).  A row whose list id is out of range is an error. */
int vdb_ivf_add_assigned(vdb_handle h, const float *x_host, int64_t n, int64_t id_base, const int32_t *list_of_row_host);
int vdb_ivf_set_nprobe(vdb_handle h, int nprobe);
/* list id of each indexed row, int32 (n) -- parity tests compare it with the oracle's assignment */
int vdb_ivf_get_assignment(vdb_handle h, int32_t *list_of_row_host);
int vdb_ivf_search(vdb_handle h, const float *q_host, int64_t nq, int k, float *D, int64_t *I);
int vdb_ivf_search_device(vdb_handle h, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                          void *stream);
/* row-sharded IVF (coarse quantizer replicated, the rows of every list split over the ranks): per-shard
 * partial top-k among the probed lists, same layout and merge as vdb_search_partial_device */
int vdb_ivf_search_partial_device(vdb_handle h, const float *q_dev, int64_t nq, int k, double *keys_dev,
                                  int64_t *ids_dev, void *stream);

/* ---- IVF<nlist>,SQ8 -- replaces faiss.index_factory(d, "IVF<nlist>,SQ8", metric) (IndexIVFScalarQuantizer, QT_8bit,
 *      RS_minmax, by_residual; the reference's `ivf_sq8` config) ------------------------------------------------------
 * One byte per dimension: the index keeps the codes, the ids and a list id per row, and NO float32 rows and no fp16 / int8
 * scan copies.  Every step is float32, rounded as written (c_l = centroid of the row's list):
 *   train   r = x - c_l over the training rows (all of them when n <= 100 000, else the rows floor(i * n / 100 000));
 *           vmin[d] = min r[d];  vdiff[d] = max r[d] - vmin[d]
 *   encode  u = vdiff[d] != 0 ? (r[d] - vmin[d]) / vdiff[d] : 0;  u = clamp(u, 0, 1);  code = (uint8) trunc(255 * u)
 *   decode  x^[d] = c_l[d] + (vmin[d] + ((code + 0.5f) / 255.0f) * vdiff[d])
 * A search returns, bit for bit, the IVF-Flat result over the float32 rows x^ under the same lists (canonical float64
 * arithmetic above): every exact kernel (list scan, refine, flagged-query scan) decodes x^ from the codes.  D <= 128: batches
 * the list-major path serves take the MFMA list scan on fp16 panels converted from the codes per batch (workspace; they equal
 * IVF-Flat's panels of x^, so the same error bound holds; vdb_stats.scan_dtype = 2).  D > 128: the exact list scan.
 * Rows enter through vdb_ivf_add / vdb_ivf_add_assigned only.  What an SQ8 handle admits and which options it refuses: the
 * table of kinds above (column "IVF-SQ8"). */
/* codec of the inverted lists: 0 = Flat (the default), 1 = SQ8, 2 = PQ (IVF<nlist>,PQ<M>, below), 3 = I8 (IVF<nlist>,I8, below; dim
 * <= 128, VDB_ERR_UNSUPPORTED beyond).  Only before centroids or rows exist (VDB_ERR_STATE after) */
int vdb_ivf_set_codec(vdb_handle h, int codec);
/* SQ8: vdb_ivf_train trains the centroids (the contract stated there, unchanged by the codec) and then the ranges on the same
 * rows, all of them and not the k-means sample; this call trains the ranges only, against
 * the installed centroids (vdb_ivf_set_centroids).  New ranges drop the rows encoded under the old ones at the next add. */
int vdb_ivf_sq8_train_ranges(vdb_handle h, const float *x_host, int64_t n);
/* inject / read the ranges, float32 (dim) each -- persistence and tests */
int vdb_ivf_sq8_set_ranges(vdb_handle h, const float *vmin_host, const float *vdiff_host);
int vdb_ivf_sq8_get_ranges(vdb_handle h, float *vmin_host, float *vdiff_host);
/* codes of an SQ8 index, uint8 (ntotal, dim), in id (insertion) order */
int vdb_ivf_get_codes(vdb_handle h, uint8_t *codes_host);

/* ---- IVF<nlist>,I8 -- IVF-Flat over a byte-valued corpus that keeps the rows ONCE, as int8 (codec 3 of vdb_ivf_set_codec) ----------
 * A byte-valued corpus (SIFT, BIGANN, any uint8 / int8 feature set: every value an integer in 0..255, or every value an integer in
 * -128..127 -- the test the flat int8 copies are admitted by) sits four times in an IVF-Flat index: float32 rows, fp16 panels, int8
 * panels, row-major int8 rows.  An IVF-I8 index keeps the last two and what is derived from them -- rows8 in list order, panels8,
 * bias8, rowstat8, the fp16 scan's bias, ids, CSR and span tables, centroids -- about 0.6 x the float32 bytes (csrc/ivf_i8_plan.hpp,
 * ivf_i8_bytes), and NO float32 rows and no resident fp16 panels.  The codec is LOSSLESS: a row is stored as byte = x - cx with cx =
 * 128 (values 0..255; chosen when both windows fit) or 0 (values -128..127) and decoded as x = byte + cx, exactly.
 * vdb_ivf_search, _device, _partial_device and vdb_reserve return, bit for bit, what an IVF-Flat handle returns with the same
 * centroids, rows, id_base, nprobe and k.  Integer batches inside the byte window take the int8 list scan on the resident panels and
 * the integer refine, as on IVF-Flat (scan_dtype = 1); every other batch of the list-major path scans fp16 panels converted from the
 * int8 panels for that batch (scan_dtype = 2; they equal IVF-Flat's panels, so the same candidates are nominated; option
 * "ivf_i8_scratch" = 0 skips them); every exact stage scores x = byte + cx in the canonical float64 arithmetic.
 * Rows enter through vdb_ivf_add / vdb_ivf_add_assigned only, in blocks of option "int8_block_rows": the corpus is never held in
 * float32 on the device.  An add of rows that are not byte-valued, or that fit no window together with the rows already filed, is
 * VDB_ERR_INVALID and leaves the handle exactly as it was.  Appends work as on IVF-Flat: any sequence of adds builds, byte for byte,
 * the index one add of all rows builds (the window is re-chosen over old and new rows).  vdb_ivf_train / vdb_ivf_set_centroids work
 * as on IVF-Flat (float32 centroids, unchanged coarse stage).  vdb_stats.has_i8_copy = 2.  What the kind admits and which options
 * it refuses: the table of kinds above (column "IVF-I8"); not served: multi-device handles, filtered and range search, D > 128. */
/* int8 (ntotal, dim) rows in id (insertion) order and the offset: x = rows + *cx.  rows_host may be NULL (only *cx is returned) */
int vdb_ivf_i8_get_rows(vdb_handle h, int8_t *rows_host, int *cx);

/* ---- IVF<nlist>,PQ<M> -- replaces faiss.index_factory(d, "IVF<nlist>,PQ<M>", metric) (IndexIVFPQ, 8 bits, by_residual; the
 *      reference's `ivf_pq` configs) -- codec 2 of vdb_ivf_set_codec ---------------------------------------------------------
 * M bytes per row: the index keeps the codes in list order, a list id and an id per row, the centroids, the codebooks and
 * (dim <= 128) the panel-space bias -- NO float32 rows and no fp16 / int8 scan copies.  The contract is the library's own, as
 * for SQ8 and flat PQ (FAISS' k-means, its float32 table sums and its tie order are not reproduced).  Every step is float32,
 * rounded as written; c_l = centroid of the row's list, dsub = dim / M:
 *   train   codebooks float32 [M][256][dsub], trained on the residuals r = x - c_l of ONE row sample (at most
 *           256 * max_points_per_centroid rows, drawn with `seed` as the flat PQ training draws them) against the installed
 *           centroids; sub-space m is clustered by the k-means of vdb_ivf_train with seed + m.  Same seed, same codebooks:
 *           bit for bit the contract stated at vdb_ivf_train (L2, nlist = 256, run on the sample's columns, which that run
 *           permutes again with its own seed; l of a sample row = its list under the index metric).
 *           Fewer than 256 rows: VDB_ERR_INVALID.  vdb_ivf_train keeps training the centroids only
 *   encode  code[i][m] = argmin over c of the canonical float64 L2 key between r[i][m dsub .. (m + 1) dsub) and
 *           codebook[m][c]; ties to the smaller c, whatever the index metric
 *   decode  x^[d] = c_l[d] + codebook[m][code[m]][j]: one float32 add (a padding dimension decodes to exactly 0)
 *   search  vdb_ivf_search / _device / _partial_device and vdb_reserve return, bit for bit, the IVF-Flat result over the
 *           float32 rows x^ under the same lists and nprobe (ids, distances, ties by id)
 * dim <= 128: batches the list-major path serves make the fp16 panels of the whole panel space from the codes per batch, as
 * (half)((c_l[d] + codebook entry) * sx) -- IVF-Flat's panels of x^, so the same error bound holds (vdb_stats.scan_dtype = 2) --
 * and run the MFMA list scan on them; dim > 128, small batches and "force_path" 1 / 3 take the exact list scan over the codes.
 * A third path, off by default: with option "ivfpq_adc_max_batch" = B a batch of at most B queries (any dim; k <= 1024, M <= 159,
 * "force_path" 0, at most 256 MiB of scores = 4 nq min(ntotal, nprobe x longest list) bytes) scores the rows of its probed lists
 * from ONE float32 lookup table per query, a scalar per (query, probe) and a resident float32 ||x^||^2 per row, re-scores the rows
 * within twice the derived bound of the k-th smallest score exactly and returns the same ids and distances, bit for bit
 * (vdb_stats.last_path = VDB_PATH_IVFPQ_ADC, scan_dtype = 3; DESIGN 4.4 "IVF-PQ ADC scan").  The norms cost 4 ntotal bytes of
 * bytes_resident, allocated by the first admitted batch after an add -- a handle that never sets the option never holds them.
 * vdb_ivf_add / vdb_ivf_add_assigned encode and append.  New codebooks (or centroids) drop the rows encoded under the old ones
 * at the next add; vdb_reset drops the rows and keeps centroids and codebooks.
 * VDB_ERR_STATE: an add before codebooks.  dim % M != 0 or M outside 1 .. min(dim, 256): VDB_ERR_INVALID.  Which handles these
 * calls admit, and what an IVF-PQ handle refuses (with a message that names IVF-PQ): the table of kinds above. */
int vdb_ivfpq_train(vdb_handle h, int M, const float *x_host, int64_t n, int niter, uint64_t seed, int max_points_per_centroid);
/* inject / read the codebooks, float32 (M, 256, dim / M) -- persistence and tests.  codebooks_host may be NULL: M only (0 = none) */
int vdb_ivfpq_set_codebooks(vdb_handle h, int M, const float *codebooks_host);
int vdb_ivfpq_get_codebooks(vdb_handle h, int *M, float *codebooks_host);
/* APPEND n rows given as codes, uint8 (n, M), with the list of every row (int32, as vdb_ivf_get_assignment returned it) -- what
 * loading a persisted index does; ids and id_base as vdb_ivf_add */
int vdb_ivfpq_add_codes(vdb_handle h, const uint8_t *codes_host, int64_t n, int64_t id_base, const int32_t *list_of_row_host);
/* codes of the indexed rows, uint8 (ntotal, M), in id (insertion) order */
int vdb_ivfpq_get_codes(vdb_handle h, uint8_t *codes_host);

/* ---- sign-LSH codes + Hamming candidate scan + exact re-rank -- replaces faiss.IndexLSH(d, nbits) with its defaults as
 *      FaissLSHIndexer / the LSH branch of FaissSearcher use it (modular.py:182-221, 455-548; the reference's `faiss_lsh`
 *      config): query -> code -> Hamming top-ncand -> exact top-k, all on the device ------------------------------------------
 * The entry points live on an ordinary flat handle of vdb_create: the index keeps its float32 rows and scan copies, and
 * next to them one bit per projection row.  The contract is the library's own, exact and deterministic (FAISS' random
 * matrix and its order among equal Hamming distances are not reproduced):
 *   projection  R, float32 (nbits, dim) row-major, given by the caller (the library draws no random numbers); nbits a
 *               multiple of 32 in [32, 1024]
 *   bits        s_j(x) = sum_d (double)x[d] * (double)R[j][d], accumulated from 0.0 with d ascending, one rounding per step;
 *               bit j = (s_j >= 0): -0.0 and 0.0 give 1, NaN gives 0.  (The product of two float32 values is exact in
 *               float64, so an fma chain and a multiply-then-add chain give the same bits.)  Rows and queries alike; cosine is
 *               the caller's normalisation, as everywhere in this ABI
 *   codes       nbits / 32 little-endian uint32 words per row; bit j is bit j % 32 of word j / 32
 *   candidates  per query the min(ncand, ntotal) rows smallest under (Hamming distance, id), both ascending, returned in
 *               that order: ids int64 (with id_base), distances int32; missing slots are id -1, distance INT32_MAX
 *   search      exactly vdb_rerank applied to those candidates (the k best in canonical float64 arithmetic under (key, id),
 *               flat conventions and padding): bit for bit what "candidates, then vdb_rerank" returns
 * The select counts instead of sorting (distances are integers in [0, nbits]): a histogram of a row sample bounds the cut
 * distance from above; one xor + popcount scan counts the pairs below that bound per distance -- which fixes the cut t and the
 * number m of rows up to it -- and appends them to the query's list (the next power of two >= min(4 ncand + 1024, ntotal)
 * entries); the entries up to t are sorted by (distance, id).  A query whose list overflowed under the bound is scanned a second
 * time with its exact t.  A query whose bound was too small, or whose m rows (ties at t included) exceed the list, takes an
 * exact fallback (full histogram of its distances, then an ordered pass); vdb_stats.last_fallback_queries counts them, option
 * "lsh_force_fallback" = 1 sends every query there.  vdb_stats.last_path = VDB_PATH_LSH; with option "timing",
 * last_prep_ms = query codes + sample, last_scan_ms = the scans, last_tail_ms = select + re-rank.
 * ncand is in [1, 65 536] (VDB_ERR_INVALID above; ncand > ntotal is legal and pads); k follows vdb_rerank (1 .. 2048; k >
 * ncand pads).  VDB_ERR_STATE: an LSH call before a projection, or before rows.  Which handles admit the LSH calls, what a handle
 * with a projection refuses, and the options (no resident float32 rows to encode from or re-rank against): the table of kinds above.
 * A handle without a projection behaves exactly as before. */
/* installs R.  With rows already present they are encoded from the resident float32 rows; with none R is only stored.
 * Every later vdb_add / vdb_add_device encodes the rows it appends (appended codes equal those of one big add).  vdb_reset
 * drops the codes and keeps R; vdb_destroy frees both; codes and R count in bytes_resident. */
int vdb_lsh_set_projection(vdb_handle h, int nbits, const float *proj_host);
/* proj_host may be NULL: nbits only (0 = no projection) */
int vdb_lsh_get_projection(vdb_handle h, int *nbits, float *proj_host);
/* codes of the indexed rows, uint32 (ntotal, nbits / 32), in id (insertion) order */
int vdb_lsh_get_codes(vdb_handle h, uint32_t *codes_host);
/* ham (nq, ncand) int32, ids (nq, ncand) int64, caller-allocated; host buffers, synchronous */
int vdb_lsh_candidates(vdb_handle h, const float *q_host, int64_t nq, int ncand, int32_t *ham, int64_t *ids);
/* device pointers on the handle's GPU; enqueued on `stream`, NOT synchronised */
int vdb_lsh_candidates_device(vdb_handle h, const float *q_dev, int64_t nq, int ncand, int32_t *ham_dev, int64_t *ids_dev,
                              void *stream);
/* D (nq, k) float32, I (nq, k) int64 */
int vdb_lsh_search(vdb_handle h, const float *q_host, int64_t nq, int k, int ncand, float *D, int64_t *I);
int vdb_lsh_search_device(vdb_handle h, const float *q_dev, int64_t nq, int k, int ncand, float *D_dev, int64_t *I_dev,
                          void *stream);

/* ---- hash-table LSH -- replaces the reference's own LSHIndexer / LSHSearcher / LSH (src/algorithms/lsh.py; its `lsh` config):
 *      T tables of H random projections, votes over the colliding buckets, a candidate cap, exact scoring ------------------------
 * The entry points live on an ordinary flat handle of vdb_create: the index keeps its float32 rows and scan copies, and next to
 * them T table keys per row.  The contract follows lsh.py step by step, so that its results are reproduced id for id
 * (tests/lsh_tables_restatement.py restates it in NumPy):
 *   parameters  T = num_tables in 1..32; H = hash_size; mode 0 "sign" (the reference's cosine branch): H in 1..64; mode 1 "E2"
 *               (its L2 branch): H in 1..16, bucket_width w > 0 (float32), offsets b float32 (T, H).  W = words per table key:
 *               ceil(H / 32) in sign mode, H in E2 mode; T W <= 128.  Projections P float32 (T, H, dim) come from the caller
 *               (the library draws no random numbers)
 *   projection  s[t][h](x) = sum_d (double)x[d] * (double)P[t][h][d], accumulated from 0.0 with d ascending, one rounding per
 *               step: the arithmetic of the sign-LSH bits above
 *   key words   uint32, T W per vector, table t at words [t W, (t + 1) W).  sign: bit h of table t is bit h % 32 of word
 *               t W + h / 32, set iff s >= 0 (-0.0 gives 1, NaN gives 0), unused bits 0.  E2: word t W + h = the int32 code
 *               floor((s + (double)b[t][h]) / (double)w), bit-cast, saturated to [INT32_MIN, INT32_MAX], NaN -> INT32_MIN
 *   votes       row r collides with query q in table t iff all W words of that table are equal; votes(q, r) = the number of
 *               such tables, first(q, r) = the smallest such t
 *   candidates  of q: the rows with votes >= 1, ordered by ((T - votes) T + first, id), both ascending, the first
 *               min(ncand, their number) of them -- Counter.most_common() over buckets that hold ids in insertion order.  ids
 *               int64 (with id_base), votes int32; padding is id -1, votes 0
 *   search      exactly vdb_rerank applied to those candidates.  fallback = 1: a query with no colliding row gets the exact
 *               flat top-k of the handle instead (the reference's list(range(n)), which is not capped); fallback = 0: such a
 *               query is all padding
 * The select is the counting select of the sign-LSH calls over T * T classes, without the pairs that have no vote; per query
 * c = min(ncand, colliding rows).  vdb_stats after a call: last_path = VDB_PATH_LSHT, last_candidates = candidates re-scored,
 * last_fallback_queries = queries that took the exact fallback of the select (option "lsh_force_fallback" = 1: all of them),
 * last_rows_scanned = ntotal x queries that took the brute-force fallback; with option "timing", last_prep_ms = query keys +
 * sample, last_scan_ms = the vote scans, last_tail_ms = select + re-rank.
 * ncand is in [1, 65 536] (ncand > ntotal pads); k follows vdb_rerank.  VDB_ERR_STATE: a call before tables, or before rows.
 * VDB_ERR_INVALID: a parameter outside the ranges above.  Which handles admit these calls and what a handle with tables refuses:
 * the table of kinds above (column "LSHT").  A handle without tables behaves exactly as before. */
/* installs the tables: proj_host (T, H, dim), offsets_host (T, H) and bucket_width (mode 1 only; ignored in mode 0).  With rows
 * present they are keyed from the resident float32 rows.  Every later vdb_add / vdb_add_device keys the rows it appends (appended
 * keys equal those of one add).  vdb_reset drops the keys and keeps the tables; keys and tables count in bytes_resident. */
int vdb_lsht_set_tables(vdb_handle h, int num_tables, int hash_size, int mode, const float *proj_host, const float *offsets_host,
                        float bucket_width);
/* num_tables = 0: no tables.  Every pointer but num_tables may be NULL */
int vdb_lsht_get_tables(vdb_handle h, int *num_tables, int *hash_size, int *mode, float *proj_host, float *offsets_host,
                        float *bucket_width);
/* keys of the indexed rows, uint32 (ntotal, T W), in id (insertion) order */
int vdb_lsht_get_keys(vdb_handle h, uint32_t *keys_host);
/* votes (nq, ncand) int32, ids (nq, ncand) int64, caller-allocated; host buffers, synchronous */
int vdb_lsht_candidates(vdb_handle h, const float *q_host, int64_t nq, int ncand, int32_t *votes, int64_t *ids);
/* device pointers on the handle's GPU; enqueued on `stream`, NOT synchronised */
int vdb_lsht_candidates_device(vdb_handle h, const float *q_dev, int64_t nq, int ncand, int32_t *votes_dev, int64_t *ids_dev,
                               void *stream);
/* D (nq, k) float32, I (nq, k) int64 */
int vdb_lsht_search(vdb_handle h, const float *q_host, int64_t nq, int k, int ncand, int fallback, float *D, int64_t *I);
int vdb_lsht_search_device(vdb_handle h, const float *q_dev, int64_t nq, int k, int ncand, int fallback, float *D_dev,
                           int64_t *I_dev, void *stream);

/* ---- flat PQ<M> -- replaces faiss.index_factory(d, "PQ<M>", metric) (IndexPQ(d, M, 8); the reference's `pq` config) --------
 * M sub-vectors of dsub = dim / M dimensions, 256 centroids each, one byte per sub-vector.  The entry points live on an ordinary
 * handle of vdb_create; once codebooks exist the handle is a PQ index: it keeps the codes (M bytes per row), one float32 of scan
 * statistics per padded row and the codebooks -- NO float32 rows, no fp16 / int8 scan copies.  The contract is the library's own
 * (FAISS' k-means, its float32 table sums and its tie order are not reproduced):
 *   codebooks  float32 [M][256][dsub].  vdb_pq_train: one row sample (at most 256 * max_points_per_centroid rows, drawn with
 *              `seed`) shared by all sub-spaces; sub-space m is clustered by the k-means of vdb_ivf_train (L2, 256 centroids,
 *              niter iterations) with seed + m.  Same seed, same codebooks: bit for bit the contract stated at vdb_ivf_train,
 *              run on the sample's columns [m dsub, (m + 1) dsub) with nlist = 256 and the same max_points_per_centroid (that
 *              run permutes the sample again with its own seed).  Fewer than 256 training rows: VDB_ERR_INVALID
 *   codes      code[i][m] = argmin over c of the canonical float64 L2 key (above) between x[i][m dsub .. (m + 1) dsub) and
 *              codebook[m][c]; ties to the smaller c, whatever the index metric
 *   x^         x^[i] = concatenation of codebook[m][code[i][m]]: a lookup, no arithmetic
 *   search     vdb_search / _device / _partial_device, vdb_rerank(_device), vdb_reserve, vdb_stats return, bit for bit, what a
 *              flat index over the float32 rows x^ returns (ids, distances, ties by id; cosine is the caller's normalisation)
 * Small corpora and batches below option "pq_scan_min_batch" take the exact kernels, which look x^ up from the codes; otherwise
 * every search makes the fp16 panels of the scan from the codes, slab by slab ("pq_slab_chunks" scan chunks per slab; default
 * the chunks of 524 288 rows, whatever ntotal), as (half)(codebook * sx) -- the rounding a flat build applies to x^ -- so the
 * scan statistics and the error bound are those of the flat index over x^ (vdb_stats.scan_dtype = 2).
 * A third path, off by default: with option "pq_adc_max_batch" = B a batch of at most B queries that the scan would serve (256-row
 * bins, k <= 1024, M <= 159: one float32 table of M x 256 partial scores per query must fit a workgroup's LDS) is scanned
 * straight from the codes -- score = cs bias + sum over m of T[m][code[m]], plain float32 adds, m ascending -- with its own error
 * bound (DESIGN 4.9 "ADC scan"); nothing is decoded and no slab of panels is allocated.  The bin select, the exact refine and the
 * fallback pass are those of the MFMA scan, so the results stay, bit for bit, the flat exact search over x^
 * (vdb_stats.last_path = VDB_PATH_PQ_ADC, scan_dtype = 3).
 * VDB_ERR_STATE: codebooks (train / set) while the handle holds rows; add / get_codes before codebooks.  Which handles admit the
 * PQ calls, and the calls and options a PQ handle refuses (its panels are made in layout "x16" only): the table of kinds above.
 * dim % M != 0 or M outside 1 .. min(dim, 256): VDB_ERR_INVALID.  vdb_reset drops the codes and keeps the codebooks. */
int vdb_pq_train(vdb_handle h, int M, const float *x_host, int64_t n, int niter, uint64_t seed, int max_points_per_centroid);
/* inject / read the codebooks, float32 (M, 256, dim / M) -- persistence and tests.  codebooks_host may be NULL: M only (0 = none) */
int vdb_pq_set_codebooks(vdb_handle h, int M, const float *codebooks_host);
int vdb_pq_get_codebooks(vdb_handle h, int *M, float *codebooks_host);
/* encode n rows (row-major float32, host memory) and APPEND their codes; ids and id_base as vdb_add */
int vdb_pq_add(vdb_handle h, const float *x_host, int64_t n, int64_t id_base);
/* same with the codes given, uint8 (n, M) -- what loading a persisted index does */
int vdb_pq_add_codes(vdb_handle h, const uint8_t *codes_host, int64_t n, int64_t id_base);
/* codes of the indexed rows, uint8 (ntotal, M), in id (insertion) order */
int vdb_pq_get_codes(vdb_handle h, uint8_t *codes_host);

/* ---- k-NN graph ("knng"; "graph" already names hipGraph replay in this ABI) -- the slot the reference fills with HNSW
 *      (HNSWIndexer + FaissSearcher and the stand-alone HNSW class of its benchmark configs): an exact k-NN graph of the corpus,
 *      pruned by the HNSW neighbour heuristic, searched by a beam search ----------------------------------------------------------
 * The entry points live on an ordinary flat handle of vdb_create that holds float32 rows; the graph is ntotal x degree int32 next
 * to them (it counts in bytes_resident).  The contract is the library's own, deterministic (FAISS' level draw, its float32
 * distances and its tie order are not reproduced; tests/knng_restatement.py restates it in NumPy):
 *   key(u, v)   the canonical float64 order key above (L2 or IP by the index metric), row u's float32 values as the query, row v as
 *               the row.  Every order is by (key, local row number), ascending
 *   candidates  of row i: the first ncand entries of the sorted list of all rows j != i (fewer when ntotal - 1 < ncand)
 *   neighbours  of row i: walk the candidates in order with an empty selected list S; candidate e is selected if |S| < degree and no
 *               s in S has key(e, s) < key(i, e) (strict: a tie accepts), else rejected.  The stored row is S, then the rejected
 *               candidates in candidate order until degree entries exist, then -1.  ncand == degree: the plain k-NN graph, reordered
 *   search      k <= ef <= 512.  L: at most ef entries (key, id, expanded), ordered by (key, id).  Init: score the distinct rows
 *               floor(j ntotal / nentry), j < min(nentry, ef, ntotal), and insert them.  Step: take the first unexpanded entry of L
 *               (none: stop), mark it expanded, score every neighbour of it that is not in L now, L <- best ef of (L u scored).
 *               Stop also after max_iters steps.  Result: the first k of L, flat conventions (id_base added, -1 / +-FLT_MAX padding,
 *               distances = the float32 rounding of the key)
 * A row scored earlier that is not in L now was rejected or evicted against a last key that has only decreased since: scoring it
 * again rejects it again.  So the kernel's per-query "seen" filter is a cache (whole ids, a collision forgets; option
 * "knng_visited_bits" never changes a result), and only the de-duplication against L is exact.
 * vdb_add, vdb_add_device and vdb_reset drop the graph: vdb_knng_get then reports degree 0 and a search returns VDB_ERR_STATE.  The
 * flat search of the handle is untouched.  VDB_ERR_UNSUPPORTED, with a message naming the k-NN graph: the handles and options of
 * the table of kinds above; a dimension whose padded query does not fit a workgroup's LDS (above roughly 14 000).  VDB_ERR_INVALID: k < 1, k > ef, ef > 512, a degree or
 * ncand out of range.  vdb_stats after a search: last_path = VDB_PATH_KNNG, last_candidates = rows scored (summed over the
 * queries), last_fallback_queries = queries the step cap stopped with an unexpanded entry left; with option "timing" the three stages
 * run as three launches: last_prep_ms = entry scoring, last_scan_ms = the traversal, last_tail_ms = writing the results. */
/* builds the graph of the rows present: degree in 4..64, ncand in degree..128, ntotal below 2^31.  Blocks of "knng_build_block" rows go
 * through the partial device search as queries (k = min(ncand + 1, ntotal)); the row itself is stripped, the rest pruned */
int vdb_knng_build(vdb_handle h, int degree, int ncand);
/* injects a graph: nbrs_host (ntotal, degree) local row numbers, degree in 1..64, -1 only as a row's tail.  Checked on the host:
 * VDB_ERR_INVALID for an entry out of range, a self loop, a duplicate within a row, an entry after a -1 */
int vdb_knng_set(vdb_handle h, int degree, const int32_t *nbrs_host);
/* nbrs_host may be NULL: degree only (0 = no graph) */
int vdb_knng_get(vdb_handle h, int *degree, int32_t *nbrs_host);
/* host buffers, synchronous: D (nq, k) float32, I (nq, k) int64 */
int vdb_knng_search(vdb_handle h, const float *q_host, int64_t nq, int k, int ef, float *D, int64_t *I);
/* device pointers on the handle's GPU; enqueued on `stream`, NOT synchronised (the first search, and one whose (ntotal, knng_nentry, ef)
 * give another list of entry rows, waits for `stream` once and uploads that list) */
int vdb_knng_search_device(vdb_handle h, const float *q_dev, int64_t nq, int k, int ef, float *D_dev, int64_t *I_dev, void *stream);

/* Sizes the search workspace for batches of up to nq queries and top-k NOW instead of inside the first search (works on
 * flat and IVF handles after add): one untimed search whose queries are corpus rows.  The reference times its very first
 * batch_search, allocations included (experiment_runner.py:431-437; metrics_methodology.md:119-121: no warm-up) -- the
 * plugins call this from build_index (`reserve_queries`, default 10 000), as FAISS' GPU resources reserve their scratch
 * memory at construction. */
int vdb_reserve(vdb_handle h, int64_t nq, int k);

/* ---- introspection / tuning ---------------------------------------------------------------- */
int vdb_stats(vdb_handle h, vdb_stats_t *out);
/* Options (vdb_set_option; every setting returns exact results unless it says otherwise).  A value outside what is listed is
 * VDB_ERR_INVALID, an unknown name too; an option given as a list of values takes exactly those, one given as a range takes every
 * number in it (truncated toward zero).  Every option named here is a row of kOptions (csrc/vdbhip.hip) and the other way round:
 *   behaviour
 *     "force_path"      0 auto | 1 exact kernels only | 2 MFMA scan whenever legal | 3 exact kernels, one query per wave
 *     "timing"          1: (re)start recording HIP-event times of every search on its stream, averaged by vdb_stats
 *     "list_cap"        work-list capacity per query (0 = default max(64, 2k + 32))
 *     "panel_dtype"     0 auto: byte-valued integer corpora are ALSO kept as an int8 scan copy, and integer query batches
 *                       in the byte window are scanned with int8 MFMA | 1 fp16 scan only
 *     "int8_only"       flat index, D <= 128, more than 32 768 rows, takes effect at the next vdb_add: 0 (default) | 1: a byte-valued
 *                       corpus (every value an integer in 0..255 or in -128..127) keeps ONLY its int8 copies -- row-major int8 rows
 *                       + int8 MFMA panels + their accumulator inits, 0.55x the float32 bytes instead of 3x (the reference holds
 *                       one copy of the corpus, exact_search.py:34-39).  Same results: integer query batches take the int8 scan
 *                       and the integer refine as always; a batch with a non-integer value is scanned in fp16 over slabs converted
 *                       from the int8 panels per search (option "int8_slab_chunks", default 8 scan chunks = 16 MiB of scratch at
 *                       D = 128) and refined in float64 from x = byte + cx.  The rows stream through in blocks at build time (a
 *                       100M x 128 shard never exists in float32 inside the library).  Built by ONE add: appending is
 *                       VDB_ERR_UNSUPPORTED; a corpus that is not byte-valued silently gets the default layout
 *                       (vdb_stats.has_i8_copy tells: 2 = int8 only)
 *     "int8_block_rows" rows per ingestion block of that build, 0 (default: 4 194 304) .. 2^31 - 1, rounded up to whole 512-row
 *                       spans (tests: several blocks on a small corpus); also the rows per block of a vdb_ivf_add on an IVF-I8 index
 *                       (0 = default 1 048 576, not rounded): one block of float32 rows is all the device holds of them
 *     "stream_panels"   D > 128, takes effect at the next vdb_add: 0 (default) the fp16 scan copy stays resident next to the
 *                       float32 rows | 1 it is NOT kept: every search converts the float32 rows slab by slab into one
 *                       scratch slab and scans that (same results; 1.8x -> ~1.15x the corpus bytes resident for a corpus that
 *                       is not exact in fp16, one extra pass over the rows per query batch)
 *     "stream_slab_rows" rows of that scratch slab (0 = default 1 280 000, rounded down to whole scan chunks whose
 *                       workgroups fill whole rounds of the chip); inf is legal and, like any value of 9e18 or more given to this
 *                       option or to "filter_sparse_pairs", stored as 9e18
 *     "upload_block_mb" staging block of the row-block ingestion (default 64)
 *     "small_batch"     1 (default): batches of <= 512 queries are scanned with finer row chunks and, up to 256 queries,
 *                       1 / 2 / 4-wave workgroups, so that the grid still covers the chip; D > 128: waves without queries
 *                       only stage panels, <= 16 queries keep their query block in LDS | 0 the batch shape for every size
 *     "fused_stats"     1 (default): batches of <= 4096 query values (serving shapes) take their statistics inside the
 *                       query-operand kernel, one dependent dispatch less | 0 a separate statistics dispatch for every size
 *     "ivf_min_batch"   smallest query batch the list-major MFMA scan of the IVF index serves (default 1); smaller ones
 *                       take the exact per-query list scan
 *     "ivf_i8_scratch"  IVF-I8 index: 1 (default) a batch the int8 list scan cannot serve (a non-integer value, a value outside the
 *                       byte window, "panel_dtype" = 1) scans fp16 panels of the whole panel space, converted from the int8 panels
 *                       for that batch into a workspace slab of 2 bytes per (padded) dimension per panel row | 0 the slab is never
 *                       allocated: such a batch is flagged on the device and every query of it answered by the exact list scan
 *                       (vdb_stats.last_fallback_queries = nq).  Same results either way.  Measured on sift-like bytes 1M x 128,
 *                       IVF1024, 10 000 non-integer queries, nprobe 8 / 32 / 128 (scripts/bench_ivf_i8.py,
 *                       profiles/r26_bench_ivf_i8.json): 1 = 0.43 / 0.54 / 0.91 ms per batch (the conversion pass is ~0.08 ms of it) and
 *                       a 288 MB slab; 0 = 14.6 / 48.6 / 173.7 ms and no slab -- for indexes that see integer batches only.
 *                       Every other kind accepts it without effect
 *     "graph"           0 (default) | 1: a vdb_search_device / vdb_search_partial_device / vdb_ivf_search*_device call of
 *                       at most 4096 queries on a non-null stream that repeats with the same buffers, shape and stream
 *                       (a serving loop) is captured into a hipGraph on its second occurrence and replayed afterwards;
 *                       any vdb_set_option / add / train drops the graph; the caller keeps the buffers alive and
 *                       rewrites the queries in place.  (The call that drops a stale graph always runs eagerly: on ROCm 7.x an
 *                       executable graph instantiated right behind the destruction of its predecessor faults on its second
 *                       replay -- a runtime defect in graph packet capture, profiles/r04_graph_fault_cause.txt.)
 *     "lsh_force_fallback"  0 (default) | 1: every query of a vdb_lsh_candidates / vdb_lsh_search / vdb_lsht_candidates /
 *                       vdb_lsht_search call takes the exact fallback of the select (tests; same results)
 *     "pq_scan_min_batch"  PQ index: smallest query batch that takes the panel pass + MFMA scan, smaller ones take the exact
 *                       kernels on the codes (0 = default .. 1e9)
 *     "pq_slab_chunks"  PQ index: scan chunks per slab of panels made per search (0 = default: 524 288 rows' worth .. 4096)
 *     "pq_adc_max_batch"  PQ index: largest query batch that takes the lookup-table (ADC) scan of the codes instead of the panel pass
 *                       + MFMA scan, 0 (default: off) .. 512; accepted without effect on every other kind of index, and for a
 *                       batch the scan would not serve (direct-bin geometry, k > 1024, M >= 160).  Same results either way.
 *                       Measured on 1M rows (profiles/r18_bench_pq_adc.json): faster than the panel pass by more than 8 % up to
 *                       8 queries for PQ16 at D = 128 and PQ64 at D = 384, up to 2 for PQ64 at D = 128 -- the value to set; the
 *                       cost grows linearly with the batch beyond
 *     "ivfpq_adc_max_batch"  IVF-PQ index: largest query batch that takes the lookup-table (ADC) scan of the probed lists instead of
 *                       the panel pass + list-major MFMA scan (dim <= 128) or the exact list scan, 0 (default: off) .. 512; accepted
 *                       without effect on every other kind of index and for a batch the scan does not serve.  Same results either
 *                       way.  Costs 4 ntotal bytes of resident norms once a batch is admitted.  Measured (profiles/r19_bench_ivfpq_adc.json,
 *                       k = 10): faster than the option-off path by more than 8 % at every batch size up to 256 / 128 (IVF1024,PQ64 on
 *                       1M x 128, nprobe 8 / 32), 512 / 256 (PQ16) and 512 (IVF256,PQ64 on 100 000 x 384, nprobe 24) -- the value to set
 *     "ivfpq_adc_part_rows"  IVF-PQ index: rows per row part (one workgroup each) of that scan, 0 (default: auto) or a multiple of 256
 *                       up to 65 536 (tests, sweeps); raised so that the longest list has at most 64 parts
 *     "knng_nentry"     k-NN graph: entry points of a search, 0 (default: 32) .. 512
 *     "knng_max_iters"  k-NN graph: step cap of a search, 0 (default: 8 ef) .. 2^31 - 1
 *     "knng_visited_bits"  k-NN graph: log2 slots of the per-query seen filter, 0 (default: up to 12, the largest that keeps a query
 *                       within 20 KiB of LDS -- 8 waves per CU) .. 14; a filter that does not fit a workgroup's 64 KiB is made
 *                       smaller.  1 is legal; no value changes a result
 *     "knng_build_block"  k-NN graph: rows per self-search block of vdb_knng_build, 0 (default: 65 536) .. 1e9
 *     "range_bitmap_mb" range search: MiB of candidate bitmap (one bit per query and row) a query slab may take, 0 (default: 256)
 *                       .. 4096; a batch whose bitmap is larger runs in several slabs (same results; at least one query per slab)
 *     "filter_sparse_pairs"  filtered search: a call with fewer (query, admitted row) pairs than this takes the sparse route over the
 *                       list of admitted rows, 0 (never by this rule) .. inf, default 8192 (the measured crossover at D = 128, profiles/r21_bench_filter.json);
 *                       same results either way.  Set it
 *                       BEFORE vdb_filter_set: setting any option drops an installed filter, and the list is built at install
 *                       according to the value in force
 *     "multi_stage_all" multi-device handles only (vdb_create_multi; every other option is forwarded to each shard, and "graph"
 *                       = 1 is VDB_ERR_UNSUPPORTED there): 1 (tests) shards on devices[0] take the remote-shard path too
 *     "graph_recapture_at_once"  diagnostic, 0 (default) | 1: the pre-round-3 ordering, for re-checking that defect
 *                       ($VDBHIP_ALLOC_LOG=<file> logs every allocation / graph event for scripts/graph_fault_analyze.py)
 *   tuning knobs (scripts/sweep_*.py)
 *     "i8_variant"      0..7: tile / stage / wave shapes of the flat int8 scan (6 / 7: variant 3 with a pacing barrier
 *                       per 1 / 2 tiles)
 *     "i8_group"        8 (default) | 4 rows per select group of the flat int8 scan
 *     "flat_shape"      (before vdb_add; alias "i8_shape") MFMA shape of the flat scans for D <= 128 and the layout of their scan
 *                       copies: 0 auto (16) | 16 | 32.  16 = v_mfma_f32_16x16x32_f16 / v_mfma_i32_16x16x64_i8 on layout x16
 *                       (octs only; +17 - 19 % on the scans); 32 = the 32x32 kernels (also taken when an option asks for quads
 *                       -- "f16_group" / "i8_group" = 4)
 *     "scan_pair"       layout x16, index with an int8 copy: 1 (default) both scans in one launch (the device picks the body), 0 two
 *                       launches (the one not needed returns at once) -- A/B and diagnosis
 *     "f16_stage_tiles" / "f16_wide" / "scan_prio"   tuning of the x16 kernels (tiles per LDS stage of the fp16 batch scan: 0 auto | 4 | 8;
 *                       1024-query workgroup tiles of the fp16 scan at D <= 64: 0 auto | 1 never; issue priority of one half of a
 *                       workgroup: 0 | 1 | 2 -- measured, no gain)
 *     "f16_group"       8 (default) | 4 rows per select group of the fp16 flat scan (D <= 128)
 *     "i8_ring"         0 auto (4) | 2 | 4 | 8 LDS staging stages of the serving-shaped and IVF int8 scans
 *     "i8_nt"           0 (default) / 2: the serving-shaped int8 scan stages its panels with non-temporal loads | 1 off
 *     "ivf_nw"          0 auto | 2 / 4 / 8 waves per IVF work item
 *     "ivf_bt"          0 auto | 4 (64-row bins) | 16 (the largest: one bin per half of a 256-row span)
 *     "ivf_tps"         D > 128, takes effect at the next vdb_ivf_add: 0 auto | 16 (256-row spans, 64-row bins) | 64
 *                       (1024-row spans, 256-row bins) of the p16 panel space
 *     "ivf_group"       D > 128, 64-row bins: rows per candidate group of the list scan, 0 auto | 1 | 2 | 4 (smaller groups cost
 *                       select instructions in the scan and save gathered rows in the exact refine)
 *     "ivf_i8_group"    4 (default) | 8 rows per candidate group of the int8 list scan (D <= 128, byte-valued corpus)
 *     "ivf_tile"        D > 128, 256-row spans: workgroup tile of the list scan, 0 auto / 2 = 256 rows x 256 query slots | 1 = 128 x 512
 *     "ivf_part"        0 auto | spans (256 rows) per row part of the IVF list scan: long lists are cut into parts
 *                       scanned by one workgroup each (rounded up to a multiple of 4 bins)
 *     "select_variant"  0..2;  "spans_per_chunk", "kloop_qgroup": grid shaping of the flat scans */
int vdb_set_option(vdb_handle h, const char *key, double value);

/* ---- test hooks (used by tests/ to validate the error bound of the fp16 scan) -------------- */
/* raw scan scores (scaled units) for queries x rows [row0,row0+nrows), any D <= 4096: out (nq, nrows) float32,
 * together with the per-query bound eps (nq) and the scale cs so that score/cs ~ (||x||^2 - 2 q.x) or -q.x.
 * Flat indexes whose fp16 panels are resident, in every layout the scans use (vdb_stats.scan_shape 16 / 32, p16 for
 * D > 128); VDB_ERR_UNSUPPORTED for D > 128 on at most 2048 rows (no MFMA scan there) */
int vdb_debug_scan_scores(vdb_handle h, const float *q_host, int64_t nq, int64_t row0, int64_t nrows,
                          float *scores_host, float *eps_host, double *cscale);
/* the same for the lookup-table (ADC) scan of a flat PQ index with rows (M <= 159): raw, unpacked scores of the scan's own table
 * kernel and per-row scoring function, the ADC bound eps (nq) and cs.  Every other kind of handle: VDB_ERR_UNSUPPORTED */
int vdb_debug_pq_adc_scores(vdb_handle h, const float *q_host, int64_t nq, int64_t row0, int64_t nrows,
                            float *scores_host, float *eps_host, double *cscale);

/* the same for the lookup-table (ADC) scan of an IVF-PQ index with rows (M <= 159, any dim): the scan's own scores of the list-order
 * rows [row0, row0 + nrows) of list `probe_list` (out (nq, nrows) float32), computed as for a batch of these nq queries that all
 * probe that one list; the bound eps (nq; 0 for a query the scan would hand to the exact list scan) and the batch's scale cs.
 * Every other kind of handle: VDB_ERR_UNSUPPORTED */
int vdb_debug_ivfpq_adc_scores(vdb_handle h, const float *q_host, int64_t nq, int probe_list, int64_t row0, int64_t nrows,
                               float *scores_host, float *eps_host, double *cscale);

#ifdef __cplusplus
}
#endif
#endif /* VDBHIP_H */

/*
 * dhr_hip.h -- C ABI of libdhr_hip.so: MI355X (gfx950) brute-force dense-hybrid retrieval.
 *
 * The reference (castorini/dhr, /root/reference) has NO native/FFI interface for this path: the
 * hot path is Python calling torch ops (retrieval/gip_retrieval.py:60-165).  This header is the
 * boundary a maintainer would bind instead of those torch calls (ctypes stub: INTEGRATION.md).
 * Each entry point names the reference code it replaces.  Plain pointers and sizes only; no C++
 * exceptions, no exit() cross this boundary; every function returns 0 or a negative dhr_status.
 *
 * Threading: one handle is used by one host thread at a time; distinct handles (e.g. one per
 * device / per rank) may be used concurrently.
 *
 * Streams: every entry point works on the stream it is given.  dhr_search ENQUEUES its first attempt (sampled run, main pass, refine /
 * rescoring / select of every chunk: no host read-backs between the phases since round 3) with two small host reads on that stream: 32
 * bytes after the sampled run (the fullest candidate lists, which size the chunks of the main pass; DHR_PARAM_ASYNC_CONTROLLER = 1 drops
 * it for a fixed plan) and, at the end, the number of queries whose verification failed (a list overflowed, or the sampled threshold came
 * out too high -- adversarial row orders), because those are redone by a host-driven controller that is exact for any input.  It
 * returns with the stream idle.  Corpora too small to sample (below ~33 k rows) use the host-driven controller throughout.
 * dhr_search_begin / dhr_search_finish and dhr_search_sharded over RCCL enqueue everything up to ONE host read (the count of queries to repair).
 */
#ifndef DHR_HIP_H
#define DHR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHR_VERSION 105 /* 0.1.5 (entry points added since, none changed: the number stands): dhr_exclude_rows / dhr_search_excluding / dhr_debug_exclude_chunk (per-query row exclusion); 0.1.5: exception barrier on every entry point (DHR_ERR_NOMEM), a failed sharded step is collective (DHR_ERR_PEER), dhr_abi_size, dhr_host_shard::struct_size, dhr_comm_abort no longer frees the handle, counts + list prefixes in ONE all-gather; 0.1.4: dhr_search_pre / dhr_search_pre_ranks / dhr_search_begin_rest (first agreement of the sharded search in two rounds), dhr_host_shard::pre_ranks / pre / begin_rest, DHR_PARAM_LIST_STRIDE; 0.1.3: dhr_comm_info / dhr_comm_abort */

typedef enum dhr_status {
  DHR_OK = 0,
  DHR_ERR_INVALID = -1,     /* bad argument (NULL, negative size, unsupported dtype ...) */
  DHR_ERR_UNSUPPORTED = -2, /* legal input the kernels do not cover (see dhr_last_error) */
  DHR_ERR_HIP = -3,         /* a HIP runtime call failed (no device, OOM, launch failure) */
  DHR_ERR_INTERNAL = -4,
  DHR_ERR_NOMEM = -5,       /* a host allocation failed (std::bad_alloc caught at the boundary); the handle stays usable */
  DHR_ERR_PEER = -6         /* sharded search: ANOTHER rank failed in this step (its status travelled with the step's all-gathers); every rank
                               returns from the same step with an error -- the failing rank with its own status, the others with this one */
} dhr_status;

typedef enum dhr_idx_dtype { DHR_IDX_NONE = 0, DHR_IDX_U8 = 1, DHR_IDX_I8 = 2, DHR_IDX_I16 = 3 } dhr_idx_dtype;
/* DHR_VAL_BF16 is taken by the six lexical head entry points only (dhr_lexical_head, dhr_lexical_head_train / _backward, dhr_lexical_proj_head,
 * dhr_lexical_proj_train / _backward): as the dtype of the logits or of hidden / weight, of the projection's bias and of the gradients the two
 * backward calls write.  Every other value dtype argument (index records, query batches, value_out, cls, the other ops) refuses it. */
typedef enum dhr_val_dtype { DHR_VAL_F16 = 0, DHR_VAL_F32 = 1, DHR_VAL_BF16 = 2 } dhr_val_dtype;
typedef enum dhr_mem_kind { DHR_MEM_HOST = 0, DHR_MEM_DEVICE = 1 } dhr_mem_kind;

typedef struct dhr_index dhr_index; /* opaque */

/* One corpus shard in the reference's record layout (3-list pickle [value, index, ids]:
 * tevatron/driver/encode.py:165-170,203-204; merged by retrieval/index.py:26-47):
 *   value  fp16 [n_rows, d_dlr + d_cls] row-major, first d_dlr columns = densified lexical (gated),
 *          the rest = dense [CLS] (ungated);
 *   index  uint8 / int8 / int16 [n_rows, d_dlr], or NULL for dense-only models (then d_dlr = 0).
 * The library copies and re-lays the data into its own device layout (MFMA-fragment tiles); the
 * caller keeps ownership of the inputs and may free them after dhr_index_create returns. */
typedef struct dhr_index_desc {
  int32_t device;      /* HIP device ordinal */
  int32_t mem_kind;    /* dhr_mem_kind of value/index */
  int64_t n_rows;      /* rows of THIS shard (gip_retrieval.py:292-306 slice) */
  int32_t d_dlr;       /* gated columns == --emb_dim when index != NULL, else 0.  Any width: where it is not a multiple of 8 the library
                          appends zero slices to its own copies (of the corpus and of every query batch) */
  int32_t d_cls;       /* ungated columns */
  const void* value;   /* fp16 */
  int64_t ld_value;    /* elements between consecutive rows (>= d_dlr + d_cls) */
  const void* index;   /* or NULL */
  int32_t index_dtype; /* dhr_idx_dtype */
  int32_t idx_buckets; /* index buckets per gated slice in the bound GEMM operands (0 = default: 2, on the 2:4 sparse matrix cores; 1 = ungated bound) */
  int64_t ld_index;    /* elements between consecutive rows (>= d_dlr) */
  int64_t row_offset;  /* global row id of local row 0; added to every returned row */
} dhr_index_desc;

/* A batch of queries, same record layout as the corpus (value may also be fp32: the reference's
 * CPU path converts queries to fp32 and scales the CLS tail by --lamda in fp32,
 * gip_retrieval.py:275-283 -- hand that fp32 array over unchanged). */
typedef struct dhr_query_batch {
  int32_t n_queries;
  int32_t mem_kind;
  const void* value;   /* [n_queries, d_dlr + d_cls] */
  int32_t value_dtype; /* dhr_val_dtype */
  int32_t index_dtype; /* dhr_idx_dtype; NONE iff the index was built without an index array */
  int64_t ld_value;
  const void* index;   /* [n_queries, d_dlr] or NULL */
  int64_t ld_index;
} dhr_query_batch;

/* Counters of the last dhr_search on a handle (what the phase controller did and how long the
 * kernels ran, measured with hipEvents on the search stream). */
typedef struct dhr_search_stats {
  int64_t n_rows, n_queries, k;
  int32_t phases;            /* bound-GEMM launches */
  int32_t overflow_retries;  /* phases re-run in halves because a candidate list filled */
  int64_t candidates_bound;  /* pairs that passed the bound filter (sum over queries) */
  int64_t candidates_exact;  /* pairs rescored exactly (incl. the dense first phase) */
  int64_t gemm_rows;         /* corpus rows pushed through the bound GEMM */
  int64_t sample_fallback_queries; /* queries redone exactly because the sampled threshold was too high */
  double gemm_ms, refine_ms, rescore_ms, select_ms, prep_ms, total_ms;
  double gemm_flops;         /* 2 * Q_pad * rows * K_tile actually issued by the bound GEMM (padding, bucket split) */
  double gemm_flops_alg;     /* algorithmic: 2 * Q * rows * (d_dlr + d_cls), summed over the launches */
} dhr_search_stats;

/* Tunables (dhr_index_set_param). */
typedef enum dhr_param {
  DHR_PARAM_CAND_CAP = 1,     /* per-query candidate list capacity (entries) */
  DHR_PARAM_FIRST_ROWS = 2,   /* rows scored exhaustively to seed the thresholds (>= k enforced) */
  DHR_PARAM_PROFILE = 3,      /* 1: record per-kernel hipEvent timings into dhr_search_stats */
  DHR_PARAM_MAX_GROWTH = 4,   /* max (next chunk rows) / (rows seen), in 1/16ths (default 32 = 2x) */
  DHR_PARAM_MAIN_CHUNKS = 7,  /* lower limit of the number of main-pass chunks (the controller adds chunks so that the candidate lists fit) */
  DHR_PARAM_AUX_CUS = 9,      /* main pass: confine refine / rescoring / select to this many CUs (multiple of 8, spread over the XCDs; 0 = no CU mask; default: 128 for dense-only indexes, no mask for gated ones) */
  DHR_PARAM_GEMM_EXCLUSIVE = 10, /* with AUX_CUS: 1 = run the bound GEMM on the other CUs only */
  DHR_PARAM_OVERLAP_AUX = 11,  /* 0: refine / rescoring / select of a chunk run after its GEMM on the same stream; 1: beside the GEMM of the next chunk on a CU-masked stream; -1 (default): 1 */
  DHR_PARAM_PROGRESSIVE_THR = 8, /* later main-pass chunks filter with 1: the running exact k-th best; 2 (default): additionally the rank extrapolated from the scattered fraction of the corpus seen so far (main pass in a scattered tile order; a query whose extrapolation was too high fails the final verification and is redone); 0: the sampled threshold only */
  DHR_PARAM_GEMM_VARIANT = 6, /* bound-GEMM kernel of the 2:4 layout: 3 = 12 waves (producer / consumer), 4 = 4 waves with 128 x 128 wave tiles, 5 = 8 waves with 128 x 64 wave tiles (default), 6 = 5, and on gated_i8 indexes persistent workgroups (gemm_g8p.hip: the same results and, the kernel being held by the package power cap, the same time in fewer cycles -- DESIGN.md section 4b) */
  DHR_PARAM_ASYNC_CONTROLLER = 13, /* the first attempt of a sampled search ENQUEUES its phases without reading list lengths back between them.
                                     2 (default): one 32-byte read after the sampled run (the fullest lists: how many chunks the main pass
                                     needs) + ONE at the end (the number of queries whose verification failed); 1: the final read only (fixed
                                     chunk plan; what the staged / sharded entry points always do); 0: the host-driven controller (reads the list
                                     lengths back after every phase).  DHR_ASYNC overrides. */
  DHR_PARAM_SAMPLE_SHARE = 12, /* staged search only (dhr_search_begin / finish): the number of shards the sampled threshold is agreed between; a shard then
                                 reports its r / shards + 5 sqrt(r / shards) + 4 best sample scores (dhr_search_sample_rank) instead of all r
                                 (dhr_search_union_rank), and plans its lists for its SHARE of k: a shard that turns out to hold far more of the top-k
                                 than k / shards reports count = -1 for those queries in dhr_search_finish (the caller's repair step, which
                                 dhr_search_sharded* run themselves, redoes them with local thresholds).  dhr_search_sharded[_local] set the
                                 parameter themselves.  Default 1. */
  DHR_PARAM_LIST_STRIDE = 14, /* entries every query owns in the uniform part of the bound-candidate lists (default 0 = 32 768); what a hot query needs
                                 beyond that comes from a shared arena planned on the device (two-tier lists: the workspace of an 8.8 M-row index is
                                 ~7 GB instead of 34).  Takes effect for indexes with a refine level whose planned list depth exceeds it; tests
                                 force a small stride to exercise the second tier on small inputs.  0 or a multiple of 256 in [1024, 4194304] */
  DHR_PARAM_SEAT_QUERIES = 15, /* main pass of a whole search of a gated int8 index (gemm_filter_g8_kernel with gated stages), batches of 257 .. 8 192 padded queries:
                                  -1 (default) = the queries are seated in the kernel's query tiles by descending length of their bound lists over the
                                  sampled run, so that the few queries that pass 10-100 x the average through the filter share wave columns instead of
                                  slowing their neighbours' scan; 0 = every query sits where the caller put it.  Results, candidate
                                  sets and launch plan do not depend on it.  Staged and sharded calls, the fp16-gated kernels, dense-only indexes (measured:
                                  no gain) and the fallback controllers never seat */
  DHR_PARAM_SAMPLE_PERIOD = 5 /* every S-th corpus tile seeds the thresholds (default 32; 0 = plain streaming) */
} dhr_param;

/* Process-wide options read by dhr_index_create (dhr_set_option). */
typedef enum dhr_option {
  DHR_OPT_DENSE_I8 = 1, /* int8 image of the UNGATED columns in the bound GEMM (v_mfma_i32_32x32x32_i8, twice the fp16 instruction's
                           columns per issue; the quantisation error is paid by the filter margin, results stay exact):
                           -1 (default) = gated indexes that also carry ungated columns, and dense-only shards of at least 1 000 000 rows whose
                           measured quantisation error is small against the spread of their scores (sqrt(d_cls) x max row error / max row norm
                           <= 0.45); 0 = never, 1 = every dense-only index too.
                           The environment variable DHR_DENSE_I8 overrides it. */
  DHR_OPT_GATED_I8 = 2  /* int8 image of the GATED columns too (v_smfmac_i32_32x32x64_i8: the 2:4 instruction on int8 operands, 32 slices
                           per issue; values rounded UP per column step, so the bound stays a bound and results stay exact):
                           -1 (default) = shards of at least 1 000 000 rows (4 000 000 where the ungated half is narrower than half the
                           gated one), where the cheaper GEMM outweighs the extra candidates the looser bound lets through (below
                           that the refine / rescoring work dominates the step); 1 = wherever the layout
                           allows it (two buckets, d_dlr a multiple of 64, the ungated half an int8 image or absent); 0 = keep the fp16
                           image.  The environment variable DHR_GATED_I8 (-1 / 0 / 1) overrides it. */
} dhr_option;
int dhr_set_option(int32_t option, int64_t value);
/* Read-only facts about a built index (dhr_index_get_info). */
typedef enum dhr_info {
  DHR_INFO_DENSE_I8 = 1,      /* 1 if the ungated stages are int8 images */
  DHR_INFO_I8_SCALE = 2,      /* corpus-side scale: max |ungated value| / 127 */
  DHR_INFO_I8_ROW_ERR = 3,    /* max over rows of || d - scale * q8(d) ||   (ungated part) */
  DHR_INFO_I8_ROW_NORM = 4,   /* max over rows of || scale * q8(d) || */
  DHR_INFO_ROW_NORM_MAX = 5,  /* max over rows of || row || */
  DHR_INFO_TILE_BYTES = 6,    /* bytes of the bound-GEMM operand images */
  DHR_INFO_GATED_I8 = 7,      /* 1 if the gated stages are int8 2:4 images */
  DHR_INFO_GEMM_KERNEL = 8    /* the bound-GEMM kernel the handle's latest search launched (0: none yet): 3 / 4 gemm_filter_wx_kernel<2> / <4>
                                 (fp16 2:4 image, 8 / 4 waves), 5 gemm_filter_g8_kernel (integer operands, 8 waves), 6 the same with persistent workgroups (A/B
                                 builds only); 1 and 2 named the two kernels retired in version 105 and are never reported */
} dhr_info;
int dhr_index_get_info(const dhr_index* index, int32_t what, double* out);

int dhr_version(void);
/* sizeof of the four public structs as this library was compiled: { dhr_index_desc, dhr_query_batch, dhr_search_stats,
 * dhr_file_info }.  A binding compares them with its own declarations at load time (a stale library whose struct layout
 * differs would otherwise corrupt memory silently). */
void dhr_abi_sizes(int32_t out[4]);
/* The same, one struct at a time (new structs get an id here instead of a longer array): returns sizeof as compiled, or a negative status. */
enum { DHR_ABI_INDEX_DESC = 0, DHR_ABI_QUERY_BATCH = 1, DHR_ABI_SEARCH_STATS = 2, DHR_ABI_FILE_INFO = 3, DHR_ABI_HOST_SHARD = 4 };
int32_t dhr_abi_size(int32_t which);
/* Message of the last failure on the calling thread ("" if none). */
const char* dhr_last_error(void);

/* Replaces the corpus half of main() (gip_retrieval.py:289-315: slice, astype, .cuda). */
int dhr_index_create(const dhr_index_desc* desc, dhr_index** out);
void dhr_index_destroy(dhr_index* index);
int dhr_index_set_param(dhr_index* index, int32_t param, int64_t value);
/* Device bytes held by the handle (index + workspaces). */
int64_t dhr_index_device_bytes(const dhr_index* index);

/* Index file.  The reference keeps ONE monolithic pickle that every run unpickles,
 * casts to fp32 and copies to the GPU (gip_retrieval.py:289-315).  dhr_index_save writes the corpus of a built
 * index as page-aligned raw sections of one file -- row-major fp16 values (rows padded to a multiple of 64
 * columns), row-major slice indices -- plus an opaque caller blob (the docid list); dhr_index_load mmaps the
 * file and streams it to the device through the ordinary ingest path: no unpickling, no host copies.  The
 * device images (operand tiles, refine lists) are NOT stored: re-tiling from device memory costs 0.06 s per
 * 2 M rows, the images would double the file.  row_offset < 0 keeps the stored value. */
typedef struct dhr_file_info {
  int64_t n_rows, row_offset;
  int32_t d_dlr, d_cls, index_dtype, idx_buckets;
  uint32_t file_version, reserved;
  int64_t payload_bytes;           /* value + index bytes in the file */
  int64_t blob_offset, blob_bytes; /* the caller blob: plain file bytes [blob_offset, blob_offset + blob_bytes) */
} dhr_file_info;
int dhr_index_save(const dhr_index* index, const char* path, const void* blob, int64_t blob_bytes);
int dhr_index_file_info(const char* path, dhr_file_info* out);
int dhr_index_load(const char* path, int32_t device, int64_t row_offset, dhr_index** out);

/* Replaces the query loop of GIP_retrieval (brute force, gip_retrieval.py:115-126) and of
 * IP_retrieval (:70-79) for ALL queries of the batch at once:
 *   score[q][n] = sum_{j<d_dlr} [c_idx[n][j]==q_idx[j]] * c_val[n][j]*q_val[j] + sum_{c} c_val*q_val
 * and returns per query the k best rows, best first (score desc, row asc on exact ties).
 *   out_scores [n_queries, k] fp32, out_rows [n_queries, k] int64 GLOBAL rows (row_offset added);
 *   if k > n_rows the tail is (-inf, -1)   (the reference raises / truncates: SURVEY appendix).
 * Scores are the exactly-rounded value of the gated inner product (fp64 accumulation of exact
 * products), i.e. within fp32 summation noise of the reference's einsum.
 * out_mem_kind says where out_scores/out_rows live.  stream is a hipStream_t (NULL = default). */
int dhr_search(dhr_index* index, const dhr_query_batch* queries, int32_t k, float* out_scores,
               int64_t* out_rows, int32_t out_mem_kind, void* stream);

/* Two-stage approximate GIP, both stages on the device (gip_retrieval.py:128-156):
 *   stage 1 = dhr_search(stage1, k1): the caller has restricted the batch the way the reference does -- values
 *             <= theta zeroed (:130-136), or index = NULL for the ungated --IP first stage (:139);
 *   stage 2 = exact gated inner product of the FULL batch on exactly those k1 rows (:144-146), top-k of that
 *             (score desc, row asc; fewer than k valid rows -> (-inf, -1) padding).
 * Same n_queries in both batches; 0 < k <= k1 <= 1048576 (above 16384 the global-memory merge, slower). */
int dhr_search_rerank(dhr_index* index, const dhr_query_batch* stage1, const dhr_query_batch* full, int32_t k1, int32_t k,
                      float* out_scores, int64_t* out_rows, int32_t out_mem_kind, void* stream);

/* Per-query row exclusion (hard-negative mining: a query's positives; corpora searched against themselves: the query's own row).
 * Exclusion lists are a CSR: excl_ptr_host int64 [n_queries + 1], a HOST array whatever the memory kind of the rest (as weights / teacher_split
 * of dhr_train_loss: the host needs the longest list to size the launch and the search depth without a hidden device read; it is read before
 * the call returns), offsets from 0 and never decreasing; excl_rows int64 GLOBAL rows in mem_kind memory, in any order, repeats allowed; rows
 * < 0 and rows that occur in no list are ignored (a -1 never matches padding).  excl_rows may be NULL when every list is empty.
 *
 * dhr_exclude_rows: drops from each query's ranked list the rows of its exclusion list and keeps the k_out best of the rest (input order kept).
 *   in_scores / in_rows [n_queries, n_in], best first, entries with row < 0 are padding (anywhere) and are dropped too; out_scores / out_rows
 *   [n_queries, k_out]: the first k_out surviving pairs, then (-inf, -1); out_valid int32 [n_queries] (may be NULL): the pairs written.  Serves
 *   the lists of dhr_search_rerank, dhr_pq_search, the sharded calls and the merges: ask them for k + E rows and filter.  All arrays but
 *   excl_ptr_host live in mem_kind memory; input and output must not overlap.  Device arrays: the call ENQUEUES on `stream` and returns without
 *   waiting (its one scratch block is allocated and freed in stream order); host arrays are staged through the device and complete on return.
 *   One workgroup per query; the list is staged into LDS in chunks of DHR_EXCLUDE_CHUNK rows (dhr_debug_exclude_chunk returns the constant the
 *   library was built with), a longer list costs further passes; no atomics on global memory: two calls on the same arguments are bit-identical.
 *   DHR_ERR_INVALID: a NULL pointer, excl_ptr_host[0] != 0, a decreasing excl_ptr_host, n_in <= 0, k_out <= 0 or k_out > n_in, an unknown
 *   mem_kind; DHR_ERR_UNSUPPORTED: n_in > 1048576 together with a list longer than one chunk.
 * dhr_search_excluding: dhr_search, except that query q never returns a row of excl_rows[excl_ptr[q] .. excl_ptr[q+1]).  Runs the ordinary
 *   search at depth k' = k + Emax (Emax: the longest list of the batch) into scratch of the handle, filters, and delivers [n_queries, k] to
 *   out_mem_kind memory; excl_rows lives in excl_mem_kind memory.  Exact by construction: the top k' holds at most Emax excluded rows, hence
 *   at least min(k, live rows) others, and they are the best of the others in the library's order.  Emax == 0 IS dhr_search (bit for bit).
 *   k' > 1048576: DHR_ERR_UNSUPPORTED; k' > 16384 takes the global-memory select of any deep dhr_search (slower); k' > n_rows relies on the
 *   (-inf, -1) tail.  ONE long list deepens the search of the whole batch: a caller with a few queries of thousands of exclusions puts them
 *   in a batch of their own.  Afterwards dhr_get_stats describes the underlying search at depth k'. */
#define DHR_EXCLUDE_CHUNK 2048 /* rows of an exclusion list per LDS pass of dhr_exclude_rows */
int dhr_exclude_rows(int32_t device, int32_t mem_kind, int32_t n_queries, int32_t n_in, const float* in_scores, const int64_t* in_rows,
                     const int64_t* excl_ptr_host, const int64_t* excl_rows, int32_t k_out, float* out_scores, int64_t* out_rows,
                     int32_t* out_valid, void* stream);
int dhr_search_excluding(dhr_index* index, const dhr_query_batch* queries, int32_t k, const int64_t* excl_ptr_host, const int64_t* excl_rows,
                         int32_t excl_mem_kind, float* out_scores, int64_t* out_rows, int32_t out_mem_kind, void* stream);
int32_t dhr_debug_exclude_chunk(void);

/* Staged form of dhr_search for the row-sharded path (one handle per shard / rank).  After
 * dhr_search_begin every shard holds the r best exact scores of its SAMPLE per query (r =
 * dhr_search_sample_rank, the same on equally sized shards; 0 = the shard is too small to sample and
 * begin already ran the whole search).  The caller gathers the [n_queries, r] score blocks of all
 * shards, takes the r-th best of the union per query as the common threshold tau_hat and hands it to
 * dhr_search_finish, which runs the main pass with it and returns the shard's top-k plus, per query,
 * how many of its rows reach tau_hat (-1: a candidate list overflowed).  If the counts of all shards
 * sum to >= k (and none is -1) the union of the shard lists contains the global top-k; otherwise
 * those queries are redone with dhr_search.  Replaces one process per shard + merge.result.py.
 * out_sample_scores_dev / tau_hat_dev / out_count_dev are DEVICE pointers.
 * Errors: a staged call (begin, finish, and the optional mid / pre / begin_rest below) that returns an error leaves NO staged search
 * open on the handle -- its workspace may be half-consumed -- so a later dhr_search_mid / dhr_search_finish is refused ("without a matching
 * dhr_search_begin"): after an error from any staged call, start again with dhr_search_begin or dhr_search_pre. */
int32_t dhr_search_sample_rank(const dhr_index* index, int32_t k);
/* The rank of the union of the shards' samples that defines the common threshold (== dhr_search_sample_rank unless
 * DHR_PARAM_SAMPLE_SHARE > 1): the caller merges the gathered [shards, Q, sample_rank] lists and takes the
 * min(union_rank, shards * sample_rank)-th best per query. */
int32_t dhr_search_union_rank(const dhr_index* index, int32_t k);
int dhr_search_begin(dhr_index* index, const dhr_query_batch* queries, int32_t k, float* out_sample_scores_dev, void* stream);
int dhr_search_finish(dhr_index* index, const float* tau_hat_dev, float* out_scores, int64_t* out_rows,
                      int32_t* out_count_dev, int32_t out_mem_kind, void* stream);
/* Optional step between the two: a SECOND agreement on the thresholds.  dhr_search_mid runs the first slice of the main pass (1/8 of it,
 * in scattered order) with the thresholds of the first agreement and leaves the shard's r_local best scores seen so far -- head, sample and
 * slice -- in out_scores_dev [n_queries, r_local] (r_local: dhr_search_mid_ranks, or the largest over the shards where their sizes differ).
 * The shards have then seen the fraction f of their rows; the caller gathers the blocks and
 * takes the r_union-th best of the union per query (r_union = k f + 6 sigma + 4: it lies below the final k-th best), and hands
 * max(first threshold, that) to dhr_search_finish, which runs the rest of the pass with it and counts against it.  A 1/8 shard of the 8.8 M-row
 * benchmark then rescores ~360 instead of ~490 rows per query in its main pass.  dhr_search_mid_ranks returns r_local (also through
 * out_local; 0: this index has no such step -- it is too small -- and dhr_search_finish follows dhr_search_begin directly). */
int32_t dhr_search_mid_ranks(const dhr_index* index, int32_t k, int32_t* out_local, int32_t* out_union);
int dhr_search_mid(dhr_index* index, const float* tau_hat_dev, int32_t r_local, float* out_scores_dev, void* stream);
/* Optional: dhr_search_begin in TWO calls with an agreement in between (round 5).  dhr_search_pre prepares the batch and streams the first
 * part of the shard's sample (1/8 of it), leaving the shard's r_local best scores seen so far in out_scores_dev [n_queries, r_local]
 * (dhr_search_pre_ranks; 0: the sample is too small to split -- use dhr_search_begin).  The caller gathers the blocks, takes the r_union-th
 * best of the union per query (it lies below the union sample's final rank-r score: the same argument as inside a sampled run) and hands it to
 * dhr_search_begin_rest, which streams the rest of the sample filtering at it and leaves the handle exactly where dhr_search_begin does
 * (out_sample_scores_dev [n_queries, dhr_search_sample_rank]).  Eight shards that each ran their sampled run from nothing rescored 3.2 k rows per
 * query between them where the unsharded search's one run rescores 0.7 k. */
int32_t dhr_search_pre_ranks(const dhr_index* index, int32_t k, int32_t* out_local, int32_t* out_union);
int dhr_search_pre(dhr_index* index, const dhr_query_batch* queries, int32_t k, int32_t r_local, float* out_scores_dev, void* stream);
int dhr_search_begin_rest(dhr_index* index, const float* tau_dev, float* out_sample_scores_dev, void* stream);

/* Exact gated inner product of each query against m given rows (stage 2 of --rerank,
 * gip_retrieval.py:144-146 / :207-208).  rows [n_queries, m] int64 GLOBAL rows (row < 0 -> -inf).
 * out_scores [n_queries, m].  Pointers live in mem_kind memory. */
int dhr_score_rows(dhr_index* index, const dhr_query_batch* queries, int32_t m, const int64_t* rows,
                   float* out_scores, int32_t mem_kind, void* stream);

/* The multi-shard reduce (retrieval/merge.result.py:22-42 without the text round trip): per query,
 * the k_out best of n_lists*k_in (score, row) pairs, best first (score desc, row asc); entries with
 * row < 0 are padding.  in_scores/in_rows are [n_queries, n_lists*k_in] (each query's lists
 * concatenated).  All four pointers are DEVICE pointers on `device`.  Any n_in (up to 16 384 entries per query in one workgroup's LDS,
 * beyond that two stable segmented sorts through global memory; n_queries * n_in < 2^31).  The call ENQUEUES on `stream` and returns without
 * waiting (the scratch of the sorted path is allocated and freed in stream order). */
int dhr_merge_topk(int32_t device, int32_t n_queries, int32_t n_in, const float* in_scores,
                   const int64_t* in_rows, int32_t k_out, float* out_scores, int64_t* out_rows, void* stream);
/* Same reduce on HOST pointers (no GPU needed; used by the CPU/gloo tests of the sharded path). */
int dhr_merge_topk_host(int32_t n_queries, int32_t n_in, const float* in_scores, const int64_t* in_rows,
                        int32_t k_out, float* out_scores, int64_t* out_rows);

/* The same reduce for lists that are already SORTED, in the layout an all-gather of the per-shard results
 * leaves them in: in_scores / in_rows are [n_lists, n_queries, list_len]; every list is in output order
 * (score desc, row asc) with its padding (row < 0) at the tail -- what dhr_search / dhr_search_finish write.
 * No sort is run: every entry finds its output rank by binary searches in the other lists.  in_rows may be
 * NULL (scores only, e.g. the shards' sample scores of dhr_search_begin; ties keep list order; out_rows is
 * ignored).  (n_lists*list_len + k_out)*12 B (4 B without rows) must fit 160 KiB, n_lists <= 64.  DEVICE pointers
 * on `device`.  The call ENQUEUES on `stream` and returns without waiting. */
int dhr_merge_topk_lists(int32_t device, int32_t n_queries, int32_t n_lists, int32_t list_len, const float* in_scores,
                         const int64_t* in_rows, int32_t k_out, float* out_scores, int64_t* out_rows, void* stream);
/* Host twin (no sortedness needed: it sorts). */
int dhr_merge_topk_lists_host(int32_t n_queries, int32_t n_lists, int32_t list_len, const float* in_scores,
                              const int64_t* in_rows, int32_t k_out, float* out_scores, int64_t* out_rows);
/* Fused densify, the step immediately upstream of the index (tevatron/DHR/utils.py:5-22 and the
 * casts of tevatron/driver/encode.py:155-158,180-183).  lexical is [batch, vocab] (value_dtype DHR_VAL_F32 or DHR_VAL_F16,
 * row stride ld); the columns [remove_dims, vocab) are viewed as [n_groups, dims] and
 *   out_value[b][j] = max_g lexical[b][remove_dims + g*dims + j]     (out_value_dtype: DHR_VAL_F16 rounds to fp16, DHR_VAL_F32 exact)
 *   out_index[b][j] = the FIRST g attaining it                        (index_dtype DHR_IDX_U8, needs n_groups <= 256, or DHR_IDX_I16)
 * written with row strides ld_value / ld_index, i.e. directly into the value / index arrays of an index record (the
 * CLS columns follow at out_value + dims).  DHR_ERR_INVALID when (vocab - remove_dims) is not a multiple of dims
 * (the reference raises ValueError).  All three arrays live in mem_kind memory.  Device arrays: the call ENQUEUES on `stream` and returns
 * without waiting, like the training ops below; host arrays are staged through the device and are complete on return. */
int dhr_densify(int32_t device, int32_t mem_kind, const void* lexical, int32_t value_dtype, int64_t ld, int64_t batch, int32_t vocab,
                int32_t remove_dims, int32_t dims, void* out_value, int32_t out_value_dtype, int64_t ld_value, void* out_index,
                int32_t index_dtype, int64_t ld_index, void* stream);
/* Densify of SPARSE term-weight vectors, the producer of the BM25 / DeepImpact / uniCOIL / SPLADE indexes (densify/densify_corpus.py:29-52,
 * densify/densify_query.py:96).  The vectors come as CSR: the entries of vector b are [row_ptr[b], row_ptr[b + 1]) of term_ids (id_bytes 4: int32,
 * 8: int64) and weights (weight_dtype DHR_VAL_F16 or DHR_VAL_F32), nnz entries in all.  Per vector the entries (t, w) are folded IN THE ORDER
 * GIVEN, with r = fp16(w) rounded once to nearest even, s = (t - omission) % dims, g = (t - omission) / dims:
 *   value[s] == 0 (+0.0 or -0.0):  value[s] = r, index[s] = g          (so an entry that rounds to zero sets the index and leaves the slice empty)
 *   otherwise:                      a collision; value[s] = r, index[s] = g if value[s] < r, compared in fp16
 * bit for bit what the reference leaves with NumPy >= 2.  Entries with t < omission, t < 0 or t >= vocab are skipped and not counted; no term id
 * is used as an address.  Row ranges are clamped to [0, nnz]; a row whose end lies before its start is empty.  NaN weights are not covered.
 *   out_value [batch, dims]   DHR_VAL_F16, or DHR_VAL_F32 holding the fp16-rounded value; row stride ld_value >= dims
 *   out_index [batch, dims]   DHR_IDX_I8 (the reference's dtype without whole-word matching), DHR_IDX_U8 or DHR_IDX_I16 (with it); ld_index >= dims
 *   collisions [batch]        int32, may be NULL
 * Every output row is written whole, zeros included, straight into the caller's record arrays.  DHR_ERR_INVALID for a null pointer (term_ids and
 * weights may be NULL when nnz is 0), a bad mem_kind or dtype code, negative sizes, omission outside [0, vocab), dims <= 0, strides below dims,
 * and when the largest group (vocab - 1 - omission) / dims does not fit index_dtype (the reference raises OverflowError when it meets such a
 * term); DHR_ERR_UNSUPPORTED for dims > 8192.  batch == 0 returns DHR_OK without touching a device.  All arrays live in mem_kind memory.  Device
 * arrays: the call ENQUEUES on `stream` and returns without waiting; host arrays are staged through the device and are complete on return. */
int dhr_densify_sparse(int32_t device, int32_t mem_kind, const int64_t* row_ptr, const void* term_ids, int32_t id_bytes, const void* weights,
                       int32_t weight_dtype, int64_t nnz, int64_t batch, int64_t vocab, int32_t omission, int32_t dims, void* out_value,
                       int32_t out_value_dtype, int64_t ld_value, void* out_index, int32_t index_dtype, int64_t ld_index, int32_t* collisions,
                       void* stream);

/* The lexical head of the encoders fused with the step after it (tevatron/DHR/modeling.py:297-300,328-331,
 * tevatron/Aggretriever/modeling.py:274-278,306-310; then densify or aggregate and the fp16 casts of tevatron/driver/encode.py:149-194).
 * logits is [batch, n_tokens, vocab] (value_dtype DHR_VAL_F16 / DHR_VAL_BF16 / DHR_VAL_F32, strides ld_batch / ld_token / 1: the [:, 1:] view of the
 * model's [B, L, V] logits), term_weights and mask are fp32 [batch, n_tokens] (row strides ld_weights / ld_mask).  With
 * p = softmax over the whole vocabulary in fp32,
 *   reps[b][v] = max_t (p[b][t][v] * w[b][t]) * mask[b][t]       (first token on ties: a fully masked column keeps the sign of its first w)
 * and mode selects what is written, with row strides, straight into the caller's record arrays:
 *   DHR_LEX_RAW       out_value [batch, vocab] = reps                                      (dims / remove_dims ignored)
 *   DHR_LEX_DENSIFY   densify(reps, dims, remove_dims): out_value [batch, dims], out_index (DHR_IDX_U8 / DHR_IDX_I16, first group on ties)
 *   DHR_LEX_AGG_FULL  aggregate(reps, dims, full=True): groups of 2*dims columns from remove_dims (a negative remove_dims pads -remove_dims
 *                     zero columns at the end), then pos * (pos > neg) - neg * (pos <= neg) of the even / odd columns
 *   DHR_LEX_AGG_SEMI  aggregate(reps, dims, full=False): groups of dims columns from remove_dims >= 0
 * out_value_dtype DHR_VAL_F16 rounds to fp16 (out_value and cls are never bf16).  bf16 logits widen to fp32 exactly: the same values in fp16 and
 * in bf16 give the same bits.  cls_dim > 0 copies cls [batch, cls_dim] (row stride ld_cls) into the record columns that follow
 * (vocab or dims), so ld_value >= those + cls_dim.  workspace: NULL, or batch * n_tokens * 16 bytes of device memory on `device` (device
 * arrays only).  All arrays live in mem_kind memory; host arrays are staged through the device in blocks of rows.  NaN and +inf logits
 * are out of scope; every unmasked row needs a finite logit.  DHR_ERR_INVALID when the vocabulary does not split into whole groups.
 * The call runs on `stream` and WAITS for it (with workspace == NULL it frees its own allocation): the outputs are complete on return. */
typedef enum dhr_lexical_mode { DHR_LEX_RAW = 0, DHR_LEX_DENSIFY = 1, DHR_LEX_AGG_FULL = 2, DHR_LEX_AGG_SEMI = 3 } dhr_lexical_mode;
int dhr_lexical_head(int32_t device, int32_t mem_kind, int32_t mode, const void* logits, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                     int32_t vocab, int64_t ld_batch, int64_t ld_token, const float* term_weights, int64_t ld_weights, const float* mask,
                     int64_t ld_mask, int32_t dims, int32_t remove_dims, void* out_value, int32_t out_value_dtype, int64_t ld_value,
                     void* out_index, int32_t index_dtype, int64_t ld_index, const void* cls, int32_t cls_dtype, int64_t ld_cls, int32_t cls_dim,
                     void* workspace, void* stream);
/* aggregate of already computed lexical reps [batch, vocab] (tevatron/Aggretriever/utils.py:16-44) on the same kernel: full != 0 is
 * DHR_LEX_AGG_FULL, else DHR_LEX_AGG_SEMI; out [batch, dims] (row stride ld_out).  The caller passes remove_dims as the reference computes it
 * (cal_remove_dim).  Runs on `stream` and waits for it: out is complete on return. */
int dhr_aggregate(int32_t device, int32_t mem_kind, const void* lexical, int32_t value_dtype, int64_t ld, int64_t batch, int32_t vocab,
                  int32_t dims, int32_t remove_dims, int32_t full, void* out, int32_t out_dtype, int64_t ld_out, void* stream);

/* dhr_lexical_head with the vocabulary projection in front of it fused in, for ENCODING (forward only): the MLM logits
 *   x[b][t][v] = sum_k hidden[b][t][k] * weight[v][k] + bias[v]      (fp32 products and sums, never rounded to fp16)
 * are never written to memory, and masked tokens are never multiplied.  hidden is [batch, n_tokens, hidden_dim] (value_dtype DHR_VAL_F16 or
 * DHR_VAL_BF16: v_mfma_f32_32x32x16_f16 / _bf16, the same tiling, walk and reduction order for both;
 * strides ld_batch / ld_token / 1: the [:, 1:] view of the projector's input, read in place; hidden_dim a multiple of 8), weight is
 * [vocab, hidden_dim] of the same dtype (row stride ld_weight), bias [vocab] (bias_dtype DHR_VAL_F32 / DHR_VAL_F16; DHR_VAL_BF16 with bf16 operands) or NULL.  term_weights,
 * mask, mode, dims, remove_dims and every output argument are those of dhr_lexical_head, and so is what is written: reps, ties (the first
 * token, the first group) and the signs of zero; a masked token enters as (p * w) * 0.  DHR_LEX_RAW writes fp32 only.
 * Device memory only (mem_kind DHR_MEM_DEVICE).  The library allocates nothing: the caller passes dhr_lexical_proj_workspace(batch, n_tokens,
 * vocab, mode) bytes of device memory (at most 4 * batch * vocab + 256 * batch * n_tokens + 65536), aligned to 16 bytes.  The call ENQUEUES
 * on `stream` and returns without waiting.  No atomics: two calls on the same arguments are bit-identical.  NaN / inf are out of scope.
 * DHR_ERR_INVALID for NULL pointers, negative sizes, hidden_dim not a multiple of 8, unknown dtypes, host memory, a workspace that is too small,
 * a vocabulary that does not split into whole groups; DHR_ERR_UNSUPPORTED for fp32 operands, a bf16 bias next to fp16 operands (the fp16
 * kernels read fp32 or fp16, as before bf16 was taken) and fp16 raw reps. */
int64_t dhr_lexical_proj_workspace(int64_t batch, int32_t n_tokens, int32_t vocab, int32_t mode);
int dhr_lexical_proj_head(int32_t device, int32_t mem_kind, int32_t mode, const void* hidden, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                          int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight, int32_t vocab, int64_t ld_weight,
                          const void* bias, int32_t bias_dtype, const float* term_weights, int64_t ld_weights, const float* mask, int64_t ld_mask,
                          int32_t dims, int32_t remove_dims, void* out_value, int32_t out_value_dtype, int64_t ld_value, void* out_index,
                          int32_t index_dtype, int64_t ld_index, const void* cls, int32_t cls_dtype, int64_t ld_cls, int32_t cls_dim,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* The gated inner product of a training step and of the in-model reranker, with its gradient (tevatron/DHR/modeling.py:161-170, 212-226,
 * 250-285: listwise_gip_scores / pairwise_gip_scores, which repeat the passage batch once per query and keep [n_q, n_p, dims] tensors for
 * autograd).  q_value [n_q, dims] and p_value [n_p, dims] are densified values (value_dtype DHR_VAL_F16 / DHR_VAL_F32, both sides alike, row
 * strides: the [:, :dims] view of a record is read in place), q_index / p_index their group indices (index_dtype DHR_IDX_U8 / I8 / I16, both
 * sides alike).  group = 0 is the listwise form, every query against every passage; group = n > 0 the pairwise form, passage row b * n + j
 * belongs to query b and n_p == n_q * n.
 *   dhr_gip_scores           out[b][p] = sum_d (q_index[b][d] == p_index[p][d]) * q_value[b][d] * p_value[p][d], fp32 products and sums whatever
 *                            the input dtype; out is fp32 [n_q, n_p] listwise, [n_q, n] pairwise (row stride ld_out).
 *   dhr_gip_scores_backward  with grad_out = dL/d out (fp32, row stride ld_grad):
 *                            grad_q[b][d] = sum_p grad_out[b][p] * match * p_value[p][d],  grad_p[p][d] = sum_b grad_out[b][p] * match * q_value[b][d]
 *                            (pairwise: over the query's own block), fp32 [n_q, dims] / [n_p, dims]; either may be NULL and is then not computed.
 *   dhr_densify_backward     the gradient of dhr_densify (max sends it to the one index it returned): grad_lexical [batch, vocab] (grad_dtype
 *                            DHR_VAL_F32 / DHR_VAL_F16) gets grad_value[b][j] at column remove_dims + index[b][j] * dims + j and zero in every
 *                            other column, the remove_dims leading ones included: the whole row is written, in one pass.
 * Every sum runs in a fixed order: two calls on the same arguments are bit-identical.  Small listwise problems split dims over workgroups
 * and fold the partial sums in order; that needs dhr_gip_scores_workspace bytes of device memory from the caller (0: none needed; a NULL or
 * too small workspace runs unsplit, slower and with another summation order).  For device arrays the library allocates nothing and the calls
 * ENQUEUE on `stream` and return without waiting (a training step stays asynchronous); host arrays are staged through the device and are
 * complete on return.  DHR_ERR_INVALID for NULL / negative sizes / unknown dtypes, n_p != n_q * group, a vocabulary that does not split. */
int64_t dhr_gip_scores_workspace(int64_t n_q, int64_t n_p, int32_t dims, int32_t group);
int dhr_gip_scores(int32_t device, int32_t mem_kind, const void* q_value, int64_t ld_q_value, const void* q_index, int64_t ld_q_index, int64_t n_q,
                   const void* p_value, int64_t ld_p_value, const void* p_index, int64_t ld_p_index, int64_t n_p, int32_t dims, int32_t value_dtype,
                   int32_t index_dtype, int32_t group, float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes, void* stream);
int dhr_gip_scores_backward(int32_t device, int32_t mem_kind, const void* q_value, int64_t ld_q_value, const void* q_index, int64_t ld_q_index,
                            int64_t n_q, const void* p_value, int64_t ld_p_value, const void* p_index, int64_t ld_p_index, int64_t n_p, int32_t dims,
                            int32_t value_dtype, int32_t index_dtype, int32_t group, const float* grad_out, int64_t ld_grad, float* grad_q,
                            int64_t ld_grad_q, float* grad_p, int64_t ld_grad_p, void* stream);
int dhr_densify_backward(int32_t device, int32_t mem_kind, const float* grad_value, int64_t ld_grad_value, const void* index, int32_t index_dtype,
                         int64_t ld_index, int64_t batch, int32_t vocab, int32_t remove_dims, int32_t dims, void* grad_lexical, int32_t grad_dtype,
                         int64_t ld_grad, void* stream);

/* The lexical head of a TRAINING step, forward and backward (the same lines of modeling.py as dhr_lexical_head, with autograd on): device
 * arrays only (DHR_ERR_UNSUPPORTED for DHR_MEM_HOST: training tensors live on the device), enqueued on `stream` without waiting, nothing
 * allocated.  logits is the model's [batch, skip_tokens + n_tokens, vocab] tensor (value_dtype DHR_VAL_F16 / DHR_VAL_BF16 / DHR_VAL_F32, strides ld_batch /
 * ld_token / 1); the first skip_tokens tokens take no part (the reference drops token 0; pass the [:, 1:] view with skip_tokens = 0 for the
 * same numbers).  term_weights and mask are fp32 [batch, n_tokens].  n_tokens <= 32767.
 *   dhr_lexical_head_train_workspace  bytes of device memory the two calls share: (max, sum, w, mask) per token, written by the forward and
 *                                     read by the backward, then one float per token the backward writes (0 for invalid sizes).
 *   dhr_lexical_head_train            out_reps fp32 [batch, vocab], bit-identical to dhr_lexical_head(DHR_LEX_RAW); out_tokens int16
 *                                     [batch, vocab], the first token that attains the maximum (counted after the skipped ones).
 *   dhr_lexical_head_backward         with grad_reps = dL/d reps (fp32 [batch, vocab]), tokens and workspace as the forward left them, and
 *                                     A[b][t] = sum over {v : tokens[b][v] == t} of grad_reps[b][v] * p[b][t][v]:
 *                                     grad_weights[b][t] = mask * A (fp32 [batch, n_tokens]),
 *                                     grad_logits[b][t][v] = p * ([tokens[b][v] == t] * grad_reps[b][v] * w * mask - w * mask * A), in the
 *                                     logits' dtype (rounded once from fp32, to nearest even), the WHOLE [batch, skip_tokens + n_tokens, vocab] tensor (strides ld_grad_batch /
 *                                     ld_grad_token / 1): skipped and masked tokens are written as zeros.  Either output may be NULL.
 * p is recomputed from the logits, never stored.  A is accumulated in fp64 in a fixed order (no atomics): two calls on the same arguments are
 * bit-identical. */
int64_t dhr_lexical_head_train_workspace(int64_t batch, int32_t n_tokens);
int dhr_lexical_head_train(int32_t device, int32_t mem_kind, const void* logits, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                           int32_t skip_tokens, int32_t vocab, int64_t ld_batch, int64_t ld_token, const float* term_weights, int64_t ld_weights,
                           const float* mask, int64_t ld_mask, float* out_reps, int64_t ld_reps, int16_t* out_tokens, int64_t ld_tokens,
                           void* workspace, void* stream);
int dhr_lexical_head_backward(int32_t device, int32_t mem_kind, const void* logits, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                              int32_t skip_tokens, int32_t vocab, int64_t ld_batch, int64_t ld_token, const float* grad_reps, int64_t ld_grad_reps,
                              const int16_t* tokens, int64_t ld_tokens, void* workspace, void* grad_logits, int64_t ld_grad_batch,
                              int64_t ld_grad_token, float* grad_weights, int64_t ld_grad_weights, void* stream);

/* dhr_lexical_head_train / dhr_lexical_head_backward with the vocabulary projection fused in, as dhr_lexical_proj_head fuses it for encoding:
 * the op starts from the projector's input and returns the gradients of hidden, weight, bias and the term weights; the logits
 *   x[r][v] = hidden[r] . weight[v] + bias[v]      (fp32 products and sums)
 * and their gradient exist only in registers and LDS, forward and backward, and masked tokens are never multiplied.  hidden is the model's
 * [batch, skip_tokens + n_tokens, hidden_dim] tensor (value_dtype DHR_VAL_F16 or DHR_VAL_BF16, strides ld_batch / ld_token / 1, hidden_dim a
 * multiple of 8 up to 1024); the first skip_tokens tokens take no part.  weight is [vocab, hidden_dim] of the same dtype (row stride ld_weight),
 * bias [vocab] (DHR_VAL_F32 / DHR_VAL_F16; DHR_VAL_BF16 with bf16 operands) or NULL, term_weights and mask fp32 [batch, n_tokens], n_tokens <= 32767.
 *   dhr_lexical_proj_train_workspace  bytes of device memory the two calls share, aligned to 16 bytes (0 for invalid sizes; at most
 *                                     256 * batch * n_tokens + 65536 * hidden_dim + 65536): the list of unmasked token rows and their softmax
 *                                     statistics, written by the forward and read by the backward, and what the backward needs itself.
 *   dhr_lexical_proj_train            out_reps fp32 [batch, vocab], bit-identical to dhr_lexical_proj_head(DHR_LEX_RAW); out_tokens int16
 *                                     [batch, vocab], the first token that attains the maximum (counted after the skipped ones; a masked token
 *                                     that wins is named like any other); out_pwin fp32 [batch, vocab], the softmax value of that token (0 for a
 *                                     masked one).
 *   dhr_lexical_proj_backward         with grad_reps = dL/d reps (fp32 [batch, vocab]), the forward's arguments, tokens, pwin and workspace as it
 *                                     left them, A[r] = sum over {v : tokens[b][v] == t} of grad_reps[b][v] * pwin[b][v] and
 *                                     dx[r][v] = p * ([tokens[b][v] == t] * grad_reps[b][v] * w * mask - w * mask * A):
 *                                     grad_term_weights[b][t] = mask * A                 fp32 [batch, n_tokens]
 *                                     grad_hidden[r][k] = sum_v dx[r][v] weight[v][k]    the WHOLE [batch, skip_tokens + n_tokens, hidden_dim]
 *                                                         tensor (strides ld_grad_batch / ld_grad_token / 1): skipped and masked tokens are zeros
 *                                     grad_weight[v][k] = sum_r dx[r][v] hidden[r][k]    [vocab, hidden_dim], row stride ld_grad_weight
 *                                     grad_bias[v]      = sum_r dx[r][v]
 *                                     each DHR_VAL_F16 or DHR_VAL_F32, or with bf16 operands DHR_VAL_BF16 (its *_dtype), rounded once from fp32
 *                                     accumulators.  Any output may be NULL
 *                                     and is then not computed (no grad_weight and no grad_bias: the weight-gradient pass does not run; no
 *                                     grad_hidden: nor does the other GEMM pass); all NULL: DHR_OK, nothing is launched.
 * dx is rounded once to the dtype of hidden / weight, as the operand of the second product.  Device memory only (DHR_ERR_UNSUPPORTED for DHR_MEM_HOST), nothing is
 * allocated, the calls ENQUEUE on `stream` and return without waiting.  No atomics, every sum in a fixed order: two calls on the same
 * arguments are bit-identical.  DHR_ERR_INVALID for NULL pointers, bad sizes / strides / dtypes, hidden_dim not a multiple of 8, a workspace
 * that is too small or not aligned; DHR_ERR_UNSUPPORTED for fp32 operands, a bf16 bias or a bf16 gradient next to fp16 operands (the
 * fp16 kernels read and write fp32 or fp16, as before bf16 was taken), hidden_dim > 1024, n_tokens > 32767. */
int64_t dhr_lexical_proj_train_workspace(int64_t batch, int32_t n_tokens, int32_t vocab, int32_t hidden_dim);
int dhr_lexical_proj_train(int32_t device, int32_t mem_kind, const void* hidden, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                           int32_t skip_tokens, int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight, int32_t vocab,
                           int64_t ld_weight, const void* bias, int32_t bias_dtype, const float* term_weights, int64_t ld_weights,
                           const float* mask, int64_t ld_mask, float* out_reps, int64_t ld_reps, int16_t* out_tokens, int64_t ld_tokens,
                           float* out_pwin, int64_t ld_pwin, void* workspace, int64_t workspace_bytes, void* stream);
int dhr_lexical_proj_backward(int32_t device, int32_t mem_kind, const void* hidden, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                              int32_t skip_tokens, int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight, int32_t vocab,
                              int64_t ld_weight, const void* bias, int32_t bias_dtype, const float* term_weights, int64_t ld_weights,
                              const float* mask, int64_t ld_mask, const float* grad_reps, int64_t ld_grad_reps, const int16_t* tokens,
                              int64_t ld_tokens, const float* pwin, int64_t ld_pwin, void* workspace, int64_t workspace_bytes, void* grad_hidden,
                              int32_t grad_hidden_dtype, int64_t ld_grad_batch, int64_t ld_grad_token, void* grad_weight,
                              int32_t grad_weight_dtype, int64_t ld_grad_weight, void* grad_bias, int32_t grad_bias_dtype,
                              float* grad_term_weights, int64_t ld_grad_term_weights, void* stream);

/* The Aggretriever TRAINING ops that follow the encoder, forward and backward: aggregate under autograd (tevatron/Aggretriever/utils.py:16-44 at
 * modeling.py:173-174) and the head without the MLM logits (--skip_mlm, modeling.py:279-284, 311-316), which the reference computes by
 * scattering the term weights into a zero [batch, L, 30522] tensor and taking the max over tokens.  Both are selections -- every output is an
 * input value, its negation or zero -- so parity with the reference is equality.  Device arrays only (DHR_ERR_UNSUPPORTED for DHR_MEM_HOST),
 * enqueued on `stream` without waiting, nothing allocated.
 *   dhr_aggregate_train            dhr_aggregate (the same arguments, the same bits in `out`) which also writes route int16 [batch, dims] (row
 *                                  stride ld_route; NULL: not written).  With groups of W columns from remove_dims (W = 2 * dims for full != 0,
 *                                  else dims; a negative remove_dims pads zero columns at the end) and m[b][c] = max_g lexical[b][remove + g * W + c]
 *                                  at its FIRST group g[b][c]:
 *                                    full == 0:  out[b][j] = m[b][j],  route[b][j] = g[b][j]
 *                                    full != 0:  pos = m[b][2j], neg = m[b][2j + 1], s = (pos > neg ? 0 : 1),
 *                                                out[b][j] = pos * (pos > neg) - neg * (pos <= neg),  route[b][j] = 2 * g[b][2j + s] + s
 *                                  A winner may lie in the zero padding.
 *   dhr_aggregate_backward         with grad_out = dL/d out ([batch, dims], grad_dtype DHR_VAL_F16 / DHR_VAL_F32) and route as the forward left
 *                                  it, grad_lexical [batch, vocab] (the same dtype) gets, in one pass over the whole row, without atomics,
 *                                    full == 0:  grad_out[b][j] at column remove + route[b][j] * dims + j
 *                                    full != 0:  (s == 0 ? +1 : -1) * grad_out[b][j] at column remove + (route[b][j] >> 1) * 2 * dims + 2j + s,  s = route[b][j] & 1
 *                                  and zero in every other column, the removed leading ones included.  Nothing is written for a winner in
 *                                  the padding.
 *   dhr_term_weight_head           input_ids is the model's [batch, skip_tokens + n_tokens] ids (id_bytes 4: int32, 8: int64; row stride ld_ids),
 *                                  the first skip_tokens take no part; term_weights is [batch, n_tokens] (value_dtype DHR_VAL_F16 / DHR_VAL_F32).
 *                                    out_reps[b][v]   = max(0, max over {t : ids[b][skip + t] == v} of w[b][t])                 fp32 [batch, vocab]
 *                                    out_tokens[b][v] = the first t that attains a strictly positive maximum, -1 where the zero wins  int16
 *                                  Every column of both rows is written.  There is no mask: a padding token deposits its weight at its own id,
 *                                  as in the reference.  Ids outside [0, vocab) are ignored and never used as an index.  The result does not
 *                                  depend on the order in which repeated ids are met: two calls are bit-identical.
 *   dhr_term_weight_head_backward  with grad_reps = dL/d reps (fp32 [batch, vocab]) and tokens as the forward left them:
 *                                    grad_weights[b][t] = (tokens[b][v] == t ? grad_reps[b][v] : 0),  v = ids[b][skip + t];  0 for an id outside
 *                                  the vocabulary.  Every entry of [batch, n_tokens] (grad_dtype, row stride ld_grad_weights) is written.
 * DHR_ERR_INVALID for NULL / non-positive sizes / unknown dtypes / strides shorter than the row / a vocabulary that does not split into whole
 * groups; DHR_ERR_UNSUPPORTED for more than 16383 groups (2 * g + 1 must fit the route) or more than 32767 tokens. */
int dhr_aggregate_train(int32_t device, int32_t mem_kind, const void* lexical, int32_t value_dtype, int64_t ld, int64_t batch, int32_t vocab,
                        int32_t dims, int32_t remove_dims, int32_t full, void* out, int32_t out_dtype, int64_t ld_out, int16_t* route,
                        int64_t ld_route, void* stream);
int dhr_aggregate_backward(int32_t device, int32_t mem_kind, const void* grad_out, int32_t grad_dtype, int64_t ld_grad_out, const int16_t* route,
                           int64_t ld_route, int64_t batch, int32_t vocab, int32_t dims, int32_t remove_dims, int32_t full, void* grad_lexical,
                           int64_t ld_grad, void* stream);
int dhr_term_weight_head(int32_t device, int32_t mem_kind, const void* input_ids, int32_t id_bytes, int64_t ld_ids, const void* term_weights,
                         int32_t value_dtype, int64_t ld_weights, int64_t batch, int32_t n_tokens, int32_t skip_tokens, int32_t vocab,
                         float* out_reps, int64_t ld_reps, int16_t* out_tokens, int64_t ld_tokens, void* stream);
int dhr_term_weight_head_backward(int32_t device, int32_t mem_kind, const void* input_ids, int32_t id_bytes, int64_t ld_ids, int64_t batch,
                                  int32_t n_tokens, int32_t skip_tokens, int32_t vocab, const float* grad_reps, int64_t ld_grad_reps,
                                  const int16_t* tokens, int64_t ld_tokens, void* grad_weights, int32_t grad_dtype, int64_t ld_grad_weights,
                                  void* stream);

/* Late-interaction (MaxSim) scores with their gradient (tevatron/ColBERT/modeling.py:188-190, 204-219: listwise_maxsim / pairwise_maxsim and
 * the paired evaluation branch, which build the [A, B, Lq, Lp] similarity tensor and keep it for autograd).  q is [A, Lq, D], p is [B, Lp, D]
 * (value_dtype DHR_VAL_F16 / DHR_VAL_F32, both sides alike; strides ld_*_batch / ld_*_tok / 1 in elements: a [:, 1:] view is read in place).
 * group = 0: every pair, cols = B; group = n > 0: passage row a * n + j belongs to query a, B == A * n, cols = n.  There is no mask: padded
 * tokens are zero vectors and take part with similarity 0, as in the reference.
 *   forward   out[a][col] = sum_i max_j <q[a][i], p[b][j]>, fp32 products and sums whatever the input dtype (fp32 inputs are never rounded
 *             to fp16), fp32 [A, cols] (row stride ld_out).  arg, if not NULL, receives int16 [A][cols][Lq] (packed): the FIRST j that
 *             attains the maximum.
 *   backward  with grad_out = dL/d out (fp32, row stride ld_grad) and arg as the forward left it:
 *             dq[a][i] = sum_b grad_out[a][b] * p[b][arg[a][b][i]],   dp[b][j] = sum_a grad_out[a][b] * sum over {i : arg[a][b][i] == j} of q[a][i]
 *             over the scored pairs, packed [A, Lq, D] / [B, Lp, D] in grad_dtype (fp32 sums, rounded once for DHR_VAL_F16); every row is
 *             written, zeros where nothing was routed.  Either may be NULL and is then not computed.
 * Every sum runs in a fixed order that depends on the shape alone (no atomics): two calls are bit-identical, and the score of a pair does
 * not depend on which other pairs are scored.  For device arrays the library allocates nothing and the calls ENQUEUE on `stream` and return
 * without waiting; host arrays are staged through the device and are complete on return.  DHR_ERR_INVALID for NULL / non-positive sizes /
 * unknown dtypes / strides shorter than D / B != A * group; DHR_ERR_UNSUPPORTED beyond D <= 1024, Lp <= 32767, 131072 rows on a side. */
int dhr_maxsim_scores(int32_t device, int32_t mem_kind, const void* q, int64_t ld_q_tok, int64_t ld_q_batch, int64_t A, int64_t Lq, const void* p,
                      int64_t ld_p_tok, int64_t ld_p_batch, int64_t B, int64_t Lp, int32_t D, int32_t value_dtype, int32_t group, float* out,
                      int64_t ld_out, int16_t* arg, void* stream);
int dhr_maxsim_scores_backward(int32_t device, int32_t mem_kind, const void* q, int64_t ld_q_tok, int64_t ld_q_batch, int64_t A, int64_t Lq,
                               const void* p, int64_t ld_p_tok, int64_t ld_p_batch, int64_t B, int64_t Lp, int32_t D, int32_t value_dtype,
                               int32_t group, const int16_t* arg, const float* grad_out, int64_t ld_grad, void* dq, void* dp, int32_t grad_dtype,
                               void* stream);

/* The loss of a training step with its gradient with respect to the score matrices (the tail of tevatron/DHR/modeling.py:170-197,
 * Aggretriever/modeling.py:184-213, ColBERT/modeling.py:146-160, Dense/modeling.py:134-140).  lexical, semantic (may be NULL) and teacher (may be
 * NULL) are [rows, cols] matrices, each DHR_VAL_F16 or DHR_VAL_F32 on its own, with row strides ld_* in elements (a [:, 1:] view is read in
 * place).  fused = lexical + lamb * semantic (lexical alone without semantic).  With a teacher the target of term k is
 * P_k = softmax(teacher * temperature * teacher_split[k]); without one it is the one-hot at column r * label_stride of row r (the reference's
 * hard_label_scores; CrossEntropyLoss(mean) is the same quantity).  With KL_r(s, P) = sum_c P[r][c] (log P[r][c] - log_softmax(s)[r][c]), a zero
 * P entry contributing exactly 0 as in KLDivLoss:
 *   loss = (1 / rows) sum_r [ weights[0] KL_r(fused, P_0) + weights[1] KL_r(semantic, P_1) + weights[2] KL_r(lexical, P_2) ]
 * weights and teacher_split are HOST arrays of 3 floats whatever mem_kind (teacher_split is read only with a teacher); a term whose weight is 0
 * is not computed.  Outputs (mem_kind memory): loss, one fp32; scores_out (may be NULL), fp32 [rows, cols] holding fused; grad_lexical and
 * grad_semantic (either may be NULL), dloss / dlexical and dloss / dsemantic in the dtype of the input each belongs to:
 * weights[k] / rows * (softmax(s) - P_k) per term, the fused term reaching lexical with factor 1 and semantic with factor lamb.
 * exp and log are fp32 with the row maximum subtracted first; the inputs must be finite.  No atomics: every sum has a fixed order and two calls
 * on the same arguments are bit-identical.  Device arrays need dhr_train_loss_workspace(rows) bytes of device workspace; the library then
 * allocates nothing, ENQUEUES two kernels on `stream` and returns without waiting.  Host arrays are staged through the device and are complete on
 * return.  rows == 0 or cols == 0: loss = 0 and nothing else is touched.  DHR_ERR_INVALID for a NULL lexical / loss / weights, negative sizes,
 * unknown dtypes, a stride shorter than cols, temperature <= 0 or a teacher_split[k] <= 0 with a teacher (the three targets share the
 * teacher's row maximum, which needs positive scales), a label column (rows - 1) * label_stride >= cols or label_stride < 0 without one,
 * weights[1] != 0 or a grad_semantic without semantic, a missing or short workspace; DHR_ERR_UNSUPPORTED from 2^31 rows or beyond 2^30 columns. */
int64_t dhr_train_loss_workspace(int64_t rows);
int dhr_train_loss(int32_t device, int32_t mem_kind, const void* lexical, int32_t lexical_dtype, int64_t ld_lexical, const void* semantic,
                   int32_t semantic_dtype, int64_t ld_semantic, const void* teacher, int32_t teacher_dtype, int64_t ld_teacher, int64_t rows,
                   int64_t cols, int64_t label_stride, float lamb, float temperature, const float* weights, const float* teacher_split, float* loss,
                   float* scores_out, int64_t ld_scores, void* grad_lexical, int64_t ld_grad_lexical, void* grad_semantic,
                   int64_t ld_grad_semantic, void* workspace, int64_t workspace_bytes, void* stream);

/* Product quantiser for the first stage of --PQIP.  The reference calls faiss
 * IndexPQ(d, M = 64, nbits = 8, METRIC_INNER_PRODUCT) (retrieval/quantize_index.py:27-37, gip_retrieval.py:167-231); faiss is not
 * part of the reference tree, so these restate its published algorithm (per-subspace Lloyd k-means, nearest-centroid codes, ADC
 * inner-product scores) -- codebooks differ from faiss's (different initialisation and sub-sampling): PARITY UNPINNED, judged
 * by recall against the exact search.  All arrays live in mem_kind memory; values are the fp16 rows of an index record
 * (row stride ld, d = M * dsub columns used), codebooks fp32 [M][256][dsub], codes uint8 [n][M].
 *   dhr_pq_train : k-means on at most max_points evenly spaced rows, `iters` Lloyd iterations; out_error (host, may be NULL)
 *                  receives the mean squared quantisation error per training row after the last assignment.
 *   dhr_pq_encode: nearest centroid per subspace (first minimum).
 *   dhr_pq_decode: fp16 reconstruction [n][ld_out]; an exact inner-product search over it (dhr_index_create with index = NULL,
 *                  then dhr_search) returns exactly the ADC ranking, on the matrix cores.
 * All three run on `stream` and wait for it: their outputs are complete on return. */
int dhr_pq_train(int32_t device, int32_t mem_kind, const void* values_f16, int64_t ld, int64_t n, int32_t d, int32_t M, int32_t iters,
                 int64_t max_points, float* codebooks, double* out_error, void* stream);
int dhr_pq_encode(int32_t device, int32_t mem_kind, const void* values_f16, int64_t ld, int64_t n, int32_t d, int32_t M,
                  const float* codebooks, uint8_t* codes, void* stream);
int dhr_pq_decode(int32_t device, int32_t mem_kind, const uint8_t* codes, int64_t n, int32_t d, int32_t M, const float* codebooks,
                  void* out_values_f16, int64_t ld_out, void* stream);
/* The same three with `--n_bits` (quantize_index.py:22,29: faiss.IndexPQ(d, M, nbits)): 2^nbits centroids per sub-quantiser, 1 <= nbits <= 8,
 * codebooks [M][2^nbits][d / M]; codes stay one byte per sub-quantiser on the device and in these calls (faiss' bit-packed rows are
 * written / read by the index file code, dhr_amd/retrieval/quantize_index.py).  The functions above are nbits = 8. */
int dhr_pq_train_nbits(int32_t device, int32_t mem_kind, const void* values_f16, int64_t ld, int64_t n, int32_t d, int32_t M, int32_t nbits,
                       int32_t iters, int64_t max_points, float* codebooks, double* out_error, void* stream);
int dhr_pq_encode_nbits(int32_t device, int32_t mem_kind, const void* values_f16, int64_t ld, int64_t n, int32_t d, int32_t M, int32_t nbits,
                        const float* codebooks, uint8_t* codes, void* stream);
int dhr_pq_decode_nbits(int32_t device, int32_t mem_kind, const uint8_t* codes, int64_t n, int32_t d, int32_t M, int32_t nbits,
                        const float* codebooks, void* out_values_f16, int64_t ld_out, void* stream);

/* The TREC run file (gip_retrieval.py:333-342): for every query, in order, one line "qid Q0 docid rank score run_name" per result row,
 * rank = 1-based position in the query's list (rows < 0 are padding of a short list and take no rank), lines whose docid equals the
 * query id skipped (their rank stays unused, as in the reference), score printed as Python prints float(score): the shortest digit
 * string that round-trips the DOUBLE, fixed notation for 1e-4 <= |x| < 1e16.  Ids are handed over as one byte blob each with
 * n + 1 offsets (id i = blob[off[i], off[i+1] - id_sep_bytes): id_sep_bytes = 1 for ids joined with one separator byte each); rows are [n_queries][k], row - row_base indexes the docid list; formatted on
 * n_threads host threads (0 = all, at most 64), written in query order.  dhr_format_float: the score formatting alone (returns the
 * length).  Host code only -- no device is touched. */
int dhr_write_trec(const char* path, int32_t append, int64_t n_queries, int64_t k, const char* qid_blob, const int64_t* qid_off,
                   const char* docid_blob, const int64_t* docid_off, int64_t n_docs, const int64_t* rows, int64_t row_base,
                   const float* scores, const char* run_name, int32_t id_sep_bytes, int32_t n_threads, int64_t* lines_out);
int dhr_format_float(double x, char* out, int32_t cap);

int dhr_get_stats(const dhr_index* index, dhr_search_stats* out);

/* Debug/test hook: the bound-GEMM scores U[q][row] for rows [row_lo,row_hi) of the shard, written
 * to a DEVICE buffer [n_queries, row_hi-row_lo] fp32 (U >= exact score; equal for dense-only). */
int dhr_debug_bound_scores(dhr_index* index, const dhr_query_batch* queries, int64_t row_lo, int64_t row_hi,
                           float* out_dev, void* stream);

/* Debug/test hook: the filter margins of a query batch (HOST buffer [n_queries] fp32): the bound GEMM guarantees
 * U[q][row] >= exact score - margin[q] for every row, which is what lets the filter drop rows without losing a top-k row. */
int dhr_debug_query_margins(dhr_index* index, const dhr_query_batch* queries, float* out_host, void* stream);

/* Debug/test hook: the bounds of the filter levels behind the bound GEMM, pair by pair.  Runs for rows [row_lo,row_hi) what one phase of a
 * search runs -- the bound GEMM into the candidate lists, then the refine level on those lists -- and scatters both lists into DEVICE buffers
 * [n_queries, row_hi-row_lo] fp32: out_u_dev the bound U of every row the filter listed, out_u2_dev the refined bound U2 of every row the
 * refine level kept, NaN where a row is not in that list.  tau_host: HOST [n_queries] exact-score thresholds -- both levels compare with
 * thr = tau - margin, as a search does -- or null: -inf, every row passes both levels.  flat: 0 = the refine kernel on a (block, query) grid,
 * 1 = on the flat grid of the controller that only enqueues, n > 1 = on a flat grid of n workgroups.  out_thr_host: HOST [n_queries], the thr
 * the levels compared with (may be null); out_unit_host: HOST [n_queries], the score units of one gated operand product of an int8 gated image
 * (U and U2 of such an index differ by integer multiples of it plus real-valued products), zeros otherwise (may be null).  DHR_ERR_UNSUPPORTED where the batch has no refine level on this index (no gated columns and no
 * residual image; a plain inner-product batch on an fp16 gated image), DHR_ERR_INVALID where the tiles of the row range hold more rows
 * than a candidate list (32 768 by default, DHR_PARAM_CAND_CAP).  Overwrites the workspace of a staged search left open on the handle. */
int dhr_debug_refine_bounds(dhr_index* index, const dhr_query_batch* queries, int64_t row_lo, int64_t row_hi, const float* tau_host,
                            int32_t flat, float* out_u_dev, float* out_u2_dev, float* out_thr_host, float* out_unit_host, void* stream);

/* Debug/test hook: one call of the running top-k merge that ends every phase of every search (dhr_search, the staged and sharded calls,
 * dhr_search_rerank, dhr_search_excluding, dhr_pq_search), through the searches' own launcher: kp <= 1024 and kp <= 4096 run the two LDS
 * kernels, kp <= 16384 the in-place kernel, larger kp the global-memory sort.  No index handle; every array is DEVICE memory of `device`.
 *   topk_keys_dev  [n_queries][kp] u64, in/out: the running lists, sorted descending.  A key is (order-preserving image of the fp32 score) << 32 |
 *                  (0xFFFFFFFF - row): the image flips the sign bit of a non-negative score and every bit of a negative one, and both zeros
 *                  map to 0x80000000, so keys order by score descending, then row ascending.  0 is an empty slot.  Keys must be unique across
 *                  a query's list and its input.  k_keep' = k_keep ? k_keep : k slots are kept; the global-memory path reads the slots behind
 *                  them as part of the list, so they come in as zeros or as an earlier call left them.
 *   in_keys_dev    [n_queries][ld_keys] u64: query q brings its first min(cnt_dev[q], cap) keys, or its first count_all where cnt_dev is null.
 *   kps            the prefix of the list the LDS kernels hold (a power of two, k_keep' <= kps <= kp); sort_n: their LDS budget in keys
 *                  (2 kp in the searches, 4 kp in dhr_pq_search; ignored for kp > 4096).
 *   margin_dev, tau_dev (in/out), thr_dev (out)   [n_queries] fp32.
 * After the call slots [0, k_keep') hold the k_keep' greatest keys of list and input, descending, zeros behind the last; tau is the score of slot
 * k - 1, or -inf while that slot is empty, on every path; with monotone != 0 it is max(old tau, that); thr = tau - margin in fp32.  Slots
 * [k_keep', kp) are defined per path and never hold a key greater than slot k_keep' - 1: the LDS kernels zero [k_keep', kps) and leave [kps, kp)
 * as it was, the in-place kernel leaves [k_keep', kp) as it was, the global-memory path keeps the next-best keys there (no reader of a search
 * looks past slot k - 1).  DHR_ERR_INVALID, before the device is touched, for: a null pointer (cnt_dev may be null); n_queries <= 0; kp not a
 * power of two in [64, 2^20]; kps not a power of two in [64, kp]; not 1 <= k <= k_keep' <= kps; for kp <= 4096, sort_n - kps < 64 or
 * sort_n * 8 + 16 bytes beyond the 160 KiB of LDS a workgroup may take; for kp > 16384, n_queries > 65535; ld_keys < 0; count_all > ld_keys
 * without cnt_dev; cap > ld_keys.  A failure of the global-memory path (more than 2^31 - 1 keys in one sort) returns DHR_ERR_HIP.  Synchronises
 * the stream.  (tests/test_select_merge.py) */
int dhr_debug_select_merge(int32_t device, int32_t n_queries, int32_t k, int32_t k_keep, int32_t kp, int32_t kps, int32_t sort_n, int32_t monotone,
                           uint64_t* topk_keys_dev, const uint64_t* in_keys_dev, int64_t ld_keys, const uint32_t* cnt_dev, uint32_t count_all,
                           uint32_t cap, const float* margin_dev, float* tau_dev, float* thr_dev, void* stream);

/* Debug/test hook: how the main pass of the latest dhr_search on this handle seated its batch (DHR_PARAM_SEAT_QUERIES).  Returns 1 and fills the
 * HOST arrays ([n_slots] each, n_slots = that batch's query count rounded up to 256; any may be null) when the pass ran seated: slot -> query,
 * query -> slot, the per-query bound-list lengths of the sampled run the order was taken from, the slot-ordered threshold mirror and the
 * thresholds as the pass left them.  Returns 0 and copies nothing when every query sat where the caller put it; negative: a dhr_status. */
int dhr_debug_query_seating(dhr_index* index, int32_t n_slots, int32_t* slot_q, int32_t* q_slot, uint32_t* lengths, float* thr_seat, float* thr_hat);

/* Test hook (host code only, no device needed): the corpus tile that position `seq` of a bound-GEMM launch maps to, computed with
 * the kernels' division-free arithmetic (out[0]) and with plain integer division (out[1]); the two must agree for every input. */
void dhr_debug_seq_to_tile(int64_t seq, int32_t map_mode, int32_t period, int64_t head, int64_t perm_mul, int64_t perm_n, int64_t out[2]);
/* Test hook of the exception barrier: arms a failure of the library's n-th HOST allocation from now (operator new inside the library only --
 * the process' allocator is not interposed; 0 disarms; the environment variable DHR_TEST_FAIL_ALLOC=n arms it at load time).  The entry
 * point in which it fires returns DHR_ERR_NOMEM.  Returns the number of host allocations the library has made so far. */
int64_t dhr_debug_fail_alloc(int64_t n);
/* Test hook: how many queries the calling thread's last dhr_search_sharded* call redid with local thresholds (its repair path: a
 * correct result either way, but each repaired query costs the step an extra pass over its query tile). */
int32_t dhr_debug_sharded_repairs(void);

/* Kernel-tuning hook: the bound GEMM alone over the whole shard with the filter closed; average
 * milliseconds per launch over `iters` launches and the flops one launch issues (padded sizes). */
int dhr_debug_gemm_time(dhr_index* index, const dhr_query_batch* queries, int32_t iters, double* ms_out,
                        double* flops_out, void* stream);

/* ---- Product-quantised first stage of --PQIP as an ADC scan.  Replaces
 * faiss.read_index(...) + IndexPQ.search(queries, agip_topk) (retrieval/gip_retrieval.py:170,202; built by
 * retrieval/quantize_index.py:27-37 as IndexPQ(d, M, nbits, METRIC_INNER_PRODUCT)).  faiss is not part of the reference tree: the
 * algorithm is restated from its publication, PARITY WITH FAISS IS UNPINNED.  The handle keeps the codes (ONE BYTE per
 * sub-quantiser and row: 64 B per row at M = 64) and the codebooks ([M][2^nbits][d/M] fp32, faiss' centroid order) on the
 * device; a search builds per-query lookup tables <q_m, c_m[j]> and scans the codes (HBM / LDS-gather bound), fused with the
 * running top-k threshold filter.  score(q, x) = sum_m LUT[q][m][code_m(x)] in fp32, m ascending.
 *   codes     [n][M] uint8, one code per byte (unpack files with nbits < 8 first)
 *   queries   values only ([n_queries][d], fp16 or fp32; index arrays are ignored: the first stage is ungated)
 *   dhr_pq_search    -> [n_queries][k] (score desc, row asc on exact ties; global rows; (-inf, -1) beyond the corpus), k <= 1048576 (above 16384 the global-memory merge)
 *   dhr_pq_adc_scores-> raw scores of rows [row_lo, row_hi), device memory [n_queries][row_hi - row_lo] (tests)
 *   dhr_pq_last_scan -> duration (ms, hipEvents) and code bytes read by the scan kernel launches of the last search */
typedef struct dhr_pq dhr_pq; /* opaque */
int dhr_pq_create(int32_t device, int32_t mem_kind, int64_t n, int32_t d, int32_t M, int32_t nbits, const float* codebooks,
                  const uint8_t* codes, int64_t row_offset, dhr_pq** out);
void dhr_pq_destroy(dhr_pq* pq);
int64_t dhr_pq_device_bytes(const dhr_pq* pq);
int dhr_pq_search(dhr_pq* pq, const dhr_query_batch* queries, int32_t k, float* out_scores, int64_t* out_rows, int32_t out_mem_kind,
                  void* stream);
int dhr_pq_adc_scores(dhr_pq* pq, const dhr_query_batch* queries, int64_t row_lo, int64_t row_hi, float* out_dev, void* stream);
int dhr_pq_last_scan(const dhr_pq* pq, double* ms, double* code_bytes);

/* ---- Row-sharded search: replaces the reference's --total_shrad / --shrad runs plus
 * retrieval/merge.result.py:22-42.  The corpus rows are split like gip_retrieval.py:292-306 (per = N // S, the last shard takes
 * the remainder; dhr_index_desc.row_offset = the shard's first global row), queries are replicated, and the result is the global
 * [n_queries, k] (scores, rows) -- bit-identical to the unsharded dhr_search of the whole corpus -- on EVERY rank.
 *
 * dhr_comm: an RCCL communicator (librccl is linked directly; all-gathers run on the caller's stream over xGMI).
 *   dhr_comm_unique_id   rank 0: a 128-byte id to hand to every rank (any out-of-band channel)
 *   dhr_comm_create      every rank: ncclCommInitRank on `device` (collective over the ranks)
 *   dhr_comm_wrap        adopt an existing ncclComm_t (not destroyed by dhr_comm_destroy)
 * dhr_search_sharded: one process per GPU; collective -- every rank calls it with the same batch and k.  Sequence: sampled
 *   pass -> all-gather of [Q, r] sample scores -> common per-query thresholds -> main pass -> all-gather of the per-query
 *   counts -> all-gather of the list prefixes [Q, kk] -> rank merge of the sorted lists; one host read at the end (number of
 *   queries whose lists were incomplete; those are redone with local thresholds).
 * dhr_search_sharded_local: one process, several shard handles (on one or more devices), no communicator -- the same control
 *   flow with the gathers done by device copies.  A device-resident query batch must be readable from every shard's device
 *   (same device, or peer access); host batches always work. */
typedef struct dhr_comm dhr_comm; /* opaque */
int dhr_comm_unique_id(void* out128, int32_t out_bytes);
int dhr_comm_create(const void* unique_id128, int32_t world, int32_t rank, int32_t device, dhr_comm** out);
int dhr_comm_wrap(void* nccl_comm, int32_t world, int32_t rank, int32_t device, dhr_comm** out);
/* A communicator whose all-gather is done by the CALLER over any transport (torch.distributed on gloo, MPI, pipes ...):
 *   allgather(user, send, recv, bytes) gathers `bytes` from every rank into recv = [world][bytes], rank order; HOST buffers
 *   (the library stages device blocks through pinned memory around the call); returns 0 on success.  Collective: every rank
 *   calls it the same number of times with the same sizes.  dhr_search_sharded then runs the same control flow as over RCCL.
 * Used where RCCL is not available between the ranks (several ranks on one GPU, CPU-only process groups). */
typedef int (*dhr_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes);
int dhr_comm_create_callback(int32_t world, int32_t rank, int32_t device, dhr_allgather_fn allgather, void* user, dhr_comm** out);
void dhr_comm_destroy(dhr_comm* comm);
/* What the communicator really is, asked of the transport itself (a scaling record can then show that RCCL spanned N ranks):
 *   DHR_COMM_TRANSPORT 0 = RCCL, 1 = caller-supplied host transport;  DHR_COMM_WORLD / DHR_COMM_RANK / DHR_COMM_DEVICE: for an RCCL
 *   communicator ncclCommCount / ncclCommUserRank / ncclCommCuDevice of the ncclComm_t, else the values given at creation.
 * Returns the value, or a negative status. */
enum { DHR_COMM_TRANSPORT = 0, DHR_COMM_WORLD = 1, DHR_COMM_RANK = 2, DHR_COMM_DEVICE = 3 };
int dhr_comm_info(const dhr_comm* comm, int32_t what);
/* Way out of a bring-up that hangs (a peer never reached ncclCommInitRank / a collective): ncclCommAbort instead of ncclCommDestroy --
 * may be called from another host thread than the one blocked in the collective.  The handle is only marked dead (every later call on it
 * fails with DHR_ERR_INVALID): the thread that was blocked unwinds through code that still uses it, so the caller frees it with
 * dhr_comm_destroy once that thread has returned. */
void dhr_comm_abort(dhr_comm* comm);
/* The sharded control flow over a shard the CALLER implements in host memory (no device is touched): test / bring-up hook.  The
 * callbacks mirror the staged C ABI: sample_rank / union_rank (dhr_search_sample_rank with DHR_PARAM_SAMPLE_SHARE = share /
 * dhr_search_union_rank), begin (writes [n_queries, sample_rank] best sample scores, best first), finish (tau [n_queries] ->
 * [n_queries, k] sorted lists with (-inf, -1) tails + per-query counts of rows >= tau, -1 = incomplete), search (plain top-k).
 * All return 0 on success; all arrays are host memory; rows are global.  The query batch must be a host batch. */
typedef struct dhr_host_shard {
  uint32_t struct_size; /* sizeof(dhr_host_shard) as the CALLER compiled it: dhr_search_sharded_host rejects any other value (the struct has grown
                           between versions; a shorter caller struct would otherwise be read past its end) */
  uint32_t reserved;
  void* user;
  int32_t (*sample_rank)(void* user, int32_t k, int32_t share);
  int32_t (*union_rank)(void* user, int32_t k);
  int32_t (*begin)(void* user, const dhr_query_batch* queries, int32_t k, int32_t share, float* out_sample);
  int32_t (*finish)(void* user, const float* tau, float* out_scores, int64_t* out_rows, int32_t* out_count);
  int32_t (*search)(void* user, const dhr_query_batch* queries, int32_t k, float* out_scores, int64_t* out_rows);
  /* optional (both NULL: no second agreement): dhr_search_mid_ranks / dhr_search_mid of the shard */
  int32_t (*mid_ranks)(void* user, int32_t k, int32_t share, int32_t* out_local, int32_t* out_union);
  int32_t (*mid)(void* user, const float* tau, int32_t r_local, float* out_scores);
  /* optional (all NULL: begin in one call): dhr_search_pre_ranks / dhr_search_pre / dhr_search_begin_rest of the shard */
  int32_t (*pre_ranks)(void* user, int32_t k, int32_t share, int32_t* out_local, int32_t* out_union);
  int32_t (*pre)(void* user, const dhr_query_batch* queries, int32_t k, int32_t share, int32_t r_local, float* out_scores);
  int32_t (*begin_rest)(void* user, const float* tau, float* out_sample);
} dhr_host_shard;
int dhr_search_sharded_host(const dhr_host_shard* shard, int32_t world, int32_t rank, dhr_allgather_fn allgather, void* user,
                            const dhr_query_batch* queries, int32_t k, float* out_scores, int64_t* out_rows);
int dhr_search_sharded(dhr_index* shard, dhr_comm* comm, const dhr_query_batch* queries, int32_t k, float* out_scores,
                       int64_t* out_rows, int32_t out_mem_kind, void* stream);
int dhr_search_sharded_local(dhr_index** shards, int32_t n_shards, const dhr_query_batch* queries, int32_t k, float* out_scores,
                             int64_t* out_rows, int32_t out_mem_kind, void* stream);

/* k-means over whole fp16 rows (kmeans.hip): the clustering behind the query-cluster files of topic-aware sampling.
 *   values [n, d] fp16 with row stride ld >= d (elements; a column range of a wider record is selected through the base pointer and ld, the
 *   base need not be aligned), centroids [K, d] fp32 packed.  1 <= d <= 4096, 1 <= K <= 65536, 1 <= n < 2^31; K > n is legal.  mem_kind says
 *   where EVERY array of the call lives: host arrays are staged through the device and complete on return, device arrays are only enqueued on
 *   `stream` and nothing waits.  Every output is a function of the arguments alone (no atomics): two calls give the same bits.
 * dhr_kmeans_assign: assign[i] = the j with the largest t(i, j) = <x_i, c_j> - 1/2 |c_j|^2 (the nearest centroid), the lowest such j on a tie;
 *   dist[i] = |x_i|^2 - 2 t(i, assign[i]) (dist may be NULL).  No [n, K] array is made; device scratch is O(K * d).
 * dhr_kmeans_update: centroid j becomes the fp32 mean of its members, added in increasing row order; a cluster without members keeps the centroid
 *   it came with and gets counts[j] = 0.  An assign entry outside [0, K) is DHR_ERR_INVALID for host arrays; in device arrays, which are not read
 *   back, such a row joins no cluster.
 * dhr_kmeans: exactly `iters` (>= 0) rounds of assign + update, then one last assign against the final centroids (no early stop: that would need
 *   a device read per round).  objective[t], t in [0, iters], is the float64 sum of dist after the t-th assignment, summed in a fixed order;
 *   changed[t] the number of rows whose assignment differs from the round before, changed[0] = n.  assign, counts and objective[iters]
 *   describe the final centroids. */
int dhr_kmeans_assign(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, const float* centroids, int32_t K,
                      int32_t* assign, float* dist, void* stream);
int dhr_kmeans_update(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, const int32_t* assign, int32_t K,
                      float* centroids, int64_t* counts, void* stream);
int dhr_kmeans(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t K, int32_t iters, float* centroids,
               int32_t* assign, int64_t* counts, double* objective, int64_t* changed, void* stream);

/* Streamed exact inner-product search over fp32 vectors of any width (stream_search.hip): the retrieval route that scores un-densified vectors,
 * [lexical reps over the whole vocabulary | semantic reps], chunk by chunk with a running top-k per query.
 *   score(q, r) = sum_c qa[q][c] pa[r][c] + sum_c qb[q][c] pb[r][c] over two column segments of d_a >= 1 and d_b >= 0 columns (q_b / p_b NULL
 *   exactly when d_b = 0), d_a + d_b <= 131072; fp32 rows with row strides (elements), any alignment.  value_dtype is DHR_VAL_F32; DHR_VAL_F16 is
 *   DHR_ERR_UNSUPPORTED.  1 <= n_queries <= 65536, 1 <= k <= 4096 (larger k: DHR_ERR_UNSUPPORTED).  block_rows: passage rows scored between two
 *   selects, 0 for the default, else a multiple of 128 in [128, 65536]; device memory is 4 (n_queries + block_rows) (d_a + d_b) bytes of fp16
 *   images, 8 n_queries block_rows of candidates and the lists.
 *   A score is a function of its query row and its passage row alone, bit for bit: it does not depend on the call or block a row arrived in, on
 *   the order of the calls or on block_rows.  Its error is at most 2^-15 sum_c |q_c p_c| (tests/test_stream_search.py derives the bound).  A row
 *   that holds a NaN or an infinity gets what IEEE arithmetic gives; a NaN score enters no list and changes no other score.
 * dhr_stream_search_create: splits the queries; the lists start as (-inf, -1).
 * dhr_stream_search_add: scores n_rows passages (n_rows = 0: DHR_OK, nothing is launched) against every query and merges them into the lists;
 *   their rows are reported as row_base + position.  mem_kind says where the arrays of THIS call live: host arrays are staged through the
 *   device block by block and the call is complete on return; device arrays are only enqueued on `stream`.
 * dhr_stream_search_result: the k best rows of every query over everything added so far, score descending, row ascending on exact ties,
 *   (-inf, -1) beyond the rows seen; out_scores [n_queries, k], out_rows [n_queries, k].  May be called any number of times and does not end the
 *   search. */
typedef struct dhr_stream_search dhr_stream_search;
int dhr_stream_search_create(int32_t device, int32_t mem_kind, const void* q_a, int64_t ld_qa, const void* q_b, int64_t ld_qb, int32_t value_dtype,
                             int32_t n_queries, int32_t d_a, int32_t d_b, int32_t k, int32_t block_rows, dhr_stream_search** out, void* stream);
int dhr_stream_search_add(dhr_stream_search* s, int32_t mem_kind, const void* p_a, int64_t ld_pa, const void* p_b, int64_t ld_pb, int32_t value_dtype,
                          int64_t n_rows, int64_t row_base, void* stream);
int dhr_stream_search_result(dhr_stream_search* s, float* out_scores, int64_t* out_rows, int32_t out_mem_kind, void* stream);
int64_t dhr_stream_search_device_bytes(const dhr_stream_search* s);
void dhr_stream_search_destroy(dhr_stream_search* s);

#ifdef __cplusplus
}
#endif
#endif /* DHR_HIP_H */

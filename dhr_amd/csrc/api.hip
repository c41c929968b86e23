// Search entry points of the C ABI (include/dhr_hip.h): dhr_search, dhr_search_rerank, the staged calls of the sharded search, dhr_score_rows;
// densify, PQ training / encoding / decoding, debug hooks, shard reduce.  Host arrays are staged with the vocabulary of host_stage.h; every HIP call
// whose failure answers DHR_ERR_HIP goes through HIP_TRY.  The handle and its build: index_build.hip; the controller (search_core): search_core.hip;
// the sharded control flow: sharded.hip; error record, exception classifier: abi.cpp.
#include "host_stage.h"

namespace {
// ---- what the search entry points share
dhr_search_stats fresh_stats(const dhr_index* ix, int Q, int k) {
  dhr_search_stats st{};
  st.n_rows = ix->n_rows; st.n_queries = Q; st.k = k;
  return st;
}
// The sorted top-k keys of the workspace -> the caller's score / row arrays (host arrays are staged through the workspace's grow-only buffer;
// the copies are enqueued)
int emit_results(dhr_index* ix, Workspace& w, int Q, int k, float* out_scores, int64_t* out_rows, int out_mem_kind, hipStream_t s) {
  if (out_mem_kind == DHR_MEM_HOST) {
    const int rc = grow(w.out_stage, w.out_stage_bytes, (size_t)Q * k * 12, w.bytes);
    if (rc != DHR_OK) return rc;
  }
  return emit_topk(w.topk_keys, w.kp, Q, k, ix->row_offset, out_scores, out_rows, out_mem_kind, w.out_stage, s);
}
// The timers of one call (its stream must be idle) added to the running stats: a call that opens a search starts them from zero (fresh_stats),
// one that continues a staged search from the handle's
void collect_timers(Timer& tm, dhr_search_stats& st) {
  double ms[5] = {0, 0, 0, 0, 0};
  tm.collect(ms);
  st.gemm_ms += ms[T_GEMM]; st.refine_ms += ms[T_REFINE]; st.rescore_ms += ms[T_RESCORE]; st.select_ms += ms[T_SELECT]; st.prep_ms += ms[T_PREP];
}
// The frame of a whole search that the caller waits for (dhr_search, dhr_search_rerank): body(timer, stats) enqueues the search and the
// delivery of its result on s; the frame times it between two events, waits for the stream, collects the timers into the handle's stats -- and
// drains the handle's streams where the body fails or throws.
template <typename Body>
int timed_search(dhr_index* ix, int Q, int k, hipStream_t s, Body&& body) {
  Events evs;
  hipEvent_t ev0, ev1;
  HIP_TRY(evs.add(&ev0)); HIP_TRY(evs.add(&ev1));
  HIP_TRY(hipEventRecord(ev0, s));
  Timer tm{ix->profile != 0, s, {}, {}};
  dhr_search_stats st = fresh_stats(ix, Q, k);
  Drain drain{ix, s};
  const int rc = body(tm, st);
  if (rc != DHR_OK) return rc;
  HIP_TRY(hipEventRecord(ev1, s));
  HIP_TRY(hipStreamSynchronize(s));
  float total = 0.f;
  hipEventElapsedTime(&total, ev0, ev1);
  st.total_ms = total;
  collect_timers(tm, st);
  ix->stats = st;
  drain.armed = false;
  return DHR_OK;
}
// Controller without read-backs: the candidate counters live on the device (zero otherwise) and run on over the calls of a staged search.
// Reads them (synchronises s) and adds what they gained since the last fold of this staged search.
int fold_device_counters(dhr_index* ix, dhr_search_stats& st, hipStream_t s) {
  Workspace& w = ix->ws;
  HIP_TRY(hipMemcpyAsync(w.h_stats, w.d_stats, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t bound = (int64_t)((unsigned long long*)w.h_stats)[0], exact = (int64_t)((unsigned long long*)w.h_stats)[1];
  st.candidates_bound += bound - ix->pend.dev_bound;
  st.candidates_exact += exact - ix->pend.dev_exact;
  ix->pend.dev_bound = bound; ix->pend.dev_exact = exact;
  return DHR_OK;
}
// Every staged entry point runs through here: one that fails -- a status or an exception on its way to the barrier -- leaves NO staged search
// open on the handle.  Its workspace may be half-consumed, so a later dhr_search_mid / _finish must not be accepted: the caller starts again
// with dhr_search_begin or dhr_search_pre.
template <typename Body>
int staged_call(dhr_index* ix, Body&& body) {
  struct Close {
    dhr_index* ix; bool ok = false;
    ~Close() { if (!ok && ix) staged_set(ix, StagedState::None); }
  } close{ix};
  const int rc = body();
  close.ok = rc == DHR_OK;
  return rc;
}
// What the staged calls hand to the shards' agreement: the r best scores a handle has seen so far, [Q, r] on the device ...
int emit_best_scores(dhr_index* ix, int Q, int r, float* out_dev, hipStream_t s) {
  HIP_TRY(launch_emit_scores(ix->ws.topk_keys, ix->ws.kp, Q, r, out_dev, s));
  return DHR_OK;
}
// ... after a sampled run: its dhr_search_sample_rank best (nothing where the shard is not sampled: the call already ran the whole search)
int emit_sample_scores(dhr_index* ix, int Q, int k, float* out_dev, hipStream_t s) {
  const int r = dhr_search_sample_rank(ix, k);
  if (r <= 0 || ix->pend.state == StagedState::Complete) return DHR_OK;
  if (!out_dev) return set_error(DHR_ERR_INVALID, "null sample score buffer");
  return emit_best_scores(ix, Q, r, out_dev, s);
}
// What the staged entry points share behind their validation: one stage of search_core, what it hands out (emit: enqueued), and -- where the
// caller waits for the call (collect) or profiles -- the device counters (fold) and the timers.  qb: the call opens the staged search and its
// counters; else it continues them.  collect = false (dhr_search_sharded*): the call only enqueues, the shards of a one-process search work concurrently.
template <typename Emit>
int staged_step(dhr_index* ix, const dhr_query_batch* qb, int k, Stage stage, const float* tau_dev, void* stream, bool collect, bool fold, Emit&& emit) {
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  if (qb) { staged_set(ix, StagedState::None); ix->pend.dev_bound = ix->pend.dev_exact = 0; }
  Timer tm{ix->profile != 0, s, {}, {}};
  dhr_search_stats st = qb ? fresh_stats(ix, qb->n_queries, k) : ix->stats;
  Drain drain{ix, s};
  int rc = search_core(ix, ix->ws, qb, k, 0, tm, st, s, stage, tau_dev);
  if (rc != DHR_OK || (rc = emit(s)) != DHR_OK) return rc;
  if (collect || ix->profile) {
    if (fold) rc = fold_device_counters(ix, st, s);
    else HIP_TRY(hipStreamSynchronize(s));
    if (rc != DHR_OK) return rc;
    collect_timers(tm, st);
  }
  ix->stats = st;
  drain.armed = false;
  return DHR_OK;
}
}  // namespace

extern "C" int dhr_search(dhr_index* ix, const dhr_query_batch* qb, int32_t k, float* out_scores, int64_t* out_rows,
                          int32_t out_mem_kind, void* stream) try {
  dhr::alloc_checkpoint();
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (k <= 0) return set_error(DHR_ERR_INVALID, "k must be > 0");
  if (k > (1 << 20)) return set_error(DHR_ERR_UNSUPPORTED, "k > 1048576 is not supported");      // k > 16384: global-memory merge (select_global.hip)
  if (!out_scores || !out_rows) return set_error(DHR_ERR_INVALID, "null output pointer");
  if (!DHR_MEM_KIND_OK(out_mem_kind)) return set_error(DHR_ERR_INVALID, "bad out_mem_kind");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  const int Q = qb->n_queries;
  staged_set(ix, StagedState::None);          // a plain search overwrites the workspace of any staged search left open on this handle
  return timed_search(ix, Q, k, s, [&](Timer& tm, dhr_search_stats& st) {
    const int rc = search_core(ix, ix->ws, qb, k, 0, tm, st, s);
    return rc != DHR_OK ? rc : emit_results(ix, ix->ws, Q, k, out_scores, out_rows, out_mem_kind, s);
  });
} DHR_CATCH_STATUS

// dhr_search with per-query exclusion lists: the ordinary search at depth k + Emax (Emax: the longest list of the batch), its lists emitted into
// the handle's grow-only staging buffer, the filter of exclude.hip behind it -- no kernel and no plan of the search itself is touched.  The
// buffer holds [rows k' | scores k' | offsets | the caller's host rows | out rows k | out scores k] (the last three only where they are staged).
extern "C" int dhr_search_excluding(dhr_index* ix, const dhr_query_batch* qb, int32_t k, const int64_t* excl_ptr_host, const int64_t* excl_rows,
                                    int32_t excl_mem_kind, float* out_scores, int64_t* out_rows, int32_t out_mem_kind, void* stream) try {
  dhr::alloc_checkpoint();
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (k <= 0) return set_error(DHR_ERR_INVALID, "k must be > 0");
  if (!out_scores || !out_rows) return set_error(DHR_ERR_INVALID, "null output pointer");
  if (!DHR_MEM_KIND_OK(out_mem_kind)) return set_error(DHR_ERR_INVALID, "bad out_mem_kind");
  if (!DHR_MEM_KIND_OK(excl_mem_kind)) return set_error(DHR_ERR_INVALID, "bad excl_mem_kind");
  const int Q = qb->n_queries;
  int64_t e_max = 0, e_total = 0;
  if ((rc = check_exclusions(Q, excl_ptr_host, excl_rows, &e_max, &e_total)) != DHR_OK) return rc;
  if (e_max == 0) return dhr_search(ix, qb, k, out_scores, out_rows, out_mem_kind, stream);      // nothing to exclude: the plain search, bit for bit
  if ((int64_t)k + e_max > (1 << 20))
    return set_error(DHR_ERR_UNSUPPORTED, "k + the longest exclusion list = " + std::to_string(k) + " + " + std::to_string(e_max) +
                                              " > 1048576 is not supported (split the batch: one long list deepens every query's search)");
  const int kd = (int)(k + e_max);              // k' > 16384: global-memory merge (select_global.hip), as for any deep dhr_search
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  staged_set(ix, StagedState::None);
  return timed_search(ix, Q, kd, s, [&](Timer& tm, dhr_search_stats& st) {
    Workspace& w = ix->ws;
    int rc = search_core(ix, w, qb, kd, 0, tm, st, s);
    if (rc != DHR_OK) return rc;
    const bool host_out = out_mem_kind == DHR_MEM_HOST, host_ex = excl_mem_kind == DHR_MEM_HOST;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_rows = 0, o_scores = o_rows + up16((size_t)Q * kd * 8), o_ptr = o_scores + up16((size_t)Q * kd * 4);
    const size_t o_ex = o_ptr + up16((size_t)(Q + 1) * 8), o_orows = o_ex + (host_ex ? up16((size_t)e_total * 8) : 0);
    const size_t o_oscores = o_orows + (host_out ? up16((size_t)Q * k * 8) : 0), need = o_oscores + (host_out ? up16((size_t)Q * k * 4) : 0);
    if ((rc = grow(w.out_stage, w.out_stage_bytes, need, w.bytes)) != DHR_OK) return rc;
    char* base = (char*)w.out_stage;
    int64_t* d_rows = (int64_t*)(base + o_rows);
    float* d_scores = (float*)(base + o_scores);
    int64_t* d_ptr = (int64_t*)(base + o_ptr);
    HIP_TRY(launch_emit(w.topk_keys, w.kp, Q, kd, ix->row_offset, d_scores, d_rows, s));
    HIP_TRY(copy_in(d_ptr, excl_ptr_host, (size_t)(Q + 1) * 8, s));
    const int64_t* d_ex = excl_rows;
    if (host_ex) {
      HIP_TRY(copy_in(base + o_ex, excl_rows, (size_t)e_total * 8, s));
      d_ex = (const int64_t*)(base + o_ex);
    }
    int64_t* f_rows = host_out ? (int64_t*)(base + o_orows) : out_rows;
    float* f_scores = host_out ? (float*)(base + o_oscores) : out_scores;
    HIP_TRY(launch_exclude_rows(Q, kd, d_scores, d_rows, d_ptr, d_ex, e_max, k, f_scores, f_rows, nullptr, s));
    if (host_out) {
      HIP_TRY(stage_out(out_rows, f_rows, (size_t)Q * k * 8, s));
      HIP_TRY(stage_out(out_scores, f_scores, (size_t)Q * k * 4, s));
    }
    return (int)DHR_OK;
  });
} DHR_CATCH_STATUS

// Two-stage approximate GIP on the device (gip_retrieval.py:128-156): stage 1 is an ordinary search of the
// restricted batch for k1 rows, stage 2 the exact gated inner product of the full batch on exactly those rows
// and the top-k of that; the k1 rows never leave the device.
extern "C" int dhr_search_rerank(dhr_index* ix, const dhr_query_batch* qb1, const dhr_query_batch* qb2, int32_t k1, int32_t k,
                                 float* out_scores, int64_t* out_rows, int32_t out_mem_kind, void* stream) try {
  dhr::alloc_checkpoint();
  int rc = check_queries(ix, qb1);
  if (rc) return rc;
  if ((rc = check_queries(ix, qb2)) != DHR_OK) return rc;
  if (qb1->n_queries != qb2->n_queries) return set_error(DHR_ERR_INVALID, "the two query batches differ in n_queries");
  if (k <= 0 || k1 < k) return set_error(DHR_ERR_INVALID, "need 0 < k <= k1");
  if (k1 > (1 << 20)) return set_error(DHR_ERR_UNSUPPORTED, "k1 > 1048576 is not supported");
  if (!out_scores || !out_rows) return set_error(DHR_ERR_INVALID, "null output pointer");
  if (!DHR_MEM_KIND_OK(out_mem_kind)) return set_error(DHR_ERR_INVALID, "bad out_mem_kind");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  const int Q = qb1->n_queries;
  return timed_search(ix, Q, k, s, [&](Timer& tm, dhr_search_stats& st) {
    Workspace& w = ix->ws;
    // ---- stage 1
    int rc = search_core(ix, w, qb1, k1, 0, tm, st, s);
    if (rc != DHR_OK) return rc;
    // ---- stage 2: exact scores of the stage-1 rows under the full batch, top-k of those
    DevMem rows_mem;
    HIP_TRY(dev_alloc(rows_mem, (int64_t)Q * k1 * 4));
    uint32_t* d_rows32 = (uint32_t*)rows_mem.p;
    HIP_TRY(launch_keys_to_rows(w.topk_keys, w.kp, Q, k1, d_rows32, s));
    if (w.keys_ld < k1) return set_error(DHR_ERR_INTERNAL, "key buffer smaller than k1");
    const bool gate2 = ix->d_dlr > 0 && qb2->index != nullptr && qb2->index_dtype != DHR_IDX_NONE;
    tm.begin(T_PREP);
    if ((rc = prep_queries(ix, w, qb2, s)) != DHR_OK) return rc;
    HIP_TRY(hipMemsetAsync(w.topk_keys, 0, (size_t)w.q_pad * w.kp * 8, s));
    tm.end();
    RescoreArgs r = base_rescore_args(ix, w, Q, gate2);
    r.rows32 = d_rows32; r.ld_rows = k1; r.count_all = (uint32_t)k1; r.max_count = (uint32_t)k1;
    r.out_keys = w.rs_keys; r.ld_keys = w.keys_ld;
    tm.begin(T_RESCORE);
    HIP_TRY(launch_rescore(r, s));
    tm.end();
    st.candidates_exact += (int64_t)Q * k1;
    SelectArgs sel = rescored_select_args(w, Q, k);
    sel.count_all = (uint32_t)k1;            // every query has exactly its k1 keys (no count array)
    tm.begin(T_SELECT);
    HIP_TRY(launch_select(sel, s));
    tm.end();
    return emit_results(ix, w, Q, k, out_scores, out_rows, out_mem_kind, s);
  });
} DHR_CATCH_STATUS

// ---- staged search for the row-sharded path (dhr_amd/dist.py): the shards agree on ONE threshold per
// query after their sampled runs, so each shard collects only its share of the global top-k.
// The rank queries read the plan the staged calls of this handle run (search_plan.h): a shard never reports a rank its controller does not chase.
extern "C" int32_t dhr_search_sample_rank(const dhr_index* ix, int32_t k) try {
  if (!ix || k <= 0) return 0;
  const SearchPlan p = search_plan_of(ix, k, 0, true);
  return p.S >= 2 ? p.r_eff : 0;
} DHR_CATCH_VALUE(0)
extern "C" int32_t dhr_search_union_rank(const dhr_index* ix, int32_t k) try {
  if (!ix || k <= 0) return 0;
  const SearchPlan p = search_plan_of(ix, k, 0, true);
  return p.S >= 2 ? p.r : 0;
} DHR_CATCH_VALUE(0)

// Ranks of the second agreement (dhr_search_mid): after the head, the sample and the first slice of the main pass a shard has seen the
// fraction f of its rows, scattered; the shards agree on the (k f + 6 sigma + 4)-th best score of the union of what they have seen, and a shard
// reports its share of that rank (SearchPlan::mid_union / mid_local; 0: this index has no mid step).
static int32_t local_and_union(int32_t local, int32_t uni, int32_t* out_local, int32_t* out_union) {
  if (out_local) *out_local = local;
  if (out_union) *out_union = uni;
  return local;
}
extern "C" int32_t dhr_search_mid_ranks(const dhr_index* ix, int32_t k, int32_t* out_local, int32_t* out_union) try {
  if (!ix || k <= 0) return local_and_union(0, 0, out_local, out_union);
  const SearchPlan p = search_plan_of(ix, k, 0, true);
  return local_and_union(p.mid_local, p.mid_union, out_local, out_union);
} DHR_CATCH_VALUE(0)
// The first slice of the main pass with the thresholds of the first agreement; leaves the shard's r_local best scores seen so far in
// out_scores_dev [Q, r_local] (r_local: dhr_search_mid_ranks, or what the shards agreed on).  dhr_search_finish then takes the thresholds of the
// second agreement.
static int search_mid_impl(dhr_index* ix, const float* tau_hat_dev, int32_t r_local, float* out_scores_dev, void* stream, bool sync) {
  if (!ix || ix->pend.state == StagedState::None) return set_error(DHR_ERR_INVALID, "dhr_search_mid without a matching dhr_search_begin");
  if (ix->pend.state == StagedState::Complete) {                                // the shard was not sampled: its search is complete already
    if (sync) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));              // (the call still answers for the caller's stream)
    return DHR_OK;
  }
  if (ix->pend.state == StagedState::AfterMid) return set_error(DHR_ERR_INVALID, "dhr_search_mid called twice");
  if (!tau_hat_dev || !out_scores_dev) return set_error(DHR_ERR_INVALID, "null pointer");
  if (dhr_search_mid_ranks(ix, ix->pend.k, nullptr, nullptr) <= 0) return set_error(DHR_ERR_INVALID, "this index has no mid step (dhr_search_mid_ranks returned 0)");
  if (r_local <= 0 || r_local > ix->pend.k) return set_error(DHR_ERR_INVALID, "r_local must be in [1, k]");
  return staged_step(ix, nullptr, ix->pend.k, Stage::Mid, tau_hat_dev, stream, sync, false,
                     [&](hipStream_t s) { return emit_best_scores(ix, ix->pend.Q, r_local, out_scores_dev, s); });
}
extern "C" int dhr_search_mid(dhr_index* ix, const float* tau_hat_dev, int32_t r_local, float* out_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_mid_impl(ix, tau_hat_dev, r_local, out_scores_dev, stream, true); });
} DHR_CATCH_STATUS
extern "C" int dhr_internal_search_mid_async(dhr_index* ix, const float* tau_hat_dev, int32_t r_local, float* out_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_mid_impl(ix, tau_hat_dev, r_local, out_scores_dev, stream, false); });
} DHR_CATCH_STATUS

// ---- first agreement in TWO rounds (round 5).  The shards of a sharded search each ran their whole sampled run from nothing, chasing their
// share of the union's rank on their own: eight runs together rescored 3.2 k rows per query where the unsharded search's one run rescores
// 0.7 k.  dhr_search_pre streams the first part of the shard's sample and reports its best scores seen so far, the shards agree on a COMMON
// threshold from them (SearchPlan::pre_union / pre_local; 0: the sample is too small to split), and dhr_search_begin_rest streams the rest of
// the sample filtering at it.  Whatever that threshold is worth, the lists a shard reports afterwards are complete above it, so the union
// threshold computed from them can only come out lower than the true one -- still valid; the count check at the end of the step verifies it.
extern "C" int32_t dhr_search_pre_ranks(const dhr_index* ix, int32_t k, int32_t* out_local, int32_t* out_union) try {
  if (!ix || k <= 0) return local_and_union(0, 0, out_local, out_union);
  const SearchPlan p = search_plan_of(ix, k, 0, true);
  return local_and_union(p.pre_local, p.pre_union, out_local, out_union);
} DHR_CATCH_VALUE(0)
static int search_pre_impl(dhr_index* ix, const dhr_query_batch* qb, int32_t k, int32_t r_local, float* out_scores_dev, void* stream, bool sync) {
  dhr::alloc_checkpoint();
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (k <= 0 || k > (1 << 20)) return set_error(DHR_ERR_INVALID, "k must be in [1, 1048576]");
  if (!out_scores_dev) return set_error(DHR_ERR_INVALID, "null pointer");
  if (dhr_search_pre_ranks(ix, k, nullptr, nullptr) <= 0) return set_error(DHR_ERR_INVALID, "this index has no pre step (dhr_search_pre_ranks returned 0)");
  if (r_local <= 0 || r_local > k) return set_error(DHR_ERR_INVALID, "r_local must be in [1, k]");
  return staged_step(ix, qb, k, Stage::Pre, nullptr, stream, sync, false,
                     [&](hipStream_t s) { return emit_best_scores(ix, qb->n_queries, r_local, out_scores_dev, s); });
}
extern "C" int dhr_search_pre(dhr_index* ix, const dhr_query_batch* qb, int32_t k, int32_t r_local, float* out_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_pre_impl(ix, qb, k, r_local, out_scores_dev, stream, true); });
} DHR_CATCH_STATUS
extern "C" int dhr_internal_search_pre_async(dhr_index* ix, const dhr_query_batch* qb, int32_t k, int32_t r_local, float* out_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_pre_impl(ix, qb, k, r_local, out_scores_dev, stream, false); });
} DHR_CATCH_STATUS
// the rest of the sampled run behind dhr_search_pre; leaves the handle where dhr_search_begin leaves it (out_sample_scores_dev: [Q, dhr_search_sample_rank])
static int search_begin_rest_impl(dhr_index* ix, const float* tau_dev, float* out_sample_scores_dev, void* stream, bool sync) {
  if (!ix || ix->pend.state != StagedState::AfterPre) return set_error(DHR_ERR_INVALID, "dhr_search_begin_rest without a matching dhr_search_pre");
  if (!tau_dev || !out_sample_scores_dev) return set_error(DHR_ERR_INVALID, "null pointer");
  const int k = ix->pend.k, Q = ix->pend.Q;
  return staged_step(ix, nullptr, k, Stage::BeginRest, tau_dev, stream, sync, true,
                     [&](hipStream_t s) { return emit_sample_scores(ix, Q, k, out_sample_scores_dev, s); });
}
extern "C" int dhr_search_begin_rest(dhr_index* ix, const float* tau_dev, float* out_sample_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_begin_rest_impl(ix, tau_dev, out_sample_scores_dev, stream, true); });
} DHR_CATCH_STATUS
extern "C" int dhr_internal_search_begin_rest_async(dhr_index* ix, const float* tau_dev, float* out_sample_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_begin_rest_impl(ix, tau_dev, out_sample_scores_dev, stream, false); });
} DHR_CATCH_STATUS

// (sync = false: the call only enqueues; statistics and timers are then not collected -- staged_step)
static int search_begin_impl(dhr_index* ix, const dhr_query_batch* qb, int32_t k, float* out_sample_scores_dev, void* stream, bool sync) {
  dhr::alloc_checkpoint();
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (k <= 0 || k > (1 << 20)) return set_error(DHR_ERR_INVALID, "k must be in [1, 1048576]");
  return staged_step(ix, qb, k, Stage::Begin, nullptr, stream, sync, true,
                     [&](hipStream_t s) { return emit_sample_scores(ix, qb->n_queries, k, out_sample_scores_dev, s); });
}
extern "C" void dhr_internal_search_abort(dhr_index* ix) try {
  if (ix) staged_set(ix, StagedState::None);
} DHR_CATCH_VOID
extern "C" int dhr_search_begin(dhr_index* ix, const dhr_query_batch* qb, int32_t k, float* out_sample_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_begin_impl(ix, qb, k, out_sample_scores_dev, stream, true); });
} DHR_CATCH_STATUS
extern "C" int dhr_internal_search_begin_async(dhr_index* ix, const dhr_query_batch* qb, int32_t k, float* out_sample_scores_dev, void* stream) try {
  return staged_call(ix, [&] { return search_begin_impl(ix, qb, k, out_sample_scores_dev, stream, false); });
} DHR_CATCH_STATUS

static int search_finish_impl(dhr_index* ix, const float* tau_hat_dev, float* out_scores, int64_t* out_rows,
                              int32_t* out_count_dev, int32_t out_mem_kind, void* stream, bool sync) {
  if (!ix || ix->pend.state == StagedState::None) return set_error(DHR_ERR_INVALID, "dhr_search_finish without a matching dhr_search_begin");
  if (!out_scores || !out_rows || !out_count_dev) return set_error(DHR_ERR_INVALID, "null output pointer");
  if (!DHR_MEM_KIND_OK(out_mem_kind)) return set_error(DHR_ERR_INVALID, "bad out_mem_kind");
  const bool complete = ix->pend.state == StagedState::Complete;      // the begin call already ran the whole (unsampled) search: no thresholds to check against
  if (!complete && !tau_hat_dev) return set_error(DHR_ERR_INVALID, "thresholds are required (the shard ran a sampled pass)");
  const int Q = ix->pend.Q, k = ix->pend.k;
  Workspace& w = ix->ws;
  const int rc = staged_step(ix, nullptr, k, Stage::Finish, tau_hat_dev, stream, sync || out_mem_kind == DHR_MEM_HOST, true, [&](hipStream_t s) {
    HIP_TRY(launch_count_ge(w.topk_keys, w.kp, k, complete ? nullptr : w.tau_hat, complete ? nullptr : w.fail_flags, Q, out_count_dev, s));
    return emit_results(ix, w, Q, k, out_scores, out_rows, out_mem_kind, s);
  });
  if (rc == DHR_OK) staged_set(ix, StagedState::None);
  return rc;
}
extern "C" int dhr_search_finish(dhr_index* ix, const float* tau_hat_dev, float* out_scores, int64_t* out_rows,
                                 int32_t* out_count_dev, int32_t out_mem_kind, void* stream) try {
  return staged_call(ix, [&] { return search_finish_impl(ix, tau_hat_dev, out_scores, out_rows, out_count_dev, out_mem_kind, stream, true); });
} DHR_CATCH_STATUS
extern "C" int dhr_internal_search_finish_async(dhr_index* ix, const float* tau_hat_dev, float* out_scores, int64_t* out_rows,
                                                int32_t* out_count_dev, int32_t out_mem_kind, void* stream) try {
  return staged_call(ix, [&] { return search_finish_impl(ix, tau_hat_dev, out_scores, out_rows, out_count_dev, out_mem_kind, stream, false); });
} DHR_CATCH_STATUS

extern "C" int dhr_score_rows(dhr_index* ix, const dhr_query_batch* qb, int32_t m, const int64_t* rows, float* out_scores,
                              int32_t mem_kind, void* stream) try {
  dhr::alloc_checkpoint();
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (m <= 0 || !rows || !out_scores) return set_error(DHR_ERR_INVALID, "bad m / null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (ix->pend.state != StagedState::None && ix->pend.state != StagedState::Complete)      // the staged search keeps its query batch in the workspace this call would overwrite
    return set_error(DHR_ERR_INVALID, "dhr_score_rows between dhr_search_begin and dhr_search_finish on the same handle");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  const int Q = qb->n_queries;
  const bool gate = ix->d_dlr > 0 && qb->index != nullptr && qb->index_dtype != DHR_IDX_NONE;
  Workspace& w = ix->ws;
  if ((rc = ensure_ws(ix, w, Q, 1, 0, 1, true, true)) != DHR_OK) return rc;
  if ((rc = prep_queries(ix, w, qb, s)) != DHR_OK) return rc;
  const size_t n = (size_t)Q * m;
  DevMem m_rows64, m_rows32, m_scores;
  const int64_t* d_rows64;
  float* d_scores;
  HIP_TRY(operand_in(m_rows64, mem_kind, rows, n * 8, s, d_rows64));
  HIP_TRY(dev_alloc(m_rows32, (int64_t)n * 4));
  HIP_TRY(operand_out(m_scores, mem_kind, out_scores, n * 4, d_scores));
  uint32_t* d_rows32 = (uint32_t*)m_rows32.p;
  HIP_TRY(launch_rows_to_local(d_rows64, (int64_t)n, ix->row_offset, ix->n_rows, d_rows32, s));
  RescoreArgs r = base_rescore_args(ix, w, Q, gate);
  r.rows32 = d_rows32; r.ld_rows = m; r.count_all = (uint32_t)m; r.max_count = (uint32_t)m;
  r.out_scores = d_scores; r.ld_scores = m;
  HIP_TRY(launch_rescore(r, s));
  HIP_TRY(operand_back(m_scores, out_scores, n * 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_densify(int32_t device, int32_t mem_kind, const void* lexical, int32_t value_dtype, int64_t ld, int64_t batch, int32_t vocab,
                           int32_t remove_dims, int32_t dims, void* out_value, int32_t out_value_dtype, int64_t ld_value, void* out_index,
                           int32_t index_dtype, int64_t ld_index, void* stream) try {
  if (!lexical || !out_value || !out_index) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (batch < 0 || vocab <= 0 || dims <= 0 || remove_dims < 0 || remove_dims >= vocab || ld < vocab || ld_value < dims || ld_index < dims)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if ((vocab - remove_dims) % dims != 0)
    return set_error(DHR_ERR_INVALID, "Input lexical representation cannot be densified, please fix dims or remove_dims");
  if (!val_ok(value_dtype) || !val_ok(out_value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  const int n_groups = (vocab - remove_dims) / dims;
  if (index_dtype != DHR_IDX_U8 && index_dtype != DHR_IDX_I16) return set_error(DHR_ERR_INVALID, "index dtype must be uint8 or int16");
  if (index_dtype == DHR_IDX_U8 && n_groups > 256) return set_error(DHR_ERR_UNSUPPORTED, "more than 256 groups need the int16 index dtype");
  if (n_groups > 32767) return set_error(DHR_ERR_UNSUPPORTED, "more than 32767 groups");
  if (batch == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int ies = val_esize(value_dtype), oes = val_esize(out_value_dtype), xes = index_dtype == DHR_IDX_I16 ? 2 : 1;
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_densify(lexical, value_dtype == DHR_VAL_F32, ld, batch, remove_dims, dims, n_groups, out_value, out_value_dtype == DHR_VAL_F32,
                           ld_value, out_index, index_dtype == DHR_IDX_I16, ld_index, s));
    return DHR_OK;                                        // enqueued: a training step stays asynchronous
  }
  // host arrays: stage blocks of rows through the device (complete on return)
  const int64_t block = std::max<int64_t>(1, std::min<int64_t>(batch, ((int64_t)256 << 20) / ((int64_t)vocab * ies)));
  DevMem m_in, m_val, m_idx;
  HIP_TRY(dev_alloc(m_in, block * vocab * ies));
  HIP_TRY(dev_alloc(m_val, block * dims * oes));
  HIP_TRY(dev_alloc(m_idx, block * dims * xes));
  for (int64_t lo = 0; lo < batch; lo += block) {
    const int64_t rows = std::min(block, batch - lo);
    HIP_TRY(copy_in(m_in.p, (const char*)lexical + lo * ld * ies, ld, rows, vocab, ies, s));
    HIP_TRY(launch_densify(m_in.p, value_dtype == DHR_VAL_F32, vocab, rows, remove_dims, dims, n_groups, m_val.p, out_value_dtype == DHR_VAL_F32, dims,
                           m_idx.p, index_dtype == DHR_IDX_I16, dims, s));
    HIP_TRY(stage_out((char*)out_value + lo * ld_value * oes, ld_value, m_val.p, rows, dims, oes, s));
    HIP_TRY(stage_out((char*)out_index + lo * ld_index * xes, ld_index, m_idx.p, rows, dims, xes, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DHR_OK;
} DHR_CATCH_STATUS

// ------------------------------------------------------------------------------------------ product quantiser
namespace {
int pq_check(const void* a, const void* b, int64_t n, int d, int M, int64_t ld, int mem_kind) {
  if (!a || !b) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (n < 0 || d <= 0 || M <= 0 || d % M != 0 || ld < d) return set_error(DHR_ERR_INVALID, "bad sizes (d must be a multiple of M, ld >= d)");
  if (d / M > 64) return set_error(DHR_ERR_UNSUPPORTED, "sub-vectors wider than 64 columns are not supported");
  return DHR_OK;
}
}  // namespace

extern "C" int dhr_pq_train(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t M, int32_t iters,
                            int64_t max_points, float* codebooks, double* out_error, void* stream) try {
  return dhr_pq_train_nbits(device, mem_kind, values, ld, n, d, M, 8, iters, max_points, codebooks, out_error, stream);
} DHR_CATCH_STATUS
extern "C" int dhr_pq_train_nbits(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t M, int32_t nbits,
                                  int32_t iters, int64_t max_points, float* codebooks, double* out_error, void* stream) try {
  int rc = pq_check(values, codebooks, n, d, M, ld, mem_kind);
  if (rc) return rc;
  if (nbits < 1 || nbits > 8) return set_error(DHR_ERR_UNSUPPORTED, "nbits must be in [1, 8] (one code byte per sub-quantiser on the device; faiss' bit-packed rows are a file format matter)");
  const int ksub = 1 << nbits;
  if (n < 1 || iters < 0 || max_points < ksub) return set_error(DHR_ERR_INVALID, "need n >= 1, iters >= 0, max_points >= 2^nbits");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int dsub = d / M;
  // training rows: every `stride`-th row (host arrays: only those rows are staged, packed; the codebooks are staged whole, as every PQ operand:
  // they are at most the corpus, which has to fit the device anyway)
  const bool host = mem_kind == DHR_MEM_HOST;
  const int64_t stride = std::max<int64_t>(1, n / max_points);
  const int64_t np = (n + stride - 1) / stride;
  DevMem m_v, m_cb, m_sums, m_counts, m_err;
  if (host) HIP_TRY(stage_in(m_v, values, ld * stride, np, d, 2, s));
  const __half* d_v = (const __half*)(host ? m_v.p : values);
  const int64_t v_ld = host ? d : ld, v_stride = host ? 1 : stride;
  const size_t cb_bytes = (size_t)M * ksub * dsub * 4, cnt_bytes = (size_t)M * ksub * 4;
  float* d_cb;
  HIP_TRY(operand_out(m_cb, mem_kind, codebooks, cb_bytes, d_cb));
  HIP_TRY(dev_alloc(m_sums, (int64_t)cb_bytes));
  HIP_TRY(dev_alloc(m_counts, (int64_t)cnt_bytes));
  HIP_TRY(dev_alloc(m_err, (int64_t)M * 4));
  float* sums = (float*)m_sums.p; uint32_t* counts = (uint32_t*)m_counts.p; float* err = (float*)m_err.p;
  HIP_TRY(launch_pq_init(d_v, v_ld, np, v_stride, dsub, M, d_cb, ksub, s));
  for (int it = 0; it <= iters; ++it) {
    HIP_TRY(hipMemsetAsync(sums, 0, cb_bytes, s));
    HIP_TRY(hipMemsetAsync(counts, 0, cnt_bytes, s));
    HIP_TRY(hipMemsetAsync(err, 0, (size_t)M * 4, s));
    HIP_TRY(launch_pq_assign(d_v, v_ld, np, v_stride, dsub, M, d_cb, nullptr, 0, sums, counts, err, ksub, s));
    if (it == iters) break;                               // the last pass only measures the error
    HIP_TRY(launch_pq_update(d_cb, sums, counts, dsub, M, ksub, s));
  }
  if (out_error) {
    std::vector<float> e(M);
    HIP_TRY(stage_out(e.data(), err, (size_t)M * 4, s));
    HIP_TRY(hipStreamSynchronize(s));
    double t = 0;
    for (float x : e) t += x;
    *out_error = t / (double)np;
  }
  HIP_TRY(operand_back(m_cb, codebooks, cb_bytes, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_pq_encode(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t M,
                             const float* codebooks, uint8_t* codes, void* stream) try {
  return dhr_pq_encode_nbits(device, mem_kind, values, ld, n, d, M, 8, codebooks, codes, stream);
} DHR_CATCH_STATUS
extern "C" int dhr_pq_encode_nbits(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t M, int32_t nbits,
                                   const float* codebooks, uint8_t* codes, void* stream) try {
  int rc = pq_check(values, codebooks, n, d, M, ld, mem_kind);
  if (rc) return rc;
  if (nbits < 1 || nbits > 8) return set_error(DHR_ERR_UNSUPPORTED, "nbits must be in [1, 8]");
  const int ksub = 1 << nbits;
  if (!codes) return set_error(DHR_ERR_INVALID, "null pointer");
  if (n == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int dsub = d / M;
  DevMem m_cb, m_cd;
  const float* d_cb;
  uint8_t* d_cd;
  HIP_TRY(operand_in(m_cb, mem_kind, codebooks, (size_t)M * ksub * dsub * 4, s, d_cb));
  HIP_TRY(operand_out(m_cd, mem_kind, codes, (size_t)n * M, d_cd));
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_pq_assign((const __half*)values, ld, n, 1, dsub, M, d_cb, d_cd, M, nullptr, nullptr, nullptr, ksub, s));
  } else {
    const int64_t block = 1 << 18;                          // rows per staged block
    DevMem stage;
    HIP_TRY(dev_alloc(stage, std::min<int64_t>(block, n) * d * 2));
    for (int64_t lo = 0; lo < n; lo += block) {
      const int64_t rows = std::min(block, n - lo);
      HIP_TRY(copy_in(stage.p, (const char*)values + lo * ld * 2, ld, rows, d, 2, s));
      HIP_TRY(launch_pq_assign((const __half*)stage.p, d, rows, 1, dsub, M, d_cb, d_cd + lo * M, M, nullptr, nullptr, nullptr, ksub, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
  }
  HIP_TRY(operand_back(m_cd, codes, (size_t)n * M, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_pq_decode(int32_t device, int32_t mem_kind, const uint8_t* codes, int64_t n, int32_t d, int32_t M, const float* codebooks,
                             void* out_values, int64_t ld_out, void* stream) try {
  return dhr_pq_decode_nbits(device, mem_kind, codes, n, d, M, 8, codebooks, out_values, ld_out, stream);
} DHR_CATCH_STATUS
extern "C" int dhr_pq_decode_nbits(int32_t device, int32_t mem_kind, const uint8_t* codes, int64_t n, int32_t d, int32_t M, int32_t nbits,
                                   const float* codebooks, void* out_values, int64_t ld_out, void* stream) try {
  int rc = pq_check(codes, codebooks, n, d, M, ld_out, mem_kind);
  if (rc) return rc;
  if (nbits < 1 || nbits > 8) return set_error(DHR_ERR_UNSUPPORTED, "nbits must be in [1, 8]");
  const int ksub = 1 << nbits;
  if (!out_values) return set_error(DHR_ERR_INVALID, "null pointer");
  if (n == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int dsub = d / M;
  const bool host = mem_kind == DHR_MEM_HOST;
  DevMem m_cb, m_cd, m_ov;
  const float* d_cb;
  const uint8_t* d_cd;
  HIP_TRY(operand_in(m_cb, mem_kind, codebooks, (size_t)M * ksub * dsub * 4, s, d_cb));
  HIP_TRY(operand_in(m_cd, mem_kind, codes, (size_t)n * M, s, d_cd));
  if (host) HIP_TRY(dev_alloc(m_ov, n * d * 2));             // decoded rows, packed
  HIP_TRY(launch_pq_decode(d_cd, M, n, M, dsub, d_cb, (__half*)(host ? m_ov.p : out_values), host ? d : ld_out, ksub, s));
  if (host) HIP_TRY(stage_out(out_values, ld_out, m_ov.p, n, d, 2, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_debug_bound_scores(dhr_index* ix, const dhr_query_batch* qb, int64_t row_lo, int64_t row_hi,
                                      float* out_dev, void* stream) try {
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (row_lo < 0 || row_hi > ix->n_rows || row_lo >= row_hi || !out_dev) return set_error(DHR_ERR_INVALID, "bad row range");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  Workspace& w = ix->ws;
  if ((rc = ensure_ws(ix, w, qb->n_queries, 1, 0)) != DHR_OK) return rc;
  if ((rc = prep_queries(ix, w, qb, s)) != DHR_OK) return rc;
  GemmArgs g = base_gemm_args(ix, w, qb->n_queries);
  g.seq_lo = row_lo / TILE_ROWS; g.seq_hi = (row_hi + TILE_ROWS - 1) / TILE_ROWS; g.map_mode = 0; g.period = 1; g.head = 0;      // the tiles of the rows, in corpus order
  g.thr = w.thr; g.cand = w.cand; g.cnt = w.cnt;
  g.dump = out_dev; g.dump_ld = row_hi - row_lo; g.dump_row0 = row_lo;
  HIP_TRY(launch_gemm_filter(g, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_debug_query_margins(dhr_index* ix, const dhr_query_batch* qb, float* out_host, void* stream) try {
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (!out_host) return set_error(DHR_ERR_INVALID, "null output pointer");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  Workspace& w = ix->ws;
  if ((rc = ensure_ws(ix, w, qb->n_queries, 1, 0)) != DHR_OK) return rc;
  if ((rc = prep_queries(ix, w, qb, s)) != DHR_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_host, w.margin, (size_t)qb->n_queries * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

// Test hook: what ONE phase of a search does with rows [row_lo, row_hi) up to the exact rescoring -- the bound GEMM into the candidate LISTS (not its
// dump path: the entries the filter epilogue appends are what the refine level reads), then launch_refine on those lists with the arguments of
// search_core.hip (base_refine_args) -- and both lists scattered into dense [Q][row_hi - row_lo] arrays: U of the rows the filter listed, U2 of the
// rows the refine level kept, NaN elsewhere.  Uniform lists only (no second tier): the tiles of the range must fit both list depths.
namespace {
// entry i of query q's list (row, float bits) -> out[q][row - row_lo] where the row lies in the range (the tiles of a range may hold rows beside it)
__global__ void __launch_bounds__(256) scatter_list_kernel(const uint2* __restrict__ list, const uint32_t* __restrict__ cnt, uint32_t cap, int64_t row_lo,
                                                           int64_t row_hi, float* __restrict__ out) {
  const int q = blockIdx.y;
  const uint32_t count = cnt[q] < cap ? cnt[q] : cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    const uint2 e = list[(int64_t)q * cap + i];
    if ((int64_t)e.x >= row_lo && (int64_t)e.x < row_hi) out[(int64_t)q * (row_hi - row_lo) + ((int64_t)e.x - row_lo)] = __uint_as_float(e.y);
  }
}
hipError_t scatter_list(const uint2* list, const uint32_t* cnt, uint32_t cap, int Q, int64_t row_lo, int64_t row_hi, float* out, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out, 0xFF, (size_t)Q * (size_t)(row_hi - row_lo) * 4, s);      // 0xFFFFFFFF: a NaN
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(scatter_list_kernel, dim3(64, (unsigned)Q), dim3(256), 0, s, list, cnt, cap, row_lo, row_hi, out);
  return hipGetLastError();
}
}  // namespace
// tau_host: [Q] exact-score thresholds (the levels compare with thr = tau - margin, make_thr_kernel), or null: -inf, every row passes both levels.
// flat: 0 = one workgroup per (block of the longest list, query); 1 = flat launch over the block offsets with the grid of the controller that
// only enqueues; n > 1 = a flat launch of n workgroups (fewer than there are blocks: the rest by grid stride).  out_thr_host: [Q] thr, may be null;
// out_unit_host: [Q] score units of one gated operand product (RefineArgs::g8_unit; zeros where the gated half has no int8 image), may be null.
extern "C" int dhr_debug_refine_bounds(dhr_index* ix, const dhr_query_batch* qb, int64_t row_lo, int64_t row_hi, const float* tau_host, int32_t flat,
                                       float* out_u_dev, float* out_u2_dev, float* out_thr_host, float* out_unit_host, void* stream) try {
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (row_lo < 0 || row_hi > ix->n_rows || row_lo >= row_hi) return set_error(DHR_ERR_INVALID, "bad row range");
  if (!out_u_dev || !out_u2_dev) return set_error(DHR_ERR_INVALID, "null output pointer");
  if (flat < 0) return set_error(DHR_ERR_INVALID, "flat must be >= 0");
  const int Q = qb->n_queries;
  const bool gate = ix->d_dlr > 0 && qb->index != nullptr && qb->index_dtype != DHR_IDX_NONE;
  if (!uses_refine(ix, gate)) return set_error(DHR_ERR_UNSUPPORTED, "this batch has no refine level on this index");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  staged_set(ix, StagedState::None);          // the call overwrites the workspace of any staged search left open on this handle
  Workspace& w = ix->ws;
  if ((rc = ensure_ws(ix, w, Q, 1, 0)) != DHR_OK) return rc;
  const int64_t t_lo = row_lo / TILE_ROWS, t_hi = (row_hi + TILE_ROWS - 1) / TILE_ROWS;      // the tiles of the rows, in corpus order
  const int64_t listed = std::min<int64_t>(t_hi * TILE_ROWS, ix->n_rows) - t_lo * TILE_ROWS;  // rows a list can receive
  if (!w.cand_r || listed > std::min(w.cap, w.cap_r)) return set_error(DHR_ERR_INVALID, "row range deeper than the candidate lists");
  if ((rc = prep_queries(ix, w, qb, s)) != DHR_OK) return rc;
  if (tau_host) HIP_TRY(hipMemcpyAsync(w.tau, tau_host, (size_t)Q * 4, hipMemcpyHostToDevice, s));      // (else -inf: query_prep_kernel)
  HIP_TRY(launch_make_thr(w.tau, w.margin, Q, w.q_pad, w.thr, s));
  GemmArgs g = base_gemm_args(ix, w, Q);
  g.seq_lo = t_lo; g.seq_hi = t_hi; g.map_mode = 0; g.period = 1; g.head = 0;
  g.thr = w.thr; g.cand = w.cand; g.cnt = w.cnt;
  HIP_TRY(hipMemsetAsync(w.cnt, 0, (size_t)w.q_pad * 4, s));
  HIP_TRY(launch_gemm_filter(g, s));
  HIP_TRY(scatter_list(w.cand, w.cnt, (uint32_t)w.cap, Q, row_lo, row_hi, out_u_dev, s));
  RefineArgs f = base_refine_args(ix, w, Q, gate, w.thr);
  f.cand = w.cand; f.cnt = w.cnt;
  if (flat == 0) f.max_count = (uint32_t)listed;
  else {
    HIP_TRY(launch_block_offsets(w.cnt, (uint32_t)w.cap, Q, REFINE_PER_WG, w.blk_off, s));
    f.max_count = 1; f.blk_off = w.blk_off; f.flat_blocks = flat == 1 ? FLAT_GRID_ASYNC : (uint32_t)flat;
  }
  HIP_TRY(hipMemsetAsync(w.cnt_r, 0, (size_t)w.q_pad * 4, s));
  HIP_TRY(launch_refine(f, s));
  HIP_TRY(scatter_list(w.cand_r, w.cnt_r, (uint32_t)w.cap_r, Q, row_lo, row_hi, out_u2_dev, s));
  if (out_thr_host) HIP_TRY(hipMemcpyAsync(out_thr_host, w.thr, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
  if (out_unit_host && f.g8_unit) HIP_TRY(hipMemcpyAsync(out_unit_host, f.g8_unit, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (out_unit_host && !f.g8_unit) std::fill(out_unit_host, out_unit_host + Q, 0.f);
  return DHR_OK;
} DHR_CATCH_STATUS

// Test hook: ONE call of the running top-k merge, as every search ends its phases -- a SelectArgs filled from the arguments and handed to
// launch_select: the launcher, the dispatch by kp (select_kernel<4> / <16>, select_big_kernel, launch_select_global) and the LDS attribute
// handling are those of the searches.  No index handle: the lists, the keys and the thresholds are the caller's DEVICE arrays.  Whatever the
// kernels assume silently about their arguments is refused here, before a device is touched (the contract: SelectArgs, dhr_internal.h).
extern "C" int dhr_debug_select_merge(int32_t device, int32_t n_queries, int32_t k, int32_t k_keep, int32_t kp, int32_t kps, int32_t sort_n, int32_t monotone,
                                      uint64_t* topk_keys_dev, const uint64_t* in_keys_dev, int64_t ld_keys, const uint32_t* cnt_dev, uint32_t count_all,
                                      uint32_t cap, const float* margin_dev, float* tau_dev, float* thr_dev, void* stream) try {
  if (!topk_keys_dev || !in_keys_dev || !margin_dev || !tau_dev || !thr_dev) return set_error(DHR_ERR_INVALID, "null argument");
  if (n_queries <= 0) return set_error(DHR_ERR_INVALID, "n_queries must be positive");
  const auto pow2_in = [](int64_t v, int64_t lo, int64_t hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; };
  if (!pow2_in(kp, 64, 1 << 20)) return set_error(DHR_ERR_INVALID, "kp must be a power of two in [64, 1048576]");
  if (!pow2_in(kps, 64, kp)) return set_error(DHR_ERR_INVALID, "kps must be a power of two in [64, kp]");
  const int keep = k_keep ? k_keep : k;
  if (k < 1 || k > keep || keep > kps) return set_error(DHR_ERR_INVALID, "need 1 <= k <= k_keep <= kps");
  if (kp <= 4096 && (int64_t)sort_n - kps < 64) return set_error(DHR_ERR_INVALID, "sort_n leaves fewer than 64 keys of LDS behind the list");
  if (kp <= 4096 && (int64_t)sort_n * 8 + 16 > 160 * 1024) return set_error(DHR_ERR_INVALID, "sort_n keys do not fit the LDS (sort_n*8 + 16 B > 160 KiB)");
  if (kp > 16384 && n_queries > 65535) return set_error(DHR_ERR_INVALID, "more than 65535 queries on the global-memory path");
  if (ld_keys < 0) return set_error(DHR_ERR_INVALID, "ld_keys must not be negative");
  if (!cnt_dev && (int64_t)count_all > ld_keys) return set_error(DHR_ERR_INVALID, "count_all exceeds ld_keys");
  if ((int64_t)cap > ld_keys) return set_error(DHR_ERR_INVALID, "cap exceeds ld_keys");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  SelectArgs sel{};
  sel.topk_keys = topk_keys_dev; sel.in_keys = in_keys_dev; sel.ld_keys = ld_keys; sel.cnt = cnt_dev; sel.count_all = count_all; sel.cap = cap;
  sel.k = k; sel.kp = kp; sel.sort_n = sort_n; sel.k_keep = k_keep; sel.kps = kps; sel.monotone = monotone ? 1 : 0;
  sel.margin = margin_dev; sel.tau = tau_dev; sel.thr = thr_dev; sel.n_queries = n_queries;
  HIP_TRY(launch_select(sel, s));             // (a failure of the global path, e.g. hipCUB's 2^31 item limit, comes back as DHR_ERR_HIP)
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

// Test hook: how the main pass of the latest dhr_search on this handle seated its batch (seating.h).  Returns 1 and fills the host arrays ([n_slots] each,
// n_slots = the batch's query count rounded up to 256; any may be null) when that pass ran seated: slot -> query, query -> slot, the bound-list
// lengths of the sampled run the order was taken from, the slot-ordered threshold mirror and the thresholds themselves as the pass left them.
// Returns 0, and copies nothing, when every query sat where the caller put it.
extern "C" int dhr_debug_query_seating(dhr_index* ix, int32_t n_slots, int32_t* slot_q, int32_t* q_slot, uint32_t* lengths, float* thr_seat, float* thr_hat) try {
  if (!ix) return set_error(DHR_ERR_INVALID, "null index");
  HIP_TRY(hipSetDevice(ix->device));
  const Workspace& w = ix->ws;
  if (!w.seated || !w.seat_rec) return 0;
  if (n_slots != w.q_pad) return set_error(DHR_ERR_INVALID, "n_slots must be the padded query count of the latest search");
  HIP_TRY(hipDeviceSynchronize());
  const size_t b = (size_t)n_slots * 4;
  if (slot_q) HIP_TRY(hipMemcpy(slot_q, w.slot_q(), b, hipMemcpyDeviceToHost));
  if (q_slot) HIP_TRY(hipMemcpy(q_slot, w.q_slot(), b, hipMemcpyDeviceToHost));
  if (lengths) HIP_TRY(hipMemcpy(lengths, w.seat_len, b, hipMemcpyDeviceToHost));
  if (thr_seat) HIP_TRY(hipMemcpy(thr_seat, w.thr_seat(), b, hipMemcpyDeviceToHost));
  if (thr_hat) HIP_TRY(hipMemcpy(thr_hat, w.thr_hat, b, hipMemcpyDeviceToHost));
  return 1;
} DHR_CATCH_STATUS

// Kernel-tuning hook: the bound GEMM alone over the whole shard with the filter closed (thr = +inf),
// `iters` launches, average milliseconds per launch (hipEvents on the stream).
extern "C" void dhr_debug_seq_to_tile(int64_t seq, int32_t map_mode, int32_t period, int64_t head, int64_t perm_mul, int64_t perm_n, int64_t out[2]) try {
  out[0] = seq_to_tile_fast(seq, map_mode, period, head, perm_mul, perm_n, 1.0 / (double)(perm_n > 0 ? perm_n : 1), 1.0 / (double)(period > 1 ? period - 1 : 1));
  out[1] = seq_to_tile(seq, map_mode, period, head, perm_mul, perm_n);
} DHR_CATCH_VOID
extern "C" int dhr_debug_gemm_time(dhr_index* ix, const dhr_query_batch* qb, int32_t iters, double* ms_out, double* flops_out,
                                   void* stream) try {
  int rc = check_queries(ix, qb);
  if (rc) return rc;
  if (iters <= 0 || !ms_out) return set_error(DHR_ERR_INVALID, "bad iters / null pointer");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = (hipStream_t)stream;
  Workspace& w = ix->ws;
  // DHR_GEMM_TIME_OPEN=1 (tuning): filter with the final thresholds of the previous dhr_search on this handle (same queries),
  // i.e. a realistic hit rate in the epilogue, instead of the closed filter.  (The workspace must be the one that search left:
  // same k, or ensure_ws would re-allocate it and the thresholds would be uninitialised memory -- as they were for a while.)
  const bool open = getenv("DHR_GEMM_TIME_OPEN") && atoi(getenv("DHR_GEMM_TIME_OPEN")) != 0 && w.thr_hat && ix->stats.k > 0 && ix->stats.n_queries == qb->n_queries;
  if ((rc = ensure_ws(ix, w, qb->n_queries, open ? (int)ix->stats.k : 1, 0)) != DHR_OK) return rc;
  if ((rc = prep_queries(ix, w, qb, s)) != DHR_OK) return rc;
  if (open) {
    HIP_TRY(hipMemcpyAsync(w.thr, w.thr_hat, (size_t)w.q_pad * 4, hipMemcpyDeviceToDevice, s));
  } else {
    std::vector<float> inf((size_t)w.q_pad, INFINITY);
    HIP_TRY(hipMemcpyAsync(w.thr, inf.data(), (size_t)w.q_pad * 4, hipMemcpyHostToDevice, s));
  }
  const bool opened = open;
  HIP_TRY(hipMemsetAsync(w.cnt, 0, (size_t)w.q_pad * 4, s));
  GemmArgs g = base_gemm_args(ix, w, qb->n_queries);
  g.seq_lo = 0; g.seq_hi = ix->n_tiles; g.map_mode = 0; g.period = 1; g.head = 0;      // the whole shard, in corpus order
  g.thr = w.thr; g.cand = w.cand; g.cnt = w.cnt;
  HIP_TRY(launch_gemm_filter(g, s));                      // warm-up
  Events evs;
  hipEvent_t e0, e1;
  HIP_TRY(evs.add(&e0)); HIP_TRY(evs.add(&e1));
  HIP_TRY(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) {
    if (opened) HIP_TRY(hipMemsetAsync(w.cnt, 0, (size_t)w.q_pad * 4, s));       // the lists fill as in a search (a full list takes the cold surplus path)
    HIP_TRY(launch_gemm_filter(g, s));
  }
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  *ms_out = ms / iters;
  if (flops_out) *flops_out = 2.0 * (double)w.q_pad * (double)ix->n_tiles * TILE_ROWS * (double)ix->kt;
  return DHR_OK;
} DHR_CATCH_STATUS

// ------------------------------------------------------------------------------------------ shard reduce
extern "C" int dhr_merge_topk(int32_t device, int32_t n_queries, int32_t n_in, const float* in_scores,
                              const int64_t* in_rows, int32_t k_out, float* out_scores, int64_t* out_rows, void* stream) try {
  if (n_queries <= 0 || n_in <= 0 || k_out <= 0 || !in_scores || !in_rows || !out_scores || !out_rows)
    return set_error(DHR_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(device));
  if (n_in > 16384) {       // beyond one workgroup's LDS: two stable segmented sorts through global memory (select_global.hip)
    if ((int64_t)n_queries * n_in > (int64_t)0x7fffffff) return set_error(DHR_ERR_UNSUPPORTED, "more than 2^31 entries in one device reduce");
    HIP_TRY(launch_merge_topk_global(n_queries, n_in, in_scores, in_rows, k_out, out_scores, out_rows, (hipStream_t)stream));
    return DHR_OK;
  }
  HIP_TRY(launch_merge_topk(n_queries, n_in, in_scores, in_rows, k_out, out_scores, out_rows, (hipStream_t)stream));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_merge_topk_lists(int32_t device, int32_t n_queries, int32_t n_lists, int32_t list_len, const float* in_scores,
                                    const int64_t* in_rows, int32_t k_out, float* out_scores, int64_t* out_rows, void* stream) try {
  if (n_queries <= 0 || n_lists <= 0 || list_len <= 0 || k_out <= 0 || !in_scores || !out_scores || (in_rows && !out_rows))
    return set_error(DHR_ERR_INVALID, "bad argument");
  if (((int64_t)n_lists * list_len + k_out) * (in_rows ? 12 : 4) > 160 * 1024 || n_lists > 64)
    return set_error(DHR_ERR_UNSUPPORTED, "the lists of one query do not fit the LDS ((n_lists*list_len + k_out)*12 B > 160 KiB) or n_lists > 64");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_merge_lists(n_queries, n_lists, list_len, in_scores, in_rows, k_out, out_scores, in_rows ? out_rows : nullptr,
                             (hipStream_t)stream));
  return DHR_OK;
} DHR_CATCH_STATUS

// The two host merges: per query, the candidates at source positions src(q, 0 .. n_per_query) of the input arrays, those with a row >= 0 where
// there are rows, best first -- score key descending, then row ascending, then (by_position) source position -- and the first k_out of them, padded
// with (-inf, -1).  (+0 and -0 share a score key: without by_position two such entries of one row tie, and which comes first is the sort's matter.)
namespace {
template <typename Src>
void merge_topk_on_host(int n_queries, int64_t n_per_query, Src&& src, bool by_position, const float* in_scores, const int64_t* in_rows, int k_out,
                        float* out_scores, int64_t* out_rows) {
  std::vector<int64_t> order;
  for (int q = 0; q < n_queries; ++q) {
    order.clear();
    for (int64_t j = 0; j < n_per_query; ++j) {
      const int64_t at = src(q, j);
      if (!in_rows || in_rows[at] >= 0) order.push_back(at);
    }
    const int take = std::min<int>(k_out, (int)order.size());
    std::partial_sort(order.begin(), order.begin() + take, order.end(), [&](int64_t a, int64_t b) {
      const uint32_t ka = f32_ordered(in_scores[a]), kb = f32_ordered(in_scores[b]);
      if (ka != kb) return ka > kb;
      if (in_rows && in_rows[a] != in_rows[b]) return in_rows[a] < in_rows[b];
      return by_position && a < b;
    });
    for (int j = 0; j < k_out; ++j) {
      out_scores[(size_t)q * k_out + j] = j < take ? in_scores[order[j]] : -INFINITY;
      if (in_rows) out_rows[(size_t)q * k_out + j] = j < take ? in_rows[order[j]] : -1;
    }
  }
}
}  // namespace

// in_scores / in_rows [n_lists][n_queries][list_len]: source positions ascend by list, then by position in the list
extern "C" int dhr_merge_topk_lists_host(int32_t n_queries, int32_t n_lists, int32_t list_len, const float* in_scores,
                                         const int64_t* in_rows, int32_t k_out, float* out_scores, int64_t* out_rows) try {
  if (n_queries <= 0 || n_lists <= 0 || list_len <= 0 || k_out <= 0 || !in_scores || !out_scores || (in_rows && !out_rows))
    return set_error(DHR_ERR_INVALID, "bad argument");
  merge_topk_on_host(n_queries, (int64_t)n_lists * list_len, [&](int q, int64_t j) { return ((j / list_len) * n_queries + q) * list_len + j % list_len; },
                     true, in_scores, in_rows, k_out, out_scores, out_rows);
  return DHR_OK;
} DHR_CATCH_STATUS

// in_scores / in_rows [n_queries][n_in]
extern "C" int dhr_merge_topk_host(int32_t n_queries, int32_t n_in, const float* in_scores, const int64_t* in_rows,
                                   int32_t k_out, float* out_scores, int64_t* out_rows) try {
  if (n_queries <= 0 || n_in <= 0 || k_out <= 0 || !in_scores || !in_rows || !out_scores || !out_rows)
    return set_error(DHR_ERR_INVALID, "bad argument");
  merge_topk_on_host(n_queries, n_in, [&](int q, int64_t j) { return (int64_t)q * n_in + j; }, false, in_scores, in_rows, k_out, out_scores, out_rows);
  return DHR_OK;
} DHR_CATCH_STATUS

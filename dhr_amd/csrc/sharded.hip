// Row-sharded search behind the C ABI: the corpus is split over ranks exactly like the reference's
// --total_shrad / --shrad (retrieval/gip_retrieval.py:292-306), queries are replicated, every shard searches its rows and the
// per-shard lists are reduced to the global top-k -- retrieval/merge.result.py:22-42 without the text files.
//
//   dhr_search_sharded        one process per GPU: this rank's shard + a dhr_comm (an RCCL communicator: librccl linked directly,
//                             all-gathers over xGMI)
//   dhr_search_sharded_local  one process, several shards (handles on one or more devices): the same control flow with the
//                             all-gather done by device copies -- also what the single-GPU tests drive
//
//   dhr_search_sharded_host   the same control flow over caller-supplied host shards and a caller-supplied all-gather (no device):
//                             what the CPU test-suite drives with world size 2 / 3 over gloo
//
// All run ONE implementation (sharded_core) over a Backend.  Sequence (collectives on the caller's stream):
//   1. every shard runs its sampled pass (dhr_search_begin) and holds the r best exact sample scores per query;
//   2. all-gather of [Q, r] fp32; the r-th best of the union is the common threshold tau_q, so a shard collects only ITS SHARE
//      of the global top-k (rank merge of the sorted lists in place, dhr_merge_topk_lists without rows);
//   2b. second agreement (dhr_search_mid; skipped where a shard is too small for it): every shard runs the first slice of
//      its main pass with tau, all-gather of its best scores seen so far [Q, r2] fp32, tau_q = max(tau_q, the (k f + 6 sigma + 4)-th best of
//      the union) -- f = the scattered fraction of the corpus the shards have seen by then;
//   3. rest of the main pass with tau (dhr_search_finish) -> sorted per-shard lists + the count of rows reaching tau (-1: list overflow);
//   4. all-gather of the counts [Q] int32: a query is complete iff the union holds >= k rows, no shard overflowed and no shard's
//      share exceeds the gathered prefix; failures are flagged ON THE DEVICE (identically on every rank);
//   5. all-gather of the list prefixes [Q, kk] (kk = a fixed fraction of k by world size: no host read decides it) and the
//      rank merge of the sorted lists (dhr_merge_topk_lists) -> the global [Q, k];
//   6. ONE host read (the number of failed queries); failed queries (unrepresentative sample, skewed shards) are redone with
//      purely local thresholds (dhr_search on the sub-batch), gathered at full length and scattered into the result.
// Shards that cannot be sampled uniformly (tiny or unequal shards, k > rows of a shard) take the local-threshold path for
// the whole batch.  Results are bit-identical to the unsharded search (exact scores, ties by global row).
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dhr_internal.h"
#include "sharded_plan.h"

struct dhr_comm {
  ncclComm_t comm = nullptr;      // RCCL (dhr_comm_create / dhr_comm_wrap), or
  dhr_allgather_fn cb = nullptr;  // ... a host transport supplied by the caller (dhr_comm_create_callback): HOST buffers
  void* cb_user = nullptr;
  bool owned = false;
  int world = 1, rank = 0, device = 0;
  void* arena = nullptr;          // grow-only device scratch
  size_t arena_bytes = 0;
  void* h_stage = nullptr;        // pinned staging of the callback transport: [send | recv]
  size_t h_stage_bytes = 0;
  bool dead = false;              // dhr_comm_abort ran: the handle only waits for dhr_comm_destroy
};


namespace {

using namespace dhr;
using namespace dhr::sharded;      // sharded_plan.h: Block, ListBlock, RankVote, StepPlan -- every block of a step is laid out there

#define SH_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return dhr_set_error_message(DHR_ERR_HIP, (std::string(#x) + ": " + hipGetErrorString(e_)).c_str()); } while (0)
#define SH_NCCL(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return dhr_set_error_message(DHR_ERR_HIP, (std::string(#x) + ": " + ncclGetErrorString(r_)).c_str()); } while (0)
#define SH_TRY(x) do { int rc_ = (x); if (rc_ != DHR_OK) return rc_; } while (0)

// ------------------------------------------------------------------------------------------------------------------------------------
// The sharded search is ONE control flow (sharded_core below) over a Backend: where the shards live, how their blocks are
// gathered, and the handful of per-query reductions between the collectives.  Two backends:
//   HipBackend   shards = dhr_index handles on GPUs; gathers = RCCL all-gathers (one process per GPU), a caller-supplied host
//                transport (dhr_comm_create_callback: torch.distributed over gloo, MPI, ...), or device copies (one process,
//                several shards); reductions = the kernels of this file and kernels.hip.  The product.
//   HostBackend  shards = caller-supplied callbacks on host memory, gathers = a caller-supplied callback, reductions = plain
//                loops (dhr_merge_topk_lists_host).  No device is touched: it exists so that the CPU test-suite can drive
//                THIS control flow with world size 2 / 3 over gloo (tests/test_dist_gloo.py) -- until round 4 those tests ran
//                a torch restatement of it (dhr_amd/dist.py sharded_search_torch, now deleted).
// ------------------------------------------------------------------------------------------------------------------------------------
// Every block of an all-gather ends in a status record (Block, sharded_plan.h).  The record is what makes a failed step COLLECTIVE (round 6): a rank whose local work failed (a HIP error, out of memory, a failing shard callback) does not leave
// the sequence of collectives -- it skips its remaining local work, keeps issuing the step's all-gathers with the agreed sizes, and its status
// travels in the record of every block it sends.  A transport whose blocks pass through host memory (the caller's host transport, host shards)
// reads the records right behind each gather and every rank returns from the SAME gather; over RCCL (and in the one-process form) the records are
// folded on the device into the word that the step's one host read fetches anyway, and every rank returns at the end of the step.  The failing
// rank returns its own status and message, the others DHR_ERR_PEER naming it.  (Until round 5 the failing rank returned at once and the others
// waited in their next collective for the transport's timeout.)
// first failing rank of a gathered buffer in HOST memory (0: none)
inline int host_block_status(const void* blocks, int world, const Block& b, int* who) {
  for (int w = 0; w < world; ++w) {
    int32_t st;
    memcpy(&st, (const char*)blocks + (size_t)w * b.stride + b.payload, 4);
    if (st != 0) { *who = w; return st; }
  }
  return 0;
}
inline int peer_error(int who, int status) {
  char buf[160];
  snprintf(buf, sizeof(buf), "rank %d failed in this sharded step (its status: %d); the step was abandoned on every rank", who, status);
  return dhr_set_error_message(DHR_ERR_PEER, buf);
}

struct Backend {
  int world = 1, n_local = 1;
  virtual ~Backend() {}
  virtual void* alloc(int i, size_t bytes) = 0;                 // scratch in local shard i's memory, released when the call ends
  virtual int zero(int i, void* p, size_t bytes) = 0;
  virtual int set_share(int i, int share) = 0;                  // DHR_PARAM_SAMPLE_SHARE
  virtual void abort(int) {}                                    // forget a staged search that did not reach its finish call
  virtual int sample_rank(int i, int k) = 0;
  virtual int union_rank(int i, int k) = 0;
  virtual int begin(int i, const dhr_query_batch* qb, int k, float* sample) = 0;
  virtual int finish(int i, const float* tau, float* ls, int64_t* lr, int32_t* cnt) = 0;
  // the (local, union) ranks of an optional agreement: MID the second agreement (dhr_search_mid_ranks / dhr_search_mid), PRE the first agreement in
  // two rounds (dhr_search_pre_ranks / dhr_search_pre / dhr_search_begin_rest); r_local 0: the shard has no such step
  enum Stage { MID, PRE };
  virtual int stage_ranks(int i, Stage stage, int k, int* r_local, int* r_union) = 0;
  virtual int mid(int i, const float* tau, int r_local, float* scores) = 0;
  virtual int pre(int i, const dhr_query_batch* qb, int k, int r_local, float* scores) = 0;
  virtual int begin_rest(int i, const float* tau, float* sample) = 0;
  virtual int search(int i, const dhr_query_batch* qb, int k, float* s, int64_t* r) = 0;
  // the status record of local shard i's outgoing block
  virtual int put_status(int i, void* block, const Block& b, int status) = 0;
  // all-gather of one block per shard: send[i] (local shard i's block, b.stride bytes) -> recv[i] = [world][b.stride] in local shard i's memory.
  // A transport whose blocks pass through host memory returns DHR_ERR_PEER here when some rank's record carries a failure.
  virtual int gather(const std::vector<const void*>& send, const std::vector<void*>& recv, const Block& b) = 0;
  // ... the others fold the records of a gathered buffer into rec[1] (status of the first failing rank) / rec[2] (that rank), on the device
  virtual int fold_status(int i, const void* gathered, const Block& b, int32_t* rec) = 0;
  // the 48 bytes of this process's rank vote -> all = [world][48 bytes] in HOST memory (SPMD only); one host read
  virtual int exchange_vote(const RankVote& mine, int32_t* all) = 0;
  // gathered [world] blocks of [Q, r] sorted sample scores -> tau[q] = the ru-th best of the union; raise: tau[q] = max(tau[q], that)
  virtual int union_threshold(int i, const float* gathered, const Block& b, int Q, int r, int ru, float* tau, bool raise) = 0;
  // counts [world] blocks of [Q] -> compact list of failed query ids + their number in rec[0] (a query is complete iff the union holds >= k rows,
  // no shard overflowed (-1) and no shard's share exceeds the gathered prefix kk)
  virtual int flag_failures(int i, const int32_t* counts, const Block& b, int Q, int k, int kk, int32_t* fail_ids, int32_t* rec) = 0;
  virtual int prefix(int i, const float* s, const int64_t* r, int k, int kk, int Q, float* os, int64_t* orow) = 0;
  // [world] blocks holding a query-major [Q, L] score section (gs) and row section (gr) each, sorted lists -> [Q, k]
  virtual int merge(int i, int Q, int L, const float* gs, const int64_t* gr, const Block& b, int k, float* os, int64_t* orow) = 0;
  // THE host read: rec[0] failed queries (+ their ids), rec[1] / rec[2] the first failing rank's status / rank (0: none)
  virtual int read_failed(const std::vector<int32_t*>& rec, const std::vector<int32_t*>& fail_ids, std::vector<int32_t>& ids, int* peer_status, int* peer_rank) = 0;
  virtual int sub_batch(int i, const dhr_query_batch* in, const std::vector<int32_t>& ids, dhr_query_batch* out, int32_t** ids_mem) = 0;
  virtual int scatter(int i, const float* s, const int64_t* r, const int32_t* ids_mem, int F, int k, float* os, int64_t* orow) = 0;
};

// The rank agreement on the wire: ONE exchange of 48 bytes per process, reduced by RankVote::reduce.  No allocation precedes the exchange for up to 64
// ranks (a rank that could not allocate must still be able to say so: vote_status_only).
int reduce_over_ranks(Backend& B, RankVote& vote) {
  if (B.world <= B.n_local) return DHR_OK;         // one process: nobody to agree with
  int32_t few[64 * RankVote::SLOTS];
  std::vector<int32_t> many;
  if (B.world > 64) many.resize((size_t)B.world * RankVote::SLOTS);
  int32_t* all = B.world > 64 ? many.data() : few;
  SH_TRY(B.exchange_vote(vote, all));
  vote.reduce(all, B.world);
  return DHR_OK;
}
// The vote of a rank that has nothing to report but a failure: it takes part in the exchange the others are about to enter (or are waiting in) with its
// status and zero ranks, so that every rank abandons the step there.  Never throws; keeps the thread's error message.
void vote_status_only(Backend& B, int status) noexcept {
  char keep[1024];
  snprintf(keep, sizeof(keep), "%s", dhr_last_error());
  try {
    RankVote vote = RankVote::status_only(status);
    (void)reduce_over_ranks(B, vote);
  } catch (...) {
  }
  (void)dhr_set_error_message(status, keep);
}

// host-side pieces shared by both backends ------------------------------------------------------------------------------------------
void host_flag_failures(const int32_t* counts, const Block& b, int world, int Q, int k, int kk, int32_t* fail_ids, int32_t* n_failed) {
  int nf = 0;
  for (int q = 0; q < Q; ++q) {
    int64_t tot = 0;
    bool bad = false;
    for (int w = 0; w < world; ++w) {
      const int32_t c = ((const int32_t*)((const char*)counts + (size_t)w * b.stride))[q];
      if (c < 0 || c > kk) bad = true;
      tot += c > 0 ? c : 0;
    }
    if (bad || tot < k) fail_ids[nf++] = q;
  }
  *n_failed = nf;
}
// rows `ids` of a HOST query batch, gathered into `v` / `x`
void host_sub_batch(const dhr_query_batch* in, const std::vector<int32_t>& ids, std::vector<char>& v, std::vector<char>& x, dhr_query_batch* out) {
  const int vsz = in->value_dtype == DHR_VAL_F32 ? 4 : 2, isz = in->index_dtype == DHR_IDX_I16 ? 2 : 1;
  const int64_t vrow = in->ld_value * vsz, irow = in->index ? in->ld_index * isz : 0;
  const int F = (int)ids.size();
  v.resize((size_t)F * vrow);
  for (int f = 0; f < F; ++f) memcpy(v.data() + (size_t)f * vrow, (const char*)in->value + (size_t)ids[f] * vrow, vrow);
  if (in->index) {
    x.resize((size_t)F * irow);
    for (int f = 0; f < F; ++f) memcpy(x.data() + (size_t)f * irow, (const char*)in->index + (size_t)ids[f] * irow, irow);
  }
  *out = *in;
  out->n_queries = F;
  out->value = v.data();
  out->index = in->index ? x.data() : nullptr;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The state of ONE sharded step: which local shard has failed (and with what message), and the device record the status words of the
// gathered blocks are folded into.
struct Step {
  Backend& B;
  const bool spmd;                 // other processes take part in the collectives: a local failure must not leave their sequence
  std::vector<int> st;             // first failure of local shard i (DHR_OK: none); its later local work is skipped
  std::vector<int32_t*> rec;       // per local shard: {failed queries, first failing rank's status, that rank, -} in the shard's memory
  char msg[1024];                  // dhr_last_error() of the first local failure (later calls overwrite the thread's record)
  std::vector<const void*> send;   // per local shard: the block it sends in the all-gather at hand, and where the [world] blocks arrive (open())
  std::vector<void*> recv;
  // What this rank still OWES the others (a failure OUTSIDE the local work -- a std::bad_alloc in the control flow, a block that cannot be allocated -- must
  // not leave them in their next collective until the transport's timeout): the rank agreement, one exchange of a fixed size, then the all-gathers that
  // follow from the agreed ranks (StepPlan, fixed storage).  leave() pays the debt with this rank's status in every block.
  StepPlan plan;
  int done = 0;                    // how many of the planned all-gathers have been issued
  bool agreed = false;             // the rank agreement has been issued (successfully or not: it is never issued twice)
  bool over = false;               // the step is over on EVERY rank at this point of the sequence (a failure all of them have just read in the same
                                   // exchange) or the transport itself failed: no further collective may be issued
  explicit Step(Backend& b) : B(b), spmd(b.world > b.n_local), st(b.n_local, DHR_OK), rec(b.n_local, nullptr), send(b.n_local), recv(b.n_local) { msg[0] = 0; }
  // scratch of local shard i; THE out-of-memory message of the control flow
  template <class T> int alloc(int i, size_t bytes, T** p) {
    *p = (T*)B.alloc(i, bytes);
    return *p ? DHR_OK : dhr_set_error_message(DHR_ERR_HIP, "out of memory in the sharded search");
  }
  // local shard i's block `b` of the all-gather at hand (-> *blk, send[i]) and its receive buffer (-> recv[i])
  template <class T> int open(int i, const Block& b, T** blk) {
    SH_TRY(alloc(i, b.stride, blk));
    send[i] = *blk;
    return alloc(i, (size_t)B.world * b.stride, &recv[i]);
  }
  // The way out of a step that failed with `status`.  SPMD: a local failure never leaves the sequence -- the vote with the status if it is still owed, else
  // every planned all-gather not yet issued, with the status in its record (host transports end the step on every rank at the first such gather; with
  // device-side records the others run the plan to its end and read it there).  Nothing once `over` is set.  Never throws; keeps the thread's message.
  void leave(int status) noexcept {
    if (!spmd || status == DHR_OK || over) return;
    if (!agreed) { agreed = true; vote_status_only(B, status); return; }
    char keep[1024];
    snprintf(keep, sizeof(keep), "%s", dhr_last_error());
    try {
      while (done < plan.n) {
        const Block& b = plan.block(plan.order[done]);
        bool ok = true;
        for (int i = 0; i < B.n_local && ok; ++i) {
          void* blk = nullptr;
          ok = open(i, b, &blk) == DHR_OK && B.zero(i, blk, b.stride) == DHR_OK && B.put_status(i, blk, b, st[i] != DHR_OK ? st[i] : status) == DHR_OK;
        }
        if (!ok) break;
        ++done;
        if (B.gather(send, recv, b) != DHR_OK) { over = true; break; }
      }
    } catch (...) {
    }
    (void)dhr_set_error_message(status, keep);
  }
  int own() const { for (int v : st) if (v != DHR_OK) return v; return DHR_OK; }
  int own_error() const { return dhr_set_error_message(own(), msg); }
  // local work of shard i.  A failure is recorded; in a one-process search (nobody else is waiting) it ends the step at once.
  template <class F> int local(int i, F&& op) {
    if (st[i] != DHR_OK) return DHR_OK;
    int rc;
    try { rc = op(); } catch (...) { rc = dhr::on_exception(); }
    if (rc == DHR_OK) return DHR_OK;
    if (!spmd) return rc;
    if (own() == DHR_OK) snprintf(msg, sizeof(msg), "%s", dhr_last_error());
    st[i] = rc;
    return DHR_OK;
  }
  int init() {
    for (int i = 0; i < B.n_local; ++i) { SH_TRY(alloc(i, 256, &rec[i])); SH_TRY(B.zero(i, rec[i], 16)); }
    return DHR_OK;
  }
  // the planned all-gather `name` of the opened blocks, status records included; that it is the NEXT one the plan lists is an internal check
  int gather(StepPlan::Name name) {
    if (done >= plan.n || plan.order[done] != name)
      return dhr_set_error_message(DHR_ERR_INTERNAL, "sharded step: an all-gather does not match the step's plan");
    const Block& b = plan.block(name);
    for (int i = 0; i < B.n_local; ++i) SH_TRY(B.put_status(i, const_cast<void*>(send[i]), b, st[i]));
    ++done;
    const int rc = B.gather(send, recv, b);
    // host-visible transports end the step on EVERY rank at the first gather that carries a failure (or the transport broke): no collective after it;
    // device-side records are folded below and read in the step's one host read
    if (rc != DHR_OK) over = true;
    if (rc == DHR_ERR_PEER && own() != DHR_OK) return own_error();      // this rank is the one that failed
    SH_TRY(rc);
    for (int i = 0; i < B.n_local; ++i) SH_TRY(B.fold_status(i, recv[i], b, rec[i]));
    return DHR_OK;
  }
  // the verdict of a step whose status words travelled on the device (peer_status / peer_rank from the host read)
  int verdict(int peer_status, int peer_rank) const {
    return own() != DHR_OK ? own_error() : peer_status != 0 ? peer_error(peer_rank, peer_status) : DHR_OK;
  }
};
#define SH_LOCAL(i, expr) SH_TRY(S.local(i, [&]() -> int { return (expr); }))

// DHR_PARAM_SAMPLE_SHARE is handle state: the sharded entry points set it for their own staged calls and put 1 back on EVERY way out, so that a later
// dhr_search_begin / finish on the same handle does not inherit a stale share; and a step that failed between begin and finish (arena out of memory, a
// transport error, a failed mid step) must not leave the handle "pending": dhr_score_rows refuses one.  After a completed step the abort is a no-op.
struct ShareGuard {
  Backend& B;
  ~ShareGuard() { for (int i = 0; i < B.n_local; ++i) { (void)B.set_share(i, 1); B.abort(i); } }
};

thread_local int g_last_repairs = 0;      // queries the calling thread's last sharded search redid with local thresholds (dhr_debug_sharded_repairs)

// ---- the steps of the driver (sharded_body), in the order of the sequence at the top of this file ---------------------------------------------------
// Agree on the ranks: every shard reports (r, ru) and its optional mid / pre ranks, the processes exchange ONE RankVote (sharded_plan.h says what
// survives).  Not cached: the answer depends on every rank's shard size and sample period, a communicator outlives the index handles, and a rank
// that hit a cache the others missed would skip a collective they issue.
int agree_ranks(Step& S, int k, Ranks* agreed) {
  Backend& B = S.B;
  std::vector<ShardRanks> mine(B.n_local);
  for (int i = 0; i < B.n_local; ++i) {
    mine[i].r = B.sample_rank(i, k);
    mine[i].ru = B.union_rank(i, k);
    SH_LOCAL(i, B.stage_ranks(i, Backend::MID, k, &mine[i].rl_mid, &mine[i].ru_mid));
    SH_LOCAL(i, B.stage_ranks(i, Backend::PRE, k, &mine[i].rl_pre, &mine[i].ru_pre));
  }
  RankVote vote = RankVote::pack(mine.data(), B.n_local, S.own());
  S.agreed = true;
  { const int rc_x = reduce_over_ranks(B, vote); if (rc_x != DHR_OK) { S.over = true; return rc_x; } }
  *agreed = vote.unpack();
  if (agreed->status == DHR_OK) return DHR_OK;
  S.over = true;                                      // every rank reads the same status and leaves here
  return S.own() != DHR_OK ? S.own_error() : dhr_set_error_message(DHR_ERR_PEER, "another rank failed while setting up this sharded step; the step was abandoned on every rank");
}

// One threshold agreement (steps 1a, 1-2 and 2b are this round): every shard's `fill(i, scores)` writes its r_local best scores per query into its
// block `name` of the plan, the blocks are gathered, and the r_union-th best of the union becomes tau (raise: tau only rises to it).
template <class Fill>
int score_round(Step& S, StepPlan::Name name, int r_local, int r_union, bool raise, const std::vector<float*>& tau, Fill&& fill) {
  Backend& B = S.B;
  const Block& b = S.plan.block(name);
  for (int i = 0; i < B.n_local; ++i) {
    float* scores = nullptr;
    SH_TRY(S.open(i, b, &scores));
    SH_LOCAL(i, fill(i, scores));
  }
  SH_TRY(S.gather(name));
  for (int i = 0; i < B.n_local; ++i) SH_LOCAL(i, B.union_threshold(i, (const float*)S.recv[i], b, S.plan.Q, r_local, r_union, tau[i], raise));
  return DHR_OK;
}

// 3-5: main passes; ONE all-gather of [counts | list prefixes: scores | rows] per shard, failure flags, reduce
int main_pass(Step& S, const std::vector<float*>& tau, std::vector<int32_t*>& fail_ids, float* const* out_s, int64_t* const* out_r) {
  Backend& B = S.B;
  const ListBlock& L = S.plan.final_;
  const int nl = B.n_local, Q = S.plan.Q, k = S.plan.k, kk = S.plan.kk;
  for (int i = 0; i < nl; ++i) {
    char* blk = nullptr;
    SH_TRY(S.open(i, L.b, &blk));
    SH_TRY(S.alloc(i, (size_t)Q * 4, &fail_ids[i]));
    float* ls = L.scores(blk);                   // kk == k: the full lists ARE the prefixes, straight into the block
    int64_t* lr = L.rows(blk);
    if (kk < k) { SH_TRY(S.alloc(i, (size_t)Q * k * 4, &ls)); SH_TRY(S.alloc(i, (size_t)Q * k * 8, &lr)); }
    SH_LOCAL(i, B.finish(i, tau[i], ls, lr, L.counts(blk)));
    if (kk < k) SH_LOCAL(i, B.prefix(i, ls, lr, k, kk, Q, L.scores(blk), L.rows(blk)));
  }
  SH_TRY(S.gather(StepPlan::FINAL));
  for (int i = 0; i < nl; ++i) {
    SH_LOCAL(i, B.flag_failures(i, L.counts(S.recv[i]), L.b, Q, k, kk, fail_ids[i], S.rec[i]));
    SH_LOCAL(i, B.merge(i, Q, kk, L.scores(S.recv[i]), L.rows(S.recv[i]), L.b, k, out_s[i], out_r[i]));
  }
  return DHR_OK;
}

// local thresholds for a (sub-)batch: every shard searches with k, full lists gathered (ONE all-gather: scores and rows in one block, `name` of the
// plan) and merged.  out_* [L.Q, k] per local shard.
int local_path(Step& S, StepPlan::Name name, const ListBlock& L, const std::vector<dhr_query_batch>& qb, float* const* out_s, int64_t* const* out_r) {
  Backend& B = S.B;
  const int nl = B.n_local, k = L.L;
  for (int i = 0; i < nl; ++i) {
    char* blk = nullptr;
    SH_TRY(S.open(i, L.b, &blk));
    SH_LOCAL(i, B.search(i, &qb[i], k, L.scores(blk), L.rows(blk)));
  }
  SH_TRY(S.gather(name));
  for (int i = 0; i < nl; ++i) SH_LOCAL(i, B.merge(i, L.Q, k, L.scores(S.recv[i]), L.rows(S.recv[i]), L.b, k, out_s[i], out_r[i]));
  return DHR_OK;
}

// 6, second half: the failed queries `ids` (unrepresentative sample, skewed shards) as a sub-batch with local thresholds, gathered at full length and
// scattered into the result.  Ends with the step's second (and last) host read.
int repair(Step& S, const dhr_query_batch* qb_in, std::vector<int32_t>& ids, float* const* out_s, int64_t* const* out_r) {
  Backend& B = S.B;
  const int nl = B.n_local, k = S.plan.k, F = (int)ids.size();
  S.plan.add_repair(F);                                  // the repair step's all-gather (every rank read the same F)
  std::sort(ids.begin(), ids.end());                     // the ids come out of an atomic append on the device: sorted, every rank and shard holds the same order
  std::vector<dhr_query_batch> sub(nl, *qb_in);
  std::vector<float*> fs(nl);
  std::vector<int64_t*> fr(nl);
  std::vector<int32_t*> ids_mem(nl);
  for (int i = 0; i < nl; ++i) {
    SH_LOCAL(i, B.sub_batch(i, qb_in, ids, &sub[i], &ids_mem[i]));
    SH_TRY(S.alloc(i, (size_t)F * k * 4, &fs[i]));
    SH_TRY(S.alloc(i, (size_t)F * k * 8, &fr[i]));
    if (S.st[i] != DHR_OK) sub[i].n_queries = F;            // (a shard that failed before it built its sub-batch still sizes its blocks by F)
  }
  for (int i = 0; i < nl; ++i) SH_TRY(B.zero(i, S.rec[i], 16));
  SH_TRY(local_path(S, StepPlan::REPAIR, S.plan.repair, sub, fs.data(), fr.data()));
  for (int i = 0; i < nl; ++i) SH_LOCAL(i, B.scatter(i, fs[i], fr[i], ids_mem[i], F, k, out_s[i], out_r[i]));
  int peer_status = 0, peer_rank = 0;
  std::vector<int32_t> none;
  SH_TRY(B.read_failed(S.rec, {}, none, &peer_status, &peer_rank));      // (no ids to read; synchronises every local shard)
  return S.verdict(peer_status, peer_rank);
}

// The driver: one sharded step, as the sequence at the top of this file.  The step has exactly ONE host read (read_failed), plus one more only when a
// repair step runs; nothing here synchronises a stream, allocates device memory outside the arenas or copies synchronously.
int sharded_body(Step& S, const dhr_query_batch* qb_in, int k, float* const* out_s, int64_t* const* out_r) {
  Backend& B = S.B;
  const int nl = B.n_local, Q = qb_in->n_queries;
  ShareGuard share_guard{B};                                            // share back to 1, pending staged search aborted: on every way out
  std::vector<dhr_query_batch> qb(nl, *qb_in);
  for (int i = 0; i < nl; ++i) SH_LOCAL(i, B.set_share(i, B.world));    // a shard chases only its share of the union's rank
  Ranks ranks;
  SH_TRY(agree_ranks(S, k, &ranks));
  // Between the agreement and this line nothing may fail or allocate: from here on Step::leave knows the all-gathers this rank owes.
  S.plan = StepPlan(Q, k, B.world, ranks);
  const StepPlan& P = S.plan;
  SH_TRY(S.init());
  std::vector<int32_t*> fail_ids(nl, nullptr);
  std::vector<int32_t> ids;
  // BEFORE the first gather: the read behind the last planned one must not allocate (a rank that failed THERE would not know whether the others repair)
  ids.reserve((size_t)Q);
  int peer_status = 0, peer_rank = 0;
  if (!P.sampled) {                // shards that cannot be sampled alike: local thresholds for the whole batch
    SH_TRY(local_path(S, StepPlan::LOCAL, P.local, qb, out_s, out_r));
    SH_TRY(B.read_failed(S.rec, fail_ids, ids, &peer_status, &peer_rank));
    return S.verdict(peer_status, peer_rank);
  }
  std::vector<float*> tau(nl);
  for (int i = 0; i < nl; ++i) SH_TRY(S.alloc(i, (size_t)Q * 4, &tau[i]));
  if (P.has_pre) {
    // 1a: the first part of every shard's sample, a first common threshold from the union of the parts, the rest of the samples filtered at it
    std::vector<float*> tau0(nl);
    for (int i = 0; i < nl; ++i) SH_TRY(S.alloc(i, (size_t)Q * 4, &tau0[i]));
    SH_TRY(score_round(S, StepPlan::PRE, P.r_pre, P.ru0, false, tau0, [&](int i, float* scores) { return B.pre(i, &qb[i], k, P.r_pre, scores); }));
    SH_TRY(score_round(S, StepPlan::SAMPLE, P.r, P.ru, false, tau, [&](int i, float* scores) { return B.begin_rest(i, tau0[i], scores); }));
  } else      // 1-2: sampled passes, common thresholds
    SH_TRY(score_round(S, StepPlan::SAMPLE, P.r, P.ru, false, tau, [&](int i, float* scores) { return B.begin(i, &qb[i], k, scores); }));
  // 2b: second agreement.  Every shard runs the first slice of its main pass with tau and reports its best scores seen so far; the threshold of the rest
  // of the pass only rises to the union's (the counts are taken against it).  What 1a and 2b buy: DESIGN.md section 5.
  if (P.has_mid) SH_TRY(score_round(S, StepPlan::MID, P.r_mid, P.ru2, true, tau, [&](int i, float* scores) { return B.mid(i, tau[i], P.r_mid, scores); }));
  SH_TRY(main_pass(S, tau, fail_ids, out_s, out_r));
  // 6: the one host read; identical on every rank (it is a function of the gathered counts and status records)
  SH_TRY(B.read_failed(S.rec, fail_ids, ids, &peer_status, &peer_rank));
  if (peer_status != 0) return S.verdict(peer_status, peer_rank);      // a failure from before the last gather: every rank reads the same record
  g_last_repairs = (int)ids.size();
  // (a failure of THIS rank behind the last gather -- its reduce -- is unknown to the others: without a repair step there is no collective left
  // and it just reports it; with one it keeps to the sequence and its status travels in that gather)
  if (ids.empty()) return S.verdict(0, 0);
  return repair(S, qb_in, ids, out_s, out_r);
}

// The step and its way out: whatever the body returns or throws, a failing rank does not leave the others waiting (Step::leave).  out_s / out_r: one [Q, k]
// device (host shards: host) array per LOCAL shard.
int sharded_core(Backend& B, const dhr_query_batch* qb_in, int k, float* const* out_s, int64_t* const* out_r) {
  g_last_repairs = 0;
  int rc;
  try {
    Step S(B);
    try {
      dhr::alloc_checkpoint();
      rc = sharded_body(S, qb_in, k, out_s, out_r);
    } catch (...) {
      rc = dhr::on_exception();
    }
    S.leave(rc);
    return rc;
  } catch (...) {          // the step's own state could not be built: nothing has been exchanged yet
    rc = dhr::on_exception();
  }
  if (B.world > B.n_local) vote_status_only(B, rc);
  return rc;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// HipBackend
// out[i] = column `col` of in [n, ld]; raise: out[i] = max(out[i], that)
__global__ void column_kernel(const float* __restrict__ in, int ld, int col, int n, float* __restrict__ out, bool raise) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = in[(int64_t)i * ld + col];
  out[i] = raise ? fmaxf(out[i], v) : v;
}
// counts [world][Q] -> compact list of failed query ids, their number
// the status records of a gathered buffer -> rec[1] / rec[2] = status / rank of the first failing rank (kept once set)
__global__ void fold_status_kernel(const char* __restrict__ gathered, int world, size_t stride, size_t payload, int32_t* __restrict__ rec) {
  if (threadIdx.x != 0 || rec[1] != 0) return;
  for (int w = 0; w < world; ++w) {
    const int32_t st = *(const int32_t*)(gathered + (size_t)w * stride + payload);
    if (st != 0) { rec[1] = st; rec[2] = w; return; }
  }
}
__global__ void fail_kernel(const int32_t* __restrict__ counts, size_t stride, int world, int n_queries, int k, int kk, int32_t* __restrict__ fail_ids,
                            int32_t* __restrict__ n_failed) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_queries) return;
  int64_t tot = 0;
  bool bad = false;
  for (int w = 0; w < world; ++w) {
    const int32_t c = ((const int32_t*)((const char*)counts + (size_t)w * stride))[q];
    if (c < 0 || c > kk) bad = true;
    tot += c > 0 ? c : 0;
  }
  if (bad || tot < k) fail_ids[atomicAdd(n_failed, 1)] = q;
}
__global__ void prefix_kernel(const float* __restrict__ s, const int64_t* __restrict__ r, int k, int kk, int n_queries, float* __restrict__ os,
                              int64_t* __restrict__ orow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_queries * kk) return;
  const int q = (int)(i / kk), j = (int)(i - (int64_t)q * kk);
  os[i] = s[(int64_t)q * k + j];
  orow[i] = r[(int64_t)q * k + j];
}
__global__ void gather_rows_bytes_kernel(const char* __restrict__ src, int64_t stride, int row_bytes, const int32_t* __restrict__ ids, int n,
                                         char* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * row_bytes) return;
  const int r = (int)(i / row_bytes), b = (int)(i - (int64_t)r * row_bytes);
  dst[i] = src[(int64_t)ids[r] * stride + b];
}
__global__ void scatter_result_kernel(const float* __restrict__ s, const int64_t* __restrict__ r, const int32_t* __restrict__ ids, int n, int k,
                                      float* __restrict__ os, int64_t* __restrict__ orow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * k) return;
  const int f = (int)(i / k), j = (int)(i - (int64_t)f * k);
  os[(int64_t)ids[f] * k + j] = s[i];
  orow[(int64_t)ids[f] * k + j] = r[i];
}

struct Arena {                    // bump allocator over a grow-only device buffer (one per shard context)
  void** base; size_t* cap; size_t used = 0; int device; bool persist = true;
  std::vector<void*> spill;       // allocations beyond the arena's current size (freed at the end of the call; the arena grows for the next)
  size_t want = 0;
  void* get(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    want += bytes;
    if (used + bytes <= *cap) { void* p = (char*)*base + used; used += bytes; return p; }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    spill.push_back(p);
    return p;
  }
  void finish() {
    for (void* p : spill) (void)hipFree(p);
    spill.clear();
    if (persist && want > *cap) { (void)hipFree(*base); *base = nullptr; *cap = 0; if (hipMalloc(base, want) == hipSuccess) *cap = want; }
  }
};

struct ShardCtx {
  dhr_index* ix;
  int device;
  hipStream_t stream;
  Arena* arena;
};

struct HipBackend : Backend {
  std::vector<ShardCtx> sh;
  dhr_comm* comm = nullptr;       // SPMD (n_local == 1, world > 1): RCCL or the caller's host transport; null: one process, gathers are device copies
  std::vector<std::vector<char>> host_v, host_i;      // host sub-batch of the repair step (shared by the local shards)
  dhr_query_batch host_sub;

  // makes shard i's device current: what every method that enqueues on the shard's stream opens with
  int use(int i) { SH_HIP(hipSetDevice(sh[i].device)); return DHR_OK; }
  void* alloc(int i, size_t bytes) override { (void)hipSetDevice(sh[i].device); return sh[i].arena->get(bytes); }
  int zero(int i, void* p, size_t bytes) override {
    SH_TRY(use(i));
    SH_HIP(hipMemsetAsync(p, 0, bytes, sh[i].stream));
    return DHR_OK;
  }
  int put_status(int i, void* block, const Block& b, int status) override {
    SH_TRY(use(i));
    SH_HIP(hipMemsetD32Async((hipDeviceptr_t)((char*)block + b.payload), status, 4, sh[i].stream));
    return DHR_OK;
  }
  int fold_status(int i, const void* gathered, const Block& b, int32_t* rec) override {
    if (comm && comm->cb) return DHR_OK;             // the host transport read the records behind the gather already
    SH_TRY(use(i));
    hipLaunchKernelGGL(fold_status_kernel, dim3(1), dim3(64), 0, sh[i].stream, (const char*)gathered, world, b.stride, b.payload, rec);
    return DHR_OK;
  }
  int set_share(int i, int share) override { return dhr_index_set_param(sh[i].ix, DHR_PARAM_SAMPLE_SHARE, share); }
  void abort(int i) override { dhr_internal_search_abort(sh[i].ix); }
  int sample_rank(int i, int k) override { return dhr_search_sample_rank(sh[i].ix, k); }
  int union_rank(int i, int k) override { return dhr_search_union_rank(sh[i].ix, k); }
  int begin(int i, const dhr_query_batch* qb, int k, float* sample) override { SH_TRY(use(i)); return dhr_internal_search_begin_async(sh[i].ix, qb, k, sample, sh[i].stream); }
  int finish(int i, const float* tau, float* ls, int64_t* lr, int32_t* cnt) override { SH_TRY(use(i)); return dhr_internal_search_finish_async(sh[i].ix, tau, ls, lr, cnt, DHR_MEM_DEVICE, sh[i].stream); }
  int stage_ranks(int i, Stage stage, int k, int* r_local, int* r_union) override {
    int32_t a = 0, b = 0;
    (void)(stage == MID ? dhr_search_mid_ranks : dhr_search_pre_ranks)(sh[i].ix, k, &a, &b);
    *r_local = a; *r_union = b;
    return DHR_OK;
  }
  int mid(int i, const float* tau, int r_local, float* scores) override { SH_TRY(use(i)); return dhr_internal_search_mid_async(sh[i].ix, tau, r_local, scores, sh[i].stream); }
  int pre(int i, const dhr_query_batch* qb, int k, int r_local, float* scores) override { SH_TRY(use(i)); return dhr_internal_search_pre_async(sh[i].ix, qb, k, r_local, scores, sh[i].stream); }
  int begin_rest(int i, const float* tau, float* sample) override { SH_TRY(use(i)); return dhr_internal_search_begin_rest_async(sh[i].ix, tau, sample, sh[i].stream); }
  int search(int i, const dhr_query_batch* qb, int k, float* s, int64_t* r) override { SH_TRY(use(i)); return dhr_search(sh[i].ix, qb, k, s, r, DHR_MEM_DEVICE, sh[i].stream); }
  int gather(const std::vector<const void*>& send, const std::vector<void*>& recv, const Block& b) override {
    const size_t bytes = b.stride;
    if (comm && comm->dead) return dhr_set_error_message(DHR_ERR_INVALID, "the communicator was aborted (dhr_comm_abort)");
    if (comm && comm->comm) {
      SH_NCCL(ncclAllGather(send[0], recv[0], bytes, ncclInt8, comm->comm, sh[0].stream));
      return DHR_OK;
    }
    if (comm && comm->cb) {       // the caller's transport moves HOST buffers: stage through pinned memory on this stream
      const size_t need = bytes * (size_t)(world + 1);
      if (comm->h_stage_bytes < need) {
        if (comm->h_stage) (void)hipHostFree(comm->h_stage);
        comm->h_stage = nullptr; comm->h_stage_bytes = 0;
        SH_HIP(hipHostMalloc(&comm->h_stage, need, hipHostMallocDefault));
        comm->h_stage_bytes = need;
      }
      char* hs = (char*)comm->h_stage;
      char* hr = hs + bytes;
      SH_HIP(hipMemcpyAsync(hs, send[0], bytes, hipMemcpyDeviceToHost, sh[0].stream));
      SH_HIP(hipStreamSynchronize(sh[0].stream));
      if (comm->cb(comm->cb_user, hs, hr, (int64_t)bytes) != 0) return dhr_set_error_message(DHR_ERR_INTERNAL, "the caller's all-gather callback failed");
      int who = 0;
      if (const int st = host_block_status(hr, world, b, &who)) return peer_error(who, st);      // the blocks are in host memory: every rank leaves HERE
      SH_HIP(hipMemcpyAsync(recv[0], hr, bytes * (size_t)world, hipMemcpyHostToDevice, sh[0].stream));
      return DHR_OK;
    }
    // one process: make every block visible to every local shard (plain device copies; peer copies across devices).  Shards that share ONE
    // stream (the single-GPU emulation: every shard on the caller's stream) need no host synchronisation: the copies are ordered by the stream
    bool one_stream = true;
    for (int i = 1; i < n_local; ++i) one_stream = one_stream && sh[i].stream == sh[0].stream && sh[i].device == sh[0].device;
    if (!one_stream) for (int i = 0; i < n_local; ++i) SH_HIP(hipStreamSynchronize(sh[i].stream));
    for (int d = 0; d < n_local; ++d) {
      SH_TRY(use(d));
      for (int s = 0; s < n_local; ++s)
        SH_HIP(hipMemcpyAsync((char*)recv[d] + (size_t)s * bytes, send[s], bytes, hipMemcpyDefault, sh[d].stream));
    }
    if (!one_stream) for (int i = 0; i < n_local; ++i) SH_HIP(hipStreamSynchronize(sh[i].stream));
    return DHR_OK;
  }
  int exchange_vote(const RankVote& mine, int32_t* all) override {
    if (comm->dead) return dhr_set_error_message(DHR_ERR_INVALID, "the communicator was aborted (dhr_comm_abort)");
    if (comm->cb) {                                  // host transport: the values are host memory already
      if (comm->cb(comm->cb_user, mine.v, all, 48) != 0) return dhr_set_error_message(DHR_ERR_INTERNAL, "the caller's all-gather callback failed");
      return DHR_OK;
    }
    SH_TRY(use(0));                                  // (no status record on this exchange: the vote carries the status)
    int32_t* d = (int32_t*)sh[0].arena->get(64 + (size_t)world * 48);
    if (!d) return dhr_set_error_message(DHR_ERR_HIP, "out of device memory");
    SH_HIP(hipMemcpyAsync(d, mine.v, 48, hipMemcpyHostToDevice, sh[0].stream));
    SH_NCCL(ncclAllGather(d, d + 16, 48, ncclInt8, comm->comm, sh[0].stream));
    SH_HIP(hipMemcpyAsync(all, d + 16, (size_t)world * 48, hipMemcpyDeviceToHost, sh[0].stream));
    SH_HIP(hipStreamSynchronize(sh[0].stream));
    return DHR_OK;
  }
  // the ru-th best of [world] sorted score lists per query, lists b.stride bytes apart
  int union_threshold(int i, const float* gathered, const Block& b, int Q, int r, int ru, float* tau, bool raise) override {
    SH_TRY(use(i));
    float* merged = (float*)sh[i].arena->get((size_t)Q * ru * 4);
    if (!merged) return dhr_set_error_message(DHR_ERR_HIP, "out of device memory in the sharded search");
    if (((int64_t)world * r + ru) * 4 > 160 * 1024 || world > 64)
      return dhr_set_error_message(DHR_ERR_UNSUPPORTED, "the sample lists of one query do not fit the LDS");
    SH_HIP(launch_merge_lists(Q, world, r, gathered, nullptr, ru, merged, nullptr, sh[i].stream, (int64_t)(b.stride / 4), 0));
    hipLaunchKernelGGL(column_kernel, dim3((Q + 255) / 256), dim3(256), 0, sh[i].stream, merged, ru, ru - 1, Q, tau, raise);
    return DHR_OK;
  }
  int flag_failures(int i, const int32_t* counts, const Block& b, int Q, int k, int kk, int32_t* fail_ids, int32_t* rec) override {
    SH_TRY(use(i));
    hipLaunchKernelGGL(fail_kernel, dim3((Q + 255) / 256), dim3(256), 0, sh[i].stream, counts, b.stride, world, Q, k, kk, fail_ids, rec);
    return DHR_OK;
  }
  int prefix(int i, const float* s, const int64_t* r, int k, int kk, int Q, float* os, int64_t* orow) override {
    SH_TRY(use(i));
    const int64_t n = (int64_t)Q * kk;
    hipLaunchKernelGGL(prefix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sh[i].stream, s, r, k, kk, Q, os, orow);
    return DHR_OK;
  }
  int merge(int i, int Q, int L, const float* gs, const int64_t* gr, const Block& b, int k, float* os, int64_t* orow) override {
    const ShardCtx& c = sh[i];
    SH_TRY(use(i));
    // sorted per-shard lists, one [Q, L] section per rank: rank merge in the LDS when the lists of a query fit, else the general reduce
    if (world <= 64 && ((int64_t)world * L + k) * 12 <= 160 * 1024) {
      SH_HIP(launch_merge_lists(Q, world, L, gs, gr, k, os, orow, c.stream, (int64_t)(b.stride / 4), (int64_t)(b.stride / 8)));
      return DHR_OK;
    }
    // [world, Q, L] -> [Q, world * L]
    float* ts = (float*)c.arena->get((size_t)Q * world * L * 4);
    int64_t* tr = (int64_t*)c.arena->get((size_t)Q * world * L * 8);
    if (!ts || !tr) return dhr_set_error_message(DHR_ERR_HIP, "out of device memory in the shard reduce");
    for (int w = 0; w < world; ++w) {
      SH_HIP(hipMemcpy2DAsync(ts + (size_t)w * L, (size_t)world * L * 4, (const char*)gs + (size_t)w * b.stride, (size_t)L * 4, (size_t)L * 4, Q, hipMemcpyDeviceToDevice, c.stream));
      SH_HIP(hipMemcpy2DAsync(tr + (size_t)w * L, (size_t)world * L * 8, (const char*)gr + (size_t)w * b.stride, (size_t)L * 8, (size_t)L * 8, Q, hipMemcpyDeviceToDevice, c.stream));
    }
    return dhr_merge_topk(c.device, Q, world * L, ts, tr, k, os, orow, c.stream);
  }
  int read_failed(const std::vector<int32_t*>& rec, const std::vector<int32_t*>& fail_ids, std::vector<int32_t>& ids, int* peer_status, int* peer_rank) override {
    int32_t h[4] = {0, 0, 0, 0};
    SH_TRY(use(0));
    SH_HIP(hipMemcpyAsync(h, rec[0], 16, hipMemcpyDeviceToHost, sh[0].stream));
    for (int i = 0; i < n_local; ++i) SH_HIP(hipStreamSynchronize(sh[i].stream));
    *peer_status = h[1]; *peer_rank = h[2];
    const int32_t nf = !fail_ids.empty() && fail_ids[0] ? h[0] : 0;
    ids.resize((size_t)nf);
    if (nf > 0) SH_HIP(hipMemcpy(ids.data(), fail_ids[0], (size_t)nf * 4, hipMemcpyDeviceToHost));
    return DHR_OK;
  }
  int sub_batch(int i, const dhr_query_batch* in, const std::vector<int32_t>& ids, dhr_query_batch* out, int32_t** ids_mem) override {
    const int F = (int)ids.size();
    SH_TRY(use(i));
    int32_t* d_ids = (int32_t*)sh[i].arena->get((size_t)F * 4);
    if (!d_ids) return dhr_set_error_message(DHR_ERR_HIP, "out of device memory in the sharded search");
    SH_HIP(hipMemcpyAsync(d_ids, ids.data(), (size_t)F * 4, hipMemcpyHostToDevice, sh[i].stream));
    *ids_mem = d_ids;
    if (in->mem_kind == DHR_MEM_HOST) {          // host batch: gathered on the host once, shared by the local shards
      if (host_v.empty()) { host_v.resize(1); host_i.resize(1); host_sub_batch(in, ids, host_v[0], host_i[0], &host_sub); }
      *out = host_sub;
      return DHR_OK;
    }
    // device batch: the caller's arrays live on ONE device; gather there (shard 0's context must be that device for SPMD, and in the
    // one-process form every shard on another device reads through peer access / managed mapping)
    const int vsz = in->value_dtype == DHR_VAL_F32 ? 4 : 2, isz = in->index_dtype == DHR_IDX_I16 ? 2 : 1;
    const int64_t vrow = in->ld_value * vsz, irow = in->index ? in->ld_index * isz : 0;
    char* gv = (char*)sh[i].arena->get((size_t)F * vrow);
    char* gi = in->index ? (char*)sh[i].arena->get((size_t)F * irow) : nullptr;
    if (!gv || (in->index && !gi)) return dhr_set_error_message(DHR_ERR_HIP, "out of device memory in the sharded search");
    int64_t n = (int64_t)F * vrow;
    hipLaunchKernelGGL(gather_rows_bytes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sh[i].stream, (const char*)in->value, vrow, (int)vrow, d_ids, F, gv);
    if (gi) {
      n = (int64_t)F * irow;
      hipLaunchKernelGGL(gather_rows_bytes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sh[i].stream, (const char*)in->index, irow, (int)irow, d_ids, F, gi);
    }
    *out = *in;
    out->n_queries = F;
    out->value = gv;
    out->index = gi;
    return DHR_OK;
  }
  int scatter(int i, const float* s, const int64_t* r, const int32_t* ids_mem, int F, int k, float* os, int64_t* orow) override {
    SH_TRY(use(i));
    const int64_t n = (int64_t)F * k;
    hipLaunchKernelGGL(scatter_result_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sh[i].stream, s, r, ids_mem, F, k, os, orow);
    return DHR_OK;
  }
};

// ------------------------------------------------------------------------------------------------------------------------------------
// HostBackend: one caller-supplied shard in host memory, caller-supplied all-gather.  Test / bring-up hook (dhr_search_sharded_host).
struct HostBackend : Backend {
  const dhr_host_shard* shard = nullptr;
  dhr_allgather_fn cb = nullptr;
  void* cb_user = nullptr;
  int share = 1;
  std::vector<std::vector<char>> mem;
  std::vector<char> sub_v, sub_i;
  std::vector<int32_t> sub_ids;

  void* alloc(int, size_t bytes) override { mem.emplace_back(bytes ? bytes : 16); return mem.back().data(); }
  int zero(int, void* p, size_t bytes) override { memset(p, 0, bytes); return DHR_OK; }
  int put_status(int, void* block, const Block& b, int status) override { const int32_t st = status; memcpy((char*)block + b.payload, &st, 4); return DHR_OK; }
  int fold_status(int, const void*, const Block&, int32_t*) override { return DHR_OK; }      // (gather read the records)
  int set_share(int, int s) override { share = s; return DHR_OK; }
  int sample_rank(int, int k) override { return shard->sample_rank(shard->user, k, share); }
  int union_rank(int, int k) override { return shard->union_rank(shard->user, k); }
  // the status of a shard callback (0: fine)
  static int cb_status(int rc, const char* what) {
    if (rc == 0) return DHR_OK;
    char buf[64];
    snprintf(buf, sizeof(buf), "host shard: %s failed", what);
    return dhr_set_error_message(DHR_ERR_INTERNAL, buf);
  }
  int begin(int, const dhr_query_batch* qb, int k, float* sample) override { return cb_status(shard->begin(shard->user, qb, k, share, sample), "begin"); }
  int finish(int, const float* tau, float* ls, int64_t* lr, int32_t* cnt) override { return cb_status(shard->finish(shard->user, tau, ls, lr, cnt), "finish"); }
  int stage_ranks(int, Stage stage, int k, int* r_local, int* r_union) override {
    int32_t a = 0, b = 0;
    if (stage == MID) { if (shard->mid_ranks && shard->mid) (void)shard->mid_ranks(shard->user, k, share, &a, &b); }
    else if (shard->pre_ranks && shard->pre && shard->begin_rest) (void)shard->pre_ranks(shard->user, k, share, &a, &b);
    *r_local = a; *r_union = b;
    return DHR_OK;
  }
  int mid(int, const float* tau, int r_local, float* scores) override { return cb_status(shard->mid(shard->user, tau, r_local, scores), "mid"); }
  int pre(int, const dhr_query_batch* qb, int k, int r_local, float* scores) override { return cb_status(shard->pre(shard->user, qb, k, share, r_local, scores), "pre"); }
  int begin_rest(int, const float* tau, float* sample) override { return cb_status(shard->begin_rest(shard->user, tau, sample), "begin_rest"); }
  int search(int, const dhr_query_batch* qb, int k, float* s, int64_t* r) override { return cb_status(shard->search(shard->user, qb, k, s, r), "search"); }
  int gather(const std::vector<const void*>& send, const std::vector<void*>& recv, const Block& b) override {
    if (world == 1) memcpy(recv[0], send[0], b.stride);
    else if (cb(cb_user, send[0], recv[0], (int64_t)b.stride) != 0) return dhr_set_error_message(DHR_ERR_INTERNAL, "the caller's all-gather callback failed");
    int who = 0;
    if (const int st = host_block_status(recv[0], world, b, &who)) return peer_error(who, st);
    return DHR_OK;
  }
  int exchange_vote(const RankVote& mine, int32_t* all) override {
    return cb(cb_user, mine.v, all, 48) == 0 ? DHR_OK : dhr_set_error_message(DHR_ERR_INTERNAL, "the caller's all-gather callback failed");
  }
  // [world] sections of [Q, L] floats / int64, b.stride bytes apart -> the dense [world, Q, L] arrays dhr_merge_topk_lists_host takes
  void densify(const void* g, const Block& b, size_t section_bytes, std::vector<char>& out) const {
    out.resize((size_t)world * section_bytes);
    for (int w = 0; w < world; ++w) memcpy(out.data() + (size_t)w * section_bytes, (const char*)g + (size_t)w * b.stride, section_bytes);
  }
  int union_threshold(int, const float* gathered, const Block& b, int Q, int r, int ru, float* tau, bool raise) override {
    std::vector<float> merged((size_t)Q * ru);
    std::vector<char> dense;
    densify(gathered, b, (size_t)Q * r * 4, dense);
    SH_TRY(dhr_merge_topk_lists_host(Q, world, r, (const float*)dense.data(), nullptr, ru, merged.data(), nullptr));
    for (int q = 0; q < Q; ++q) {
      const float v = merged[(size_t)q * ru + (ru - 1)];
      tau[q] = raise ? std::max(tau[q], v) : v;
    }
    return DHR_OK;
  }
  int flag_failures(int, const int32_t* counts, const Block& b, int Q, int k, int kk, int32_t* fail_ids, int32_t* rec) override {
    host_flag_failures(counts, b, world, Q, k, kk, fail_ids, rec);
    return DHR_OK;
  }
  int prefix(int, const float* s, const int64_t* r, int k, int kk, int Q, float* os, int64_t* orow) override {
    for (int q = 0; q < Q; ++q) {
      memcpy(os + (size_t)q * kk, s + (size_t)q * k, (size_t)kk * 4);
      memcpy(orow + (size_t)q * kk, r + (size_t)q * k, (size_t)kk * 8);
    }
    return DHR_OK;
  }
  int merge(int, int Q, int L, const float* gs, const int64_t* gr, const Block& b, int k, float* os, int64_t* orow) override {
    std::vector<char> ds, dr;
    densify(gs, b, (size_t)Q * L * 4, ds);
    densify(gr, b, (size_t)Q * L * 8, dr);
    return dhr_merge_topk_lists_host(Q, world, L, (const float*)ds.data(), (const int64_t*)dr.data(), k, os, orow);
  }
  int read_failed(const std::vector<int32_t*>& rec, const std::vector<int32_t*>& fail_ids, std::vector<int32_t>& ids, int* peer_status, int* peer_rank) override {
    *peer_status = 0; *peer_rank = 0;                 // (host-visible blocks: a failure ended the step at its gather)
    if (!fail_ids.empty() && fail_ids[0]) ids.assign(fail_ids[0], fail_ids[0] + rec[0][0]); else ids.clear();
    return DHR_OK;
  }
  int sub_batch(int, const dhr_query_batch* in, const std::vector<int32_t>& ids, dhr_query_batch* out, int32_t** ids_mem) override {
    if (in->mem_kind != DHR_MEM_HOST) return dhr_set_error_message(DHR_ERR_INVALID, "host shards take host query batches");
    host_sub_batch(in, ids, sub_v, sub_i, out);
    sub_ids = ids;
    *ids_mem = sub_ids.data();
    return DHR_OK;
  }
  int scatter(int, const float* s, const int64_t* r, const int32_t* ids_mem, int F, int k, float* os, int64_t* orow) override {
    for (int f = 0; f < F; ++f) {
      memcpy(os + (size_t)ids_mem[f] * k, s + (size_t)f * k, (size_t)k * 4);
      memcpy(orow + (size_t)ids_mem[f] * k, r + (size_t)f * k, (size_t)k * 8);
    }
    return DHR_OK;
  }
};

// ---- what the two device entry points share ---------------------------------------------------------------------------------------------------------
// Where a local shard builds its [Q, k] result: shard 0 straight in the caller's arrays when those are device memory (direct), else in the shard's arena
int stage_result(const ShardCtx& c, bool direct, int Q, int k, float* out_scores, int64_t* out_rows, float** ds, int64_t** dr) {
  if (direct) { *ds = out_scores; *dr = out_rows; return DHR_OK; }
  *ds = (float*)c.arena->get((size_t)Q * k * 4);
  *dr = (int64_t*)c.arena->get((size_t)Q * k * 8);
  return *ds && *dr ? DHR_OK : dhr_set_error_message(DHR_ERR_HIP, "out of device memory");
}
int deliver(const ShardCtx& c, int Q, int k, const float* ds, const int64_t* dr, float* out_scores, int64_t* out_rows, int mem_kind) {
  if (mem_kind == DHR_MEM_HOST) {
    SH_HIP(hipMemcpyAsync(out_scores, ds, (size_t)Q * k * 4, hipMemcpyDeviceToHost, c.stream));
    SH_HIP(hipMemcpyAsync(out_rows, dr, (size_t)Q * k * 8, hipMemcpyDeviceToHost, c.stream));
  }
  SH_HIP(hipStreamSynchronize(c.stream));
  return DHR_OK;
}
// The way out of both, whatever `rc` the call has come to: shard 0's result to its destination, then every shard's stream drained and what its arena
// spilled released (the arena grows for the next call).
int finish_call(HipBackend& B, int rc, int Q, int k, const float* ds, const int64_t* dr, float* out_scores, int64_t* out_rows, int mem_kind) {
  if (rc == DHR_OK) { (void)hipSetDevice(B.sh[0].device); rc = deliver(B.sh[0], Q, k, ds, dr, out_scores, out_rows, mem_kind); }
  for (const ShardCtx& c : B.sh) {
    (void)hipSetDevice(c.device);
    (void)hipStreamSynchronize(c.stream);
    c.arena->finish();
  }
  return rc;
}

}  // namespace


extern "C" int dhr_comm_unique_id(void* out, int32_t out_bytes) try {
  if (!out || out_bytes < (int32_t)NCCL_UNIQUE_ID_BYTES) return dhr_set_error_message(DHR_ERR_INVALID, "the unique id needs a 128-byte buffer");
  ncclUniqueId id;
  SH_NCCL(ncclGetUniqueId(&id));
  memcpy(out, id.internal, NCCL_UNIQUE_ID_BYTES);
  return DHR_OK;
} DHR_CATCH_STATUS
extern "C" int dhr_comm_create(const void* unique_id, int32_t world, int32_t rank, int32_t device, dhr_comm** out) try {
  if (!unique_id || !out || world < 1 || rank < 0 || rank >= world) return dhr_set_error_message(DHR_ERR_INVALID, "bad argument");
  SH_HIP(hipSetDevice(device));
  ncclUniqueId id;
  memcpy(id.internal, unique_id, NCCL_UNIQUE_ID_BYTES);
  dhr_comm* c = new dhr_comm();
  c->world = world; c->rank = rank; c->device = device; c->owned = true;
  ncclResult_t r = ncclCommInitRank(&c->comm, world, id, rank);
  if (r != ncclSuccess) { delete c; return dhr_set_error_message(DHR_ERR_HIP, (std::string("ncclCommInitRank: ") + ncclGetErrorString(r)).c_str()); }
  *out = c;
  return DHR_OK;
} DHR_CATCH_STATUS
extern "C" int dhr_comm_wrap(void* nccl_comm, int32_t world, int32_t rank, int32_t device, dhr_comm** out) try {
  if (!nccl_comm || !out || world < 1 || rank < 0 || rank >= world) return dhr_set_error_message(DHR_ERR_INVALID, "bad argument");
  dhr_comm* c = new dhr_comm();
  c->comm = (ncclComm_t)nccl_comm; c->world = world; c->rank = rank; c->device = device; c->owned = false;
  *out = c;
  return DHR_OK;
} DHR_CATCH_STATUS
extern "C" int dhr_comm_create_callback(int32_t world, int32_t rank, int32_t device, dhr_allgather_fn allgather, void* user, dhr_comm** out) try {
  if (!allgather || !out || world < 1 || rank < 0 || rank >= world) return dhr_set_error_message(DHR_ERR_INVALID, "bad argument");
  dhr_comm* c = new dhr_comm();
  c->cb = allgather; c->cb_user = user; c->world = world; c->rank = rank; c->device = device; c->owned = false;
  *out = c;
  return DHR_OK;
} DHR_CATCH_STATUS
extern "C" void dhr_comm_destroy(dhr_comm* c) try {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->owned && c->comm && !c->dead) (void)ncclCommDestroy(c->comm);      // (an aborted communicator is gone already)
  (void)hipFree(c->arena);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  delete c;
} DHR_CATCH_VOID

extern "C" int32_t dhr_debug_sharded_repairs(void) try { return g_last_repairs; } DHR_CATCH_VALUE(0)
extern "C" int dhr_comm_info(const dhr_comm* c, int32_t what) try {
  if (!c) return dhr_set_error_message(DHR_ERR_INVALID, "null communicator");
  if (c->dead) return dhr_set_error_message(DHR_ERR_INVALID, "the communicator was aborted (dhr_comm_abort)");
  int v = 0;
  switch (what) {
    case DHR_COMM_TRANSPORT: return c->comm ? 0 : 1;
    case DHR_COMM_WORLD: if (!c->comm) return c->world; SH_NCCL(ncclCommCount(c->comm, &v)); return v;
    case DHR_COMM_RANK: if (!c->comm) return c->rank; SH_NCCL(ncclCommUserRank(c->comm, &v)); return v;
    case DHR_COMM_DEVICE: if (!c->comm) return c->device; SH_NCCL(ncclCommCuDevice(c->comm, &v)); return v;
    default: return dhr_set_error_message(DHR_ERR_INVALID, "unknown dhr_comm_info field");
  }
} DHR_CATCH_STATUS
// Only aborts and marks the handle: the thread that was blocked in one of the communicator's collectives returns through sharded_core /
// HipBackend, which still use the struct and its arena (until round 5 this freed both under that thread: use after free).  The caller
// frees the handle with dhr_comm_destroy once that thread is back.
extern "C" void dhr_comm_abort(dhr_comm* c) try {
  if (!c || c->dead) return;
  c->dead = true;
  if (c->owned && c->comm) (void)ncclCommAbort(c->comm);
} DHR_CATCH_VOID

extern "C" int dhr_search_sharded_host(const dhr_host_shard* shard, int32_t world, int32_t rank, dhr_allgather_fn allgather, void* user,
                                       const dhr_query_batch* qb, int32_t k, float* out_scores, int64_t* out_rows) try {
  if (!shard) return dhr_set_error_message(DHR_ERR_INVALID, "bad argument");
  if (shard->struct_size != (uint32_t)sizeof(dhr_host_shard))
    return dhr_set_error_message(DHR_ERR_INVALID, "dhr_host_shard::struct_size does not match this library (the caller was built against another version of dhr_hip.h)");
  if (!shard->sample_rank || !shard->union_rank || !shard->begin || !shard->finish || !shard->search || !qb || !out_scores || !out_rows ||
      k <= 0 || world < 1 || rank < 0 || rank >= world || (world > 1 && !allgather))
    return dhr_set_error_message(DHR_ERR_INVALID, "bad argument");
  if (qb->mem_kind != DHR_MEM_HOST) return dhr_set_error_message(DHR_ERR_INVALID, "host shards take host query batches");
  HostBackend B;
  B.world = world; B.n_local = 1;
  B.shard = shard; B.cb = allgather; B.cb_user = user;
  return sharded_core(B, qb, k, &out_scores, &out_rows);
} DHR_CATCH_STATUS

extern "C" int dhr_search_sharded(dhr_index* shard, dhr_comm* comm, const dhr_query_batch* qb, int32_t k, float* out_scores, int64_t* out_rows,
                                  int32_t out_mem_kind, void* stream) try {
  // TODO(ADVICE 2): these per-rank checks return BEFORE the rank agreement, so the other ranks wait in it; they should answer it (vote_status_only)
  if (!shard || !comm || !qb || !out_scores || !out_rows || k <= 0 || !DHR_MEM_KIND_OK(out_mem_kind)) return dhr_set_error_message(DHR_ERR_INVALID, "bad argument");
  if (comm->dead) return dhr_set_error_message(DHR_ERR_INVALID, "the communicator was aborted (dhr_comm_abort)");
  const int device = dhr_index_device(shard);
  if (device != comm->device) return dhr_set_error_message(DHR_ERR_INVALID, "the shard and the communicator live on different devices");
  SH_HIP(hipSetDevice(device));
  Arena arena{&comm->arena, &comm->arena_bytes, 0, device};
  HipBackend B;
  B.world = comm->world; B.n_local = 1;
  B.comm = comm->world > 1 ? comm : nullptr;       // a single rank gathers by copy (n_local == world == 1)
  std::vector<ShardCtx>& sh = B.sh;
  const int Q = qb->n_queries;
  float* ds = out_scores;
  int64_t* dr = out_rows;
  // this rank's set-up: a failure here is answered in the rank agreement the others are about to enter (the step's own failures: Step::leave)
  int rc = DHR_OK;
  try {
    sh.push_back({shard, device, (hipStream_t)stream, &arena});
    rc = stage_result(sh[0], out_mem_kind == DHR_MEM_DEVICE, Q, k, out_scores, out_rows, &ds, &dr);
  } catch (...) {
    rc = dhr::on_exception();
  }
  if (rc != DHR_OK && sh.size() == 1 && B.comm) vote_status_only(B, rc);
  if (rc == DHR_OK) rc = sharded_core(B, qb, k, &ds, &dr);
  return finish_call(B, rc, Q, k, ds, dr, out_scores, out_rows, out_mem_kind);
} DHR_CATCH_STATUS

extern "C" int dhr_search_sharded_local(dhr_index** shards, int32_t n_shards, const dhr_query_batch* qb, int32_t k, float* out_scores,
                                        int64_t* out_rows, int32_t out_mem_kind, void* stream) try {
  if (!shards || n_shards < 1 || n_shards > 64 || !qb || !out_scores || !out_rows || k <= 0 || !DHR_MEM_KIND_OK(out_mem_kind))
    return dhr_set_error_message(DHR_ERR_INVALID, "bad argument (1 <= n_shards <= 64)");
  std::vector<Arena> arenas;
  arenas.reserve(n_shards);
  HipBackend B;
  B.world = n_shards; B.n_local = n_shards;
  std::vector<ShardCtx>& sh = B.sh;
  std::vector<hipStream_t> own(n_shards, nullptr);
  const int dev0 = dhr_index_device(shards[0]);
  for (int i = 0; i < n_shards; ++i) {
    if (!shards[i]) return dhr_set_error_message(DHR_ERR_INVALID, "null shard handle");
    const int dev = dhr_index_device(shards[i]);
    // (the scratch of a step lives in the shard's handle and is kept between steps: until round 6 every block of every step was a hipMalloc /
    // hipFree pair -- 24 instead of 18 ms per shard of the 8-shard benchmark step)
    void** a_base = nullptr; size_t* a_cap = nullptr;
    dhr_internal_index_arena(shards[i], &a_base, &a_cap);
    arenas.push_back(Arena{a_base, a_cap, 0, dev});
    hipStream_t s = (hipStream_t)stream;
    if (dev != dev0) { SH_HIP(hipSetDevice(dev)); SH_HIP(hipStreamCreateWithFlags(&own[i], hipStreamNonBlocking)); s = own[i]; }
    sh.push_back({shards[i], dev, s, &arenas[i]});
  }
  const int Q = qb->n_queries;
  std::vector<float*> os(n_shards);
  std::vector<int64_t*> orow(n_shards);
  int rc = DHR_OK;
  for (int i = 0; i < n_shards && rc == DHR_OK; ++i) {
    if (hipSetDevice(sh[i].device) != hipSuccess) rc = dhr_set_error_message(DHR_ERR_HIP, "hipSetDevice failed");
    else rc = stage_result(sh[i], i == 0 && out_mem_kind == DHR_MEM_DEVICE, Q, k, out_scores, out_rows, &os[i], &orow[i]);
  }
  if (rc == DHR_OK) rc = sharded_core(B, qb, k, os.data(), orow.data());
  rc = finish_call(B, rc, Q, k, os[0], orow[0], out_scores, out_rows, out_mem_kind);
  for (int i = 0; i < n_shards; ++i)
    if (own[i]) { (void)hipSetDevice(sh[i].device); (void)hipStreamDestroy(own[i]); }
  return rc;
} DHR_CATCH_STATUS

// The pure parts of the sharded search (sharded.hip): the layout of the blocks a step all-gathers, the ranks' vote before the step,
// and the ordered all-gathers a step owes once the vote is in.  Every block is laid out HERE and nowhere else: a rank that sized one gather differently
// from the others would hang them.  Plain C++17, no HIP, no RCCL: tests/sharded_plan_check.cpp checks the invariants over a grid on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
namespace dhr {
namespace sharded {

// ---- blocks ----------------------------------------------------------------------------------------------------------------------------------------
// One rank's share of an all-gather: [payload | status record (16 B)], `stride` bytes apart in the receive buffer.
struct Block { size_t payload = 0, stride = 0; };
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline Block block_of(size_t payload) {
  payload = align16(payload);
  return {payload, (payload + 16 + 255) & ~(size_t)255};
}
// [Q, r] fp32: the scores of one threshold agreement
inline Block score_block(int Q, int r) { return block_of((size_t)Q * r * 4); }
// Sorted lists of L entries per query.  The step's last all-gather: [Q] counts | [Q, L] scores | [Q, L] rows; the local / repair path: [Q, L] scores |
// [Q, L] rows (no counts: off_scores == 0).
struct ListBlock {
  Block b;
  size_t off_scores = 0, off_rows = 0;      // (the counts, where present, sit at offset 0)
  int Q = 0, L = 0;
  template <class T> int32_t* counts(T* blk) const { return (int32_t*)blk; }
  template <class T> float* scores(T* blk) const { return (float*)((char*)blk + off_scores); }
  template <class T> int64_t* rows(T* blk) const { return (int64_t*)((char*)blk + off_rows); }
};
inline ListBlock list_block(int Q, int L, bool with_counts) {
  ListBlock l;
  l.off_scores = with_counts ? align16((size_t)Q * 4) : 0;
  l.off_rows = align16(l.off_scores + (size_t)Q * L * 4);
  l.b = block_of(l.off_rows + (size_t)Q * L * 8);
  l.Q = Q; l.L = L;
  return l;
}
// length of the list prefixes of the last all-gather: a fixed fraction of k by world size (no host read decides it)
inline int prefix_len(int k, int world) {
  if (world <= 2) return k;
  const int kk = ((3 * k + world - 1) / world + 64 + 63) / 64 * 64;
  return std::min(k, kk);
}

// ---- the rank vote -----------------------------------------------------------------------------------------------------------------------------------
// What a shard's controller reports before a step: its share r of the union's rank ru, and the (local, union) ranks of the optional second agreement
// (mid) and of the first agreement in two rounds (pre); (0, 0): the shard has no such step.
struct ShardRanks { int r = 0, ru = 0, rl_mid = 0, ru_mid = 0, rl_pre = 0, ru_pre = 0; };
struct Ranks { int r = 0, ru = 0, rl_mid = 0, ru_mid = 0, rl_pre = 0, ru_pre = 0, status = 0; };
// The agreement is ONE exchange of 48 bytes per rank and an element-wise MINIMUM: maxima travel negated.  All shards must report the same r > 0 AND the
// same ru (the share is many-to-one: unequal shard sizes or sample periods can give equal shares of different union ranks, and the count check of the
// step assumes ONE common threshold column), else r = 0 and the step takes the local path.  Mid and pre ranks of shards whose sizes differ by a tile may
// differ by one: every shard uses the LARGEST (a lower threshold: still valid), none if some shard has none.  STATUS carries the ranks' status so far (a
// rank whose set-up failed says so here instead of staying away from the exchange); statuses are <= 0, so the minimum is a failure if there is one.
struct RankVote {
  enum Slot { R_MIN, R_NEG_MAX, RU_MIN, RU_NEG_MAX, MID_L_MIN, MID_L_NEG_MAX, MID_U_NEG_MAX, PRE_L_MIN, PRE_L_NEG_MAX, PRE_U_NEG_MAX, STATUS, ZERO, SLOTS };
  int32_t v[SLOTS] = {};
  static RankVote status_only(int status) { RankVote x; x.v[STATUS] = status; return x; }
  // from the n local shards' ranks and this process's status so far
  static RankVote pack(const ShardRanks* s, int n, int status) {
    int r = s[0].r, ru = s[0].ru;
    int ml_min = 1 << 30, ml_max = 0, mu_max = 0, pl_min = 1 << 30, pl_max = 0, pu_max = 0;
    for (int i = 0; i < n; ++i) {
      if (s[i].r != r || s[i].ru != ru) r = 0;
      const bool mid = s[i].rl_mid > 0 && s[i].ru_mid > 0, pre = s[i].rl_pre > 0 && s[i].ru_pre > 0;
      const int ml = mid ? s[i].rl_mid : 0, mu = mid ? s[i].ru_mid : 0, pl = pre ? s[i].rl_pre : 0, pu = pre ? s[i].ru_pre : 0;
      ml_min = std::min(ml_min, ml); ml_max = std::max(ml_max, ml); mu_max = std::max(mu_max, mu);
      pl_min = std::min(pl_min, pl); pl_max = std::max(pl_max, pl); pu_max = std::max(pu_max, pu);
    }
    return RankVote{{r, -r, ru, -ru, ml_min, -ml_max, -mu_max, pl_min, -pl_max, -pu_max, status, 0}};
  }
  // all: the gathered votes [world][SLOTS]
  void reduce(const int32_t* all, int world) {
    for (int w = 0; w < world; ++w)
      for (int j = 0; j < SLOTS; ++j) v[j] = std::min(v[j], all[(size_t)w * SLOTS + j]);
  }
  // (min == max: every rank reported that value)
  Ranks unpack() const {
    Ranks a;
    a.r = (v[R_MIN] == -v[R_NEG_MAX] && v[RU_MIN] == -v[RU_NEG_MAX]) ? v[R_MIN] : 0;
    a.ru = v[RU_MIN];
    if (v[MID_L_MIN] > 0) { a.rl_mid = -v[MID_L_NEG_MAX]; a.ru_mid = -v[MID_U_NEG_MAX]; }      // (a rank without the step reports 0: none for everybody)
    if (v[PRE_L_MIN] > 0) { a.rl_pre = -v[PRE_L_NEG_MAX]; a.ru_pre = -v[PRE_U_NEG_MAX]; }
    a.status = v[STATUS];
    return a;
  }
};
static_assert(sizeof(RankVote) == 48, "the rank vote is 48 bytes on the wire");

// ---- the step's plan -----------------------------------------------------------------------------------------------------------------------------------
// The all-gathers ONE step owes the other ranks, in order, from the agreed ranks alone: [pre], sample, [mid], final -- or the single local block when the
// shards cannot be sampled alike (r <= 0).  The repair block is appended once every rank has read the same number of failed queries.  Fixed storage:
// building a plan cannot fail or allocate, and a rank that fails later still knows what it owes (Step::leave).
struct StepPlan {
  enum Name { PRE, SAMPLE, MID, FINAL, LOCAL, REPAIR, NAMES };
  int Q = 0, k = 0, world = 1;
  bool sampled = false, has_pre = false, has_mid = false;
  int r = 0, ru = 0;              // sample lists are r long; the ru-th best of their union is the common threshold
  int r_pre = 0, ru0 = 0;         // the same for the first round of a two-round first agreement
  int r_mid = 0, ru2 = 0;         // ... and for the second agreement
  int kk = 0;                     // list prefixes of the final gather
  Block b[NAMES];                 // the block of each planned gather
  ListBlock final_, local, repair;      // ... and the sections of those that carry lists
  Name order[NAMES];
  int n = 0;
  StepPlan() {}
  StepPlan(int Q_, int k_, int world_, const Ranks& a) : Q(Q_), k(k_), world(world_) {
    sampled = a.r > 0;
    if (!sampled) { local = list_block(Q, k, false); owe(LOCAL, local.b); return; }
    r = a.r;
    ru = std::min(a.ru, world * r);
    has_pre = a.rl_pre > 0 && a.ru_pre > 0;
    has_mid = a.rl_mid > 0 && a.ru_mid > 0;
    if (has_pre) { r_pre = a.rl_pre; ru0 = std::min(a.ru_pre, world * r_pre); owe(PRE, score_block(Q, r_pre)); }
    owe(SAMPLE, score_block(Q, r));
    if (has_mid) { r_mid = a.rl_mid; ru2 = std::min(a.ru_mid, world * r_mid); owe(MID, score_block(Q, r_mid)); }
    kk = prefix_len(k, world);
    final_ = list_block(Q, kk, true);
    owe(FINAL, final_.b);
  }
  // F failed queries are redone with local thresholds: one more all-gather of full lists
  void add_repair(int F) { repair = list_block(F, k, false); owe(REPAIR, repair.b); }
  const Block& block(Name name) const { return b[name]; }

 private:
  void owe(Name name, const Block& blk) { b[name] = blk; if (n < NAMES) order[n++] = name; }
};

}  // namespace sharded
}  // namespace dhr

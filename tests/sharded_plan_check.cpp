// The invariants of the sharded step's plan (dhr_amd/csrc/sharded_plan.h) over a grid of batch sizes, k, world sizes and ranks, on the CPU.
// Built and run by tests/test_sharded_plan.py with -fsanitize=address,undefined; includes nothing of the library but that header.
#include "sharded_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace dhr::sharded;

static long n_checked = 0;
static int g_Q = 0, g_k = 0, g_world = 0;
#define CHECK(cond)                                                                                                     \
  do {                                                                                                                  \
    ++n_checked;                                                                                                        \
    if (!(cond)) {                                                                                                      \
      std::fprintf(stderr, "FAILED %s (line %d): Q %d k %d world %d\n", #cond, __LINE__, g_Q, g_k, g_world);             \
      std::exit(1);                                                                                                     \
    }                                                                                                                   \
  } while (0)

static bool same(const Block& a, const Block& b) { return a.payload == b.payload && a.stride == b.stride; }
static void check_block(const Block& b, size_t content) {
  CHECK(b.payload % 16 == 0 && b.payload >= content && b.payload < content + 16);
  CHECK(b.stride % 256 == 0 && b.stride >= b.payload + 16 && b.stride < b.payload + 16 + 256);
}

// sections [counts] | scores | rows: aligned, in this order, inside the payload, not overlapping
static void check_list(const ListBlock& l, int Q, int L, bool with_counts) {
  const size_t counts = with_counts ? (size_t)Q * 4 : 0, scores = (size_t)Q * L * 4, rows = (size_t)Q * L * 8;
  CHECK(l.Q == Q && l.L == L);
  CHECK(l.off_scores % 16 == 0 && l.off_rows % 16 == 0);
  CHECK(l.off_scores >= counts && l.off_scores < counts + 16);
  CHECK(l.off_rows >= l.off_scores + scores && l.off_rows < l.off_scores + scores + 16);
  CHECK(l.off_rows + rows <= l.b.payload);
  check_block(l.b, l.off_rows + rows);
  char* base = nullptr;
  CHECK((char*)l.counts(base) == base && (char*)l.scores(base) == base + l.off_scores && (char*)l.rows(base) == base + l.off_rows);
}

// ---- the rank vote, restated: r survives only if every rank reports the same (r, ru); mid and pre ranks are the maximum over the ranks, or none if
// any rank has none; the status is the minimum
static Ranks restated(const std::vector<std::vector<ShardRanks>>& ranks, const std::vector<int>& status) {
  Ranks a;
  bool same_r = true, all_mid = true, all_pre = true;
  const ShardRanks& first = ranks[0][0];
  a.status = status[0];
  for (size_t w = 0; w < ranks.size(); ++w) {
    a.status = std::min(a.status, status[w]);
    for (const ShardRanks& s : ranks[w]) {
      if (s.r != first.r || s.ru != first.ru) same_r = false;
      const bool mid = s.rl_mid > 0 && s.ru_mid > 0, pre = s.rl_pre > 0 && s.ru_pre > 0;
      all_mid = all_mid && mid;
      all_pre = all_pre && pre;
      if (mid) { a.rl_mid = std::max(a.rl_mid, s.rl_mid); a.ru_mid = std::max(a.ru_mid, s.ru_mid); }
      if (pre) { a.rl_pre = std::max(a.rl_pre, s.rl_pre); a.ru_pre = std::max(a.ru_pre, s.ru_pre); }
    }
  }
  a.r = same_r ? first.r : 0;
  a.ru = first.ru;
  if (!all_mid) a.rl_mid = a.ru_mid = 0;
  if (!all_pre) a.rl_pre = a.ru_pre = 0;
  return a;
}

static unsigned long long g_seed = 88172645463325252ull;
static int rnd(int n) {
  g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
  return (int)(g_seed % (unsigned long long)n);
}

static void check_vote(int world, int n_local, int variety) {
  std::vector<std::vector<ShardRanks>> ranks(world, std::vector<ShardRanks>(n_local));
  std::vector<int> status(world, 0);
  const int r = 1 + rnd(100), ru = r + rnd(100);
  for (int w = 0; w < world; ++w) {
    if (variety >= 2 && rnd(world) == 0) status[w] = -(1 + rnd(8));
    for (ShardRanks& s : ranks[w]) {
      s.r = r; s.ru = ru;
      if (variety >= 1 && rnd(3 * world) == 0) s.r += 1;
      if (variety >= 1 && rnd(3 * world) == 0) s.ru += 1;
      s.rl_mid = 20 + rnd(2); s.ru_mid = 60 + rnd(2);
      s.rl_pre = 10 + rnd(2); s.ru_pre = 17 + rnd(2);
      if (variety >= 1 && rnd(2 * world) == 0) s.rl_mid = s.ru_mid = 0;
      if (variety >= 1 && rnd(2 * world) == 0) s.rl_pre = 0;                 // (half a pair counts as none)
      if (variety >= 3) s.rl_mid = s.ru_mid = 0;
      if (variety >= 4) s.rl_pre = s.ru_pre = 0;
    }
  }
  std::vector<int32_t> all((size_t)world * RankVote::SLOTS);
  std::vector<RankVote> sent(world);
  for (int w = 0; w < world; ++w) {
    sent[w] = RankVote::pack(ranks[w].data(), n_local, status[w]);
    CHECK(sent[w].v[RankVote::STATUS] == status[w] && sent[w].v[RankVote::ZERO] == 0);
    for (int j = 0; j < RankVote::SLOTS; ++j) all[(size_t)w * RankVote::SLOTS + j] = sent[w].v[j];
  }
  const Ranks want = restated(ranks, status);
  for (int w = 0; w < world; ++w) {                    // every rank reduces the same gathered votes to the same answer
    RankVote v = sent[w];
    v.reduce(all.data(), world);
    const Ranks got = v.unpack();
    CHECK(got.status == want.status);
    CHECK(got.r == want.r);
    if (got.r > 0) CHECK(got.ru == want.ru);           // (the union rank is only used when r survived)
    CHECK(got.rl_mid == want.rl_mid && got.ru_mid == want.ru_mid);
    CHECK(got.rl_pre == want.rl_pre && got.ru_pre == want.ru_pre);
  }
  // a rank that only reports a failure: zero ranks, its status; everybody reads the status, nothing else survives
  const RankVote bad = RankVote::status_only(-3);
  for (int j = 0; j < RankVote::SLOTS; ++j) CHECK(bad.v[j] == (j == RankVote::STATUS ? -3 : 0));
  if (world > 1 && want.status == 0) {
    for (int j = 0; j < RankVote::SLOTS; ++j) all[j] = bad.v[j];
    RankVote v = sent[world - 1];
    v.reduce(all.data(), world);
    CHECK(v.unpack().status == -3);
  }
}

static void check_plan(int Q, int k, int world, const Ranks& a) {
  const StepPlan p(Q, k, world, a);
  CHECK(p.Q == Q && p.k == k && p.world == world);
  if (a.r <= 0) {
    CHECK(!p.sampled && p.n == 1 && p.order[0] == StepPlan::LOCAL);
    check_list(p.local, Q, k, false);
    CHECK(same(p.block(StepPlan::LOCAL), p.local.b));
    return;
  }
  const bool pre = a.rl_pre > 0 && a.ru_pre > 0, mid = a.rl_mid > 0 && a.ru_mid > 0;
  CHECK(p.sampled && p.has_pre == pre && p.has_mid == mid);
  StepPlan::Name want[4];
  int n = 0;
  if (pre) want[n++] = StepPlan::PRE;
  want[n++] = StepPlan::SAMPLE;
  if (mid) want[n++] = StepPlan::MID;
  want[n++] = StepPlan::FINAL;
  CHECK(p.n == n);
  for (int i = 0; i < n; ++i) CHECK(p.order[i] == want[i]);
  CHECK(p.r == a.r && p.ru == std::min(a.ru, world * a.r) && p.ru >= 1 && p.ru <= world * p.r);
  check_block(p.block(StepPlan::SAMPLE), (size_t)Q * p.r * 4);
  if (pre) {
    CHECK(p.r_pre == a.rl_pre && p.ru0 == std::min(a.ru_pre, world * a.rl_pre));
    check_block(p.block(StepPlan::PRE), (size_t)Q * p.r_pre * 4);
  }
  if (mid) {
    CHECK(p.r_mid == a.rl_mid && p.ru2 == std::min(a.ru_mid, world * a.rl_mid));
    check_block(p.block(StepPlan::MID), (size_t)Q * p.r_mid * 4);
  }
  CHECK(p.kk == prefix_len(k, world));
  check_list(p.final_, Q, p.kk, true);
  CHECK(same(p.block(StepPlan::FINAL), p.final_.b));
  // the repair block is appended once F is known, behind everything else
  for (int F = 1; F <= Q; F += std::max(1, Q / 3)) {
    StepPlan q = p;
    q.add_repair(F);
    CHECK(q.n == n + 1 && q.order[n] == StepPlan::REPAIR);
    for (int i = 0; i < n; ++i) CHECK(q.order[i] == want[i]);
    check_list(q.repair, F, k, false);
    CHECK(same(q.block(StepPlan::REPAIR), q.repair.b));
  }
}

int main() {
  static_assert(sizeof(RankVote) == 48, "48 bytes on the wire");
  const int Qs[] = {1, 2, 3, 5, 7, 16, 33, 100, 257}, ks[] = {1, 5, 10, 60, 63, 64, 65, 100, 300, 1000, 4097, 16385};
  for (int world = 1; world <= 70; ++world) {
    for (int k : ks) {
      g_k = k; g_world = world; g_Q = 0;
      const int kk = prefix_len(k, world);
      if (world <= 2) CHECK(kk == k);
      else CHECK(kk <= k && kk >= 1 && (kk == k || kk % 64 == 0) && (kk == k || (long long)kk * world >= 3LL * k));
      for (int Q : Qs) {
        g_Q = Q;
        const int rs[] = {0, -1, 1, 6, 27, 40, k};
        for (int r : rs)
          for (int stages = 0; stages < 4; ++stages) {
            Ranks a;
            a.r = r; a.ru = std::max(r, 64);
            if (stages & 1) { a.rl_pre = 10; a.ru_pre = 17; }
            if (stages & 2) { a.rl_mid = 21; a.ru_mid = 60; }
            check_plan(Q, k, world, a);
          }
      }
    }
    for (int n_local : {1, 3})
      for (int variety = 0; variety < 5; ++variety)
        for (int rep = 0; rep < 20; ++rep) check_vote(world, n_local, variety);
  }
  std::printf("sharded plan ok: %ld checks\n", n_checked);
  return 0;
}

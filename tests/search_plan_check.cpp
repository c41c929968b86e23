// The invariants of the search plan (dhr_amd/csrc/search_plan.h) over a grid of corpus sizes, k and handle parameters, on the CPU.
// Built and run by tests/test_search_plan.py with -fsanitize=address,undefined; includes nothing of the library but that header.
#include "search_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace dhr::plan;

static long n_checked = 0;
#define CHECK(cond)                                                                                                                     \
  do {                                                                                                                                  \
    ++n_checked;                                                                                                                        \
    if (!(cond)) {                                                                                                                      \
      std::fprintf(stderr, "FAILED %s (line %d): n_rows %lld k %d period %d share %d first_rows %lld staged %d depth %d\n", #cond, __LINE__, \
                   (long long)in.n_rows, in.k, in.sample_period, in.sample_share, (long long)in.first_rows, (int)in.staged, in.depth);  \
      std::exit(1);                                                                                                                     \
    }                                                                                                                                   \
  } while (0)

static void check(const PlanInput& in) {
  const SearchPlan p = make_search_plan(in);
  const int k = in.k;
  CHECK(p.S == 0 || p.S == 4 || p.S == 8 || p.S == 16 || p.S == 32);
  CHECK(1 <= p.r_eff && p.r_eff <= p.r && p.r <= k);
  CHECK(in.staged || p.r_eff == p.r);                     // a whole search chases the union rank itself
  if (in.depth == 2) CHECK(p.S == 0 && !p.sampled && !p.bootstrap);
  if (p.S == 0) CHECK(p.r == k && !p.sampled);
  CHECK(p.head >= 0 && p.head * TILE_ROWS == p.first && p.head + p.rest == in.n_tiles);
  CHECK(p.first_valid <= p.first && p.first_valid <= in.n_rows);
  if (p.sampled) {
    CHECK(p.head + p.n_sample + p.n_main == in.n_tiles);
    CHECK(p.n_sample > 0 && p.n_main >= 0);
    CHECK(p.sample_rows == p.first_valid + p.n_sample * TILE_ROWS);
  } else {
    CHECK(p.n_sample == 0 && p.n_main == 0 && p.pre_positions == 0 && p.mid_offset == 0);
  }
  if (p.bootstrap) {
    CHECK(p.S >= 2 && p.first == 0 && p.boot_r0 >= 1 && p.boot_r0 <= BOOT_M && p.boot_m >= p.boot_r0 && p.boot_m <= BOOT_M);
  } else {
    CHECK(p.boot_r0 == 0 && p.boot_m == 0);
    CHECK(p.first_valid >= std::min<int64_t>(in.n_rows, 2 * (int64_t)p.r_eff));      // tau exists after the head
  }
  CHECK(1 <= p.head_rank && p.head_rank <= p.r_eff);
  // pre step
  CHECK(p.pre_positions % DOC_GROUP == 0 && (p.pre_positions == 0 || p.pre_positions < p.n_sample));
  if (p.pre_positions > 0) {
    CHECK(p.pre_phi > 0.0 && p.pre_phi < 1.0);
    CHECK(1 <= p.pre_local && p.pre_local <= p.pre_union && p.pre_union <= p.r && p.pre_union <= k);
  } else {
    CHECK(p.pre_local == 0 && p.pre_union == 0);
  }
  // mid step
  CHECK(p.mid_offset % DOC_GROUP == 0 && p.mid_offset <= p.n_main);
  if (p.mid_offset > 0) {
    CHECK(p.mid_f > 0.0 && p.mid_f <= 1.0);
    CHECK(1 <= p.mid_local && p.mid_local <= p.mid_union && p.mid_union <= k);
    CHECK(p.perm_mul >= 1 && p.perm_mul % 2 == 1);
  } else {
    CHECK(p.mid_local == 0 && p.mid_union == 0 && p.perm_mul == 1);
  }
  // chunk bounds of the main pass: non-decreasing, whole tile groups (the last chunk ends at n_main whatever its remainder), from the mid offset to n_main
  for (int64_t off : {(int64_t)0, p.mid_offset})
    for (int M = 1; M <= 24; ++M) {
      const std::vector<int64_t> b = main_chunk_bounds(p.n_main, M, off);
      CHECK((int)b.size() == M + 1 && b.front() == off && b.back() == p.n_main);
      for (int i = 0; i < M; ++i) CHECK(b[i] <= b[i + 1]);
      for (int i = 0; i <= M; ++i) CHECK(b[i] % DOC_GROUP == 0 || b[i] == p.n_main);
    }
}

int main() {
  // the helper formulas at their edges
  {
    PlanInput in;      // (CHECK prints it)
    CHECK(share_rank(64, 1) == 64 && share_rank(64, 8) == 27 && share_rank(1, 8) == 1 && share_rank(0, 8) == 0);
    CHECK(adaptive_rank(64, 1.0) == 64 && adaptive_rank(64, 2.0) == 64 && adaptive_rank(64, -1.0) == 4 && adaptive_rank(1, 0.5) == 1);
    CHECK(extrapolated_rank(1000, 0.0) == 4 && extrapolated_rank(1000, 1.0) == 1004);
  }
  const int64_t rows[] = {1, 255, 256, 257, 5000, 40000, 80000, 300000, 8841823};
  const int ks[] = {1, 10, 100, 1000, 10000};
  const int periods[] = {0, 4, 32};
  const int shares[] = {1, 8};
  const int64_t firsts[] = {0, 2048};
  long sampled = 0, boots = 0, pres = 0, mids = 0;
  for (int64_t n : rows)
    for (int k : ks)
      for (int period : periods)
        for (int share : shares)
          for (int64_t first_rows : firsts)
            for (int staged = 0; staged < 2; ++staged)
              for (int depth : {0, 2}) {
                PlanInput in;
                in.n_rows = n; in.n_tiles = (n + TILE_ROWS - 1) / TILE_ROWS; in.k = k; in.sample_period = period; in.sample_share = share;
                in.first_rows = first_rows; in.depth = depth; in.staged = staged != 0;
                check(in);
                const SearchPlan p = make_search_plan(in);
                sampled += p.sampled; boots += p.bootstrap; pres += p.pre_positions > 0; mids += p.mid_offset > 0;
              }
  {
    PlanInput in;
    CHECK(sampled > 0 && boots > 0 && pres > 0 && mids > 0);      // the grid reaches every branch of the plan
  }
  std::printf("search plan ok: %ld checks (%ld sampled plans, %ld with a bootstrap, %ld with a pre step, %ld with a mid step)\n", n_checked, sampled, boots,
              pres, mids);
  return 0;
}

// The geometry of one search, computed ONCE: the controller (search_core.hip) and the exported rank queries (api.hip) read
// a SearchPlan and derive nothing of it themselves -- a shard that reported a rank its own controller does not chase would silently lose the
// bound's guarantee.  Plain C++17, no HIP: tests/search_plan_check.cpp checks the invariants over a grid on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#ifndef DHR_DOC_GROUP
#define DHR_DOC_GROUP 4
#endif
namespace dhr {
namespace plan {
// (the library's constants of the same names, dhr_internal.h: dhr_state.h asserts that they agree)
constexpr int TILE_ROWS = 256;
constexpr int DOC_GROUP = DHR_DOC_GROUP;
constexpr int BOOT_M = 64;       // most rows the threshold bootstrap rescores per query
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// A 1 / shares part of a set holds ~Binomial(r, 1 / shares) of the set's r best: its r / shares + 5 sqrt(r / shares) + 4 best cover them (4 sigma
// until round 2: one query in ~50 000 failed, and a failed query costs its whole query tile extra passes).  The rank of the sampled threshold
// (shares = S), and a shard's share of the rank that defines the common threshold in the UNION of the shards' samples (27 of 64 at 8 shards).
inline int share_rank(int r, int shares) {
  if (shares <= 1 || r <= 0) return r;
  const double m = (double)r / shares;
  return std::min(r, (int)std::ceil(m + 5.0 * std::sqrt(m) + 4.0));
}
// Of a set's k best rows a scattered fraction f holds k f +- sqrt(k f (1 - f)), so the (k f + 6 sigma + 4)-th best seen lies below the set's final
// k-th best except with negligible probability (Poisson tail < 1e-8 per check; a query for which it does not fails the final verification and is
// redone: 6 sigma, a failure costs its query tile a whole extra pass).  adaptive_rank: the rank that defines the threshold of a sampled run after
// the fraction phi of the sample; the same rank extrapolates the thresholds of the main pass from the fraction of the corpus seen.
inline int extrapolated_rank(int k, double f) { return (int)std::ceil((double)k * f + 6.0 * std::sqrt((double)k * f * (1.0 - f)) + 4.0); }
inline int adaptive_rank(int r, double phi) {
  if (!(phi < 1.0)) return r;
  if (phi < 0.0) phi = 0.0;
  return std::max(1, std::min(r, extrapolated_rank(r, phi)));
}
// Share of the SAMPLE that dhr_search_pre streams, and of the MAIN PASS that dhr_search_mid runs, before the shards agree, in 1/16ths (round 6
// swept pre 2 / 4 and mid 1 / 2 / 3 on the emulated 8-shard step: 18.1-18.6 ms, inside the box-to-box noise, profiles/r06_shard_sim.txt)
constexpr int PRE_SHARE16 = 2, MID_SHARE16 = 2;
struct PlanInput {
  int64_t n_rows = 0, n_tiles = 0, first_rows = 0;      // first_rows: DHR_PARAM_FIRST_ROWS (0: default)
  int k = 0, sample_period = 0, sample_share = 1;       // DHR_PARAM_SAMPLE_PERIOD / _SAMPLE_SHARE of the handle
  int depth = 0;                                        // 0: first attempt; 1: the same with deeper lists; 2: plain streaming, exact for any input (no sampling)
  bool staged = false;                                  // a staged call or a rank query: the handle chases its SHARE of the union's rank
};
struct SearchPlan {
  int S = 0;                  // sample period: 0 = no sampling, else every S-th tile behind the head is a sample tile
  int r = 0, r_eff = 0;       // rank of the sampled threshold in the union of the shards' samples, and the rank THIS handle chases (k, k without sampling)
  bool sampled = false;       // S >= 2 and there are tiles behind the head: sampled run + main pass (else: plain streaming)
  bool bootstrap = false;     // phase 0 seeds the thresholds from the bound GEMM over tile 0 (no exhaustive head)
  int boot_r0 = 0, boot_m = 0;      // ... the boot_r0-th best exact score of the boot_m best rows by bound
  int64_t first = 0, first_valid = 0;      // rows of the exhaustive head (whole tiles / real rows)
  int head_rank = 0;          // rank of the threshold after the head: the head is the first part of the sample (adaptive_rank); r_eff without sampling
  int64_t head = 0, rest = 0, n_sample = 0, n_main = 0;      // in tiles: head + rest = n_tiles; sampled: rest = n_sample + n_main
  int64_t sample_rows = 0;    // rows of the whole sample, head included (what the rank of the sampled run grows over)
  // pre step (dhr_search_pre): the first pre_positions sample positions, a fraction pre_phi of the sample; 0 = the sample is too small to split
  int64_t pre_positions = 0; double pre_phi = 0.0; int pre_union = 0, pre_local = 0;
  // mid step (dhr_search_mid): main-pass positions [0, mid_offset), after which the fraction mid_f of the corpus has been seen; 0 = no such step
  int64_t mid_offset = 0; double mid_f = 0.0; int mid_union = 0, mid_local = 0;
  int64_t perm_mul = 1;       // scattered order of the main pass: position i -> tile i * perm_mul mod n_main (~0.618 n_main, coprime); 1 where n_main < 64
};
inline SearchPlan make_search_plan(const PlanInput& in) {
  SearchPlan p;
  const int k = in.k;
  // Sample period and rank: the configured period, halved (32 -> 16 -> 8 -> 4) while the corpus is too small for it -- the sample must span
  // >= 32 tiles and hold >= 16 r rows, and r must stay below k; S = 0 (r = k): no sampling, plain streaming.
  p.r = k;
  if (in.depth < 2) {
    for (int S = in.sample_period; S >= 2; S = S >= 8 ? S / 2 : 0) {
      const int rr = share_rank(k, S);
      const int64_t head_guess = round_up(std::max<int64_t>(256, 2 * (int64_t)rr), TILE_ROWS) / TILE_ROWS;
      const int64_t rest_guess = in.n_tiles - head_guess;
      if (!(rr >= k || rest_guess < 32 * (int64_t)S || (rest_guess / S) * TILE_ROWS < 16 * (int64_t)rr)) { p.S = S; p.r = rr; break; }
    }
  }
  // A stage-0 search chases r itself, even on a handle whose sample share is above 1 (the repair dhr_search inside a sharded step)
  p.r_eff = (p.S >= 2 && in.staged) ? share_rank(p.r, in.sample_share) : p.r;
  // Phase 0.  A SAMPLED search seeds its thresholds without an exhaustive head, unless the caller fixed one (DHR_PARAM_FIRST_ROWS): ONE corpus
  // tile through the bound GEMM with an open filter, the boot_m best rows of every query BY BOUND rescored exactly, and the r0-th best of those
  // exact scores is the first threshold (adaptive_rank's argument with phi = 256 rows of the sample).  It takes the r0-th
  // best of at most BOOT_M rows: a sampling rule under which r0 outgrows that (today r0 <= 44) must not publish the threshold of a lower rank
  // -- it falls back to the exhaustive head.  Else: rows scored exhaustively (>= the rank that defines tau, so that tau exists afterwards),
  // whole tiles: 256 with sampled thresholds (the head only has to hold 2 r rows, and it is a fixed cost of every shard), else 512.
  if (p.S >= 2 && in.first_rows <= 0 && in.n_tiles >= 8) {
    const int64_t rows = ((in.n_tiles + p.S - 1) / p.S) * TILE_ROWS;
    const int r0 = adaptive_rank(p.r_eff, (double)TILE_ROWS / (double)rows);
    if (r0 <= BOOT_M) { p.bootstrap = true; p.boot_r0 = r0; p.boot_m = std::min(BOOT_M, std::max(16, 2 * r0)); }
  }
  int64_t first = 0;
  if (!p.bootstrap)
    first = in.first_rows > 0 ? std::max<int64_t>(in.first_rows, 2 * (int64_t)p.r_eff) : std::max<int64_t>(p.S >= 2 ? 256 : 512, 2 * (int64_t)p.r_eff);
  p.first = std::min(round_up(first, TILE_ROWS), round_up(in.n_rows, TILE_ROWS));
  p.first_valid = std::min(p.first, in.n_rows);
  p.head = p.first / TILE_ROWS;
  p.rest = in.n_tiles - p.head;
  p.head_rank = p.r_eff;
  p.sampled = p.S >= 2 && p.rest > 0;
  if (!p.sampled) return p;
  p.n_sample = (p.rest + p.S - 1) / p.S;
  p.n_main = p.rest - p.n_sample;
  p.sample_rows = p.first_valid + p.n_sample * TILE_ROWS;
  if (!p.bootstrap) p.head_rank = adaptive_rank(p.r_eff, (double)p.first_valid / (double)p.sample_rows);
  // pre step: whole tile groups
  if (p.n_sample >= 64) {
    const int64_t a = round_up(std::max<int64_t>(DOC_GROUP, p.n_sample * PRE_SHARE16 / 16), DOC_GROUP);
    if (a < p.n_sample) {
      p.pre_positions = a;
      p.pre_phi = (double)(p.first_valid + a * TILE_ROWS) / (double)p.sample_rows;
      p.pre_union = adaptive_rank(p.r, p.pre_phi);
      p.pre_local = share_rank(p.pre_union, in.sample_share);
    }
  }
  if (p.n_main >= 64) {
    // mid step: the union of what the shards have seen holds k f +- sqrt(k f (1 - f)) of the final top-k, so its (k f + 6 sigma + 4)-th best score
    // lies below the final k-th best (the counts verify it; a failure is repaired like any other).  A shard reports its share of that rank.
    p.mid_offset = std::min<int64_t>(p.n_main, round_up(p.n_main * MID_SHARE16 / 16, DOC_GROUP));
    p.mid_f = (double)(p.head + p.n_sample + p.mid_offset) / (double)in.n_tiles;
    p.mid_union = std::min(k, extrapolated_rank(k, p.mid_f));      // (clamped; the main pass instead skips a raise whose rank reaches k)
    p.mid_local = share_rank(p.mid_union, in.sample_share);
    p.perm_mul = (int64_t)(0.6180339887 * (double)p.n_main) | 1;
    auto gcd = [](int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; };
    while (gcd(p.perm_mul, p.n_main) != 1) p.perm_mul += 2;
  }
  return p;
}
// Chunk i of the main pass covers positions [b[i], b[i + 1]), b[0] = mid_offset (what a mid step already ran; else 0), b[M_plain] = n_main:
// sizes fall off linearly (weights M, M-1, ..., 1 on top of an equal share) so that the refine / rescoring tail that cannot overlap a GEMM
// (the last chunk's) is short.  (The chunk COUNT depends on run-time rates and on the workspace: it stays in the controller.)
inline std::vector<int64_t> main_chunk_bounds(int64_t n_main, int M_plain, int64_t mid_offset) {
  std::vector<int64_t> b((size_t)M_plain + 1, 0);
  b[0] = mid_offset;
  double acc = 0.0, tot = 0.0;
  for (int i = 0; i < M_plain; ++i) tot += 1.0 + 2.0 * (M_plain - 1 - i) / std::max(1, M_plain - 1);
  for (int i = 0; i < M_plain; ++i) {
    acc += 1.0 + 2.0 * (M_plain - 1 - i) / std::max(1, M_plain - 1);
    b[(size_t)i + 1] = std::min<int64_t>(n_main, mid_offset + round_up((int64_t)((n_main - mid_offset) * acc / tot), DOC_GROUP));
  }
  b[(size_t)M_plain] = n_main;
  return b;
}

}  // namespace plan
}  // namespace dhr

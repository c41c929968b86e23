// dhr_amd/csrc/lexical_proj_layout.h on its own: the workspace layout of the lexical heads with the projection fused in, over the grid of
// tests/golden/make_golden_lexical_entry_points.py.  Built as host C++ with AddressSanitizer and UBSan and run as a plain executable
// (tests/test_lexical_entry_points.py); the header is included alone, so it cannot lean on a HIP include.
#include "lexical_proj_layout.h"

#include <cstdio>
#include <cstdlib>

static long long checks = 0;
#define CHECK(cond)                                                                                                     \
  do {                                                                                                                  \
    ++checks;                                                                                                           \
    if (!(cond)) {                                                                                                      \
      std::printf("FAILED %s (line %d) at B=%lld T=%d V=%d H=%d\n", #cond, __LINE__, (long long)B, T, V, H);          \
      return 1;                                                                                                         \
    }                                                                                                                   \
  } while (0)

// the sections both heads share: aligned, in order, each at least as large as its use (the comments of ProjArgs in lexical_proj_common.h)
static int check_prefix(const ProjLayout& l, int64_t B, int T, int V, int H) {
  const int64_t BT = B * T;
  const int64_t at[] = {l.hdr, l.cnt, l.start, l.tmask, l.rows, l.stats, l.part, l.end};
  const int64_t use[] = {4, 4 * B, 4 * (B + 1), 4 * B, 4 * BT, 16 * BT, 8 * BT * l.n_split};      // hdr[0]; cnt[B]; start[B + 1]; tmask[B]; rows, stats: at most
  CHECK(l.hdr == 0);                                                                                // B * T unmasked rows; part[n_split][B * T] float2
  for (int i = 0; i < 8; ++i) CHECK(at[i] % 256 == 0);
  for (int i = 0; i < 7; ++i) CHECK(at[i] + use[i] <= at[i + 1]);
  CHECK(l.n_ntiles == (V + 255) / 256);
  CHECK(l.n_split >= 1 && l.n_split <= MAX_SPLIT && l.n_split <= l.n_ntiles);
  return 0;
}

static int check_shape(int64_t B, int T, int V, int H) {
  const int64_t BT = B * T;
  const ProjLayout p = proj_layout(B, T, V);
  if (check_prefix(p, B, T, V, H)) return 1;
  for (int with_reps = 0; with_reps < 2; ++with_reps) {
    const ProjEncodeLayout e = proj_encode_layout(B, T, V, with_reps != 0);
    if (check_prefix(e, B, T, V, H)) return 1;
    CHECK(e.hdr == p.hdr && e.cnt == p.cnt && e.start == p.start && e.tmask == p.tmask && e.rows == p.rows && e.stats == p.stats && e.part == p.part &&
          e.end == p.end && e.n_split == p.n_split && e.n_ntiles == p.n_ntiles);
    CHECK(e.reps == e.end && e.total % 256 == 0);
    CHECK(with_reps ? e.reps + 4 * B * V <= e.total : e.total == e.reps);                           // reps[B][V] fp32
  }
  const ProjTrainLayout t = proj_train_layout(B, T, V, H);
  if (check_prefix(t, B, T, V, H)) return 1;
  CHECK(t.hdr == p.hdr && t.cnt == p.cnt && t.start == p.start && t.tmask == p.tmask && t.rows == p.rows && t.stats == p.stats && t.part == p.part &&
        t.end == p.end && t.n_split == p.n_split && t.n_ntiles == p.n_ntiles);
  CHECK(t.D == t.end && t.partial % 256 == 0 && t.total % 256 == 0);
  CHECK(t.D + 4 * BT <= t.partial);                                                                  // D[B * T] fp32
  CHECK(t.grad_split >= 1 && t.grad_split <= MAX_SPLIT && t.grad_split <= t.n_ntiles);
  CHECK(t.grad_split > 1 ? t.partial + 4 * BT * H * t.grad_split <= t.total : t.total == t.partial); // partial[grad_split][B * T][H] fp32
  return 0;
}

// totals as dhr_lexical_proj_workspace (raw, with reps) and dhr_lexical_proj_train_workspace returned them before the layouts were shared
// (tests/golden/lexical_entry_points.json).  The third row by hand: 18 token rows, 2 vocabulary tiles, 2 shares; hdr 0, cnt 256, start 512,
// tmask 768, rows 1024, stats 1280 (+ 72 -> 1352), part 1792 (+ 288 -> 1568), end 2304 (+ 288 -> 2080); reps + 3600 -> 6144; D 2304, partial 2560,
// two shares of 18 * 72 floats + 10368 -> 13056.
struct Pinned {
  int64_t B;
  int T, V, H;
  int64_t raw, with_reps, train;
};
static const Pinned PINNED[] = {
    {0, 1, 1, 8, 512, 512, 512},
    {1, 1, 1, 1024, 1792, 2048, 2048},
    {3, 6, 300, 72, 2304, 6144, 13056},
    {3, 6, 300, 768, 2304, 6144, 113152},
    {3, 6, 30522, 1024, 4096, 370432, 1184000},
    {700, 512, 30522, 768, 10043904, 95505664, 11477504},
    {70000, 6, 257, 8, 12600576, 84560640, 14280704},
    {1, 32767, 256, 72, 918528, 919552, 1049600},
};

int main() {
  const int64_t Bs[] = {0, 1, 3, 700, 70000};
  const int Ts[] = {1, 6, 512, 32767, 32768}, Vs[] = {1, 256, 257, 300, 30522}, Hs[] = {8, 72, 768, 776, 1024, 1032};
  for (int64_t B : Bs)
    for (int T : Ts)
      for (int V : Vs)
        for (int H : Hs) {
          if (B * T > ((int64_t)1 << 31) - 1) continue;                                             // refused by every entry point
          if (check_shape(B, T, V, H)) return 1;
        }
  for (const Pinned& q : PINNED) {
    const int64_t B = q.B;
    const int T = q.T, V = q.V, H = q.H;
    CHECK(proj_encode_layout(B, T, V, false).total == q.raw);
    CHECK(proj_encode_layout(B, T, V, true).total == q.with_reps);
    CHECK(proj_train_layout(B, T, V, H).total == q.train);
  }
  std::printf("lexical proj layout ok: %lld checks\n", checks);
  return 0;
}

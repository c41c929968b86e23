// The invariants of the index layout, the column-step rule and the bucket deal (dhr_amd/csrc/index_layout.h) over a grid of descriptors, on the CPU.
// Built and run by tests/test_index_layout.py with -fsanitize=address,undefined; includes nothing of the library but that header.
#include "index_layout.h"

#include <cstdio>
#include <cstdlib>

using namespace dhr::layout;

static long n_checked = 0;
static LayoutInput cur;      // the input under test, for the failure message
#define CHECK(cond)                                                                                                                              \
  do {                                                                                                                                           \
    ++n_checked;                                                                                                                                 \
    if (!(cond)) {                                                                                                                               \
      std::fprintf(stderr, "FAILED %s (line %d): n_rows %lld d_dlr %d d_cls %d index %d dtype %d buckets %d dense_i8 %d gated_i8 %d\n", #cond, __LINE__, \
                   (long long)cur.n_rows, cur.d_dlr, cur.d_cls, (int)cur.index_array, cur.idx_dtype, cur.idx_buckets, cur.want_dense_i8, cur.want_gated_i8); \
      std::exit(1);                                                                                                                              \
    }                                                                                                                                            \
  } while (0)

static bool same(const IndexLayout& a, const IndexLayout& b) {
  return a.has_idx == b.has_idx && a.dlr_pad == b.dlr_pad && a.d_dlr == b.d_dlr && a.k == b.k && a.k_rm == b.k_rm && a.n_tiles == b.n_tiles && a.n_buckets == b.n_buckets &&
         a.ts == b.ts && a.td == b.td && a.kt == b.kt && a.ksteps == b.ksteps && a.dense_i8 == b.dense_i8 && a.dense_only_trial == b.dense_only_trial && a.gated_i8 == b.gated_i8;
}

static void check(const LayoutInput& in) {
  cur = in;
  const IndexLayout L = make_layout(in);
  CHECK(L.has_idx == (in.d_dlr > 0));
  CHECK(L.dlr_pad >= 0 && L.dlr_pad <= 7 && L.d_dlr == in.d_dlr + L.dlr_pad);
  if (L.has_idx) CHECK(L.d_dlr % 8 == 0);
  CHECK(L.ts % 2 == 0 && L.td % 2 == 0);
  CHECK(32 * L.ts >= L.d_dlr && (L.has_idx || L.ts == 0));
  CHECK(L.td * (L.dense_i8 ? 64 : 32) >= in.d_cls);
  CHECK(L.kt == L.ts * 64 + L.td * 32);
  CHECK(L.ksteps == (L.kt + 63) / 64 && L.ksteps * 64 >= L.kt && (L.ksteps - 1) * 64 < L.kt);
  CHECK(L.k == L.d_dlr + in.d_cls && L.k_rm % 64 == 0 && L.k_rm >= L.k && L.k_rm - L.k < 64);
  CHECK(L.n_tiles * TILE_ROWS >= in.n_rows && (L.n_tiles - 1) * TILE_ROWS < in.n_rows);
  CHECK(L.n_buckets == (L.has_idx && in.idx_buckets != 1 ? 2 : 1));
  if (L.gated_i8) CHECK(L.n_buckets == 2 && L.d_dlr <= 4096 && (in.d_cls == 0 || L.dense_i8) && in.want_gated_i8 != 0);
  if (L.dense_i8) CHECK(in.d_cls > 0 && in.want_dense_i8 != 0);
  if (L.dense_only_trial) CHECK(!in.index_array && in.n_rows >= 1000000 && in.d_cls >= 128 && in.want_dense_i8 == -1 && L.dense_i8);
  // a rejected trial (and any other layout) falls back to the layout of the same input with the ungated int8 image off
  LayoutInput off = in;
  off.want_dense_i8 = 0;
  const IndexLayout F = fp16_fallback(L);
  CHECK(same(F, make_layout(off)) && !F.dense_i8 && !F.dense_only_trial && F.td == even_up((in.d_cls + 31) / 32));
  CHECK(L.tile_bytes() == (size_t)L.n_tiles * ((size_t)L.ts * (L.gated_i8 ? 10240 : 18432) + (size_t)L.td * 16384));
  CHECK(L.tile_bytes() == tile_bytes(L.n_tiles, L.ts, L.td, L.gated_i8));
  CHECK(L.refine_lists() == (L.has_idx && L.d_dlr <= 4096));
  CHECK(L.resid_ld() == (in.d_cls + 255) / 256 * 128);
  CHECK(L.has_residual(1.f) == (L.dense_i8 && !L.has_idx && in.d_cls <= 1024) && !L.has_residual(0.f));
  const int sh = L.g8_max_shift();
  CHECK(sh >= 0 && sh <= 7 && (sh == 0 || 255.0 * 127.0 * 32.0 * L.ts * (double)(1 << sh) <= 1073741824.0) && (sh == 7 || 255.0 * 127.0 * 32.0 * L.ts * (double)(2 << sh) > 1073741824.0));
}

static LayoutInput input(int64_t n, int g, int u, int dtype, int buckets = 0, int dense = -1, int gated = -1) {
  LayoutInput in;
  in.n_rows = n; in.d_dlr = g; in.d_cls = u; in.index_array = g > 0; in.idx_dtype = g > 0 ? dtype : 0; in.idx_buckets = buckets; in.want_dense_i8 = dense; in.want_gated_i8 = gated;
  return in;
}

static void check_grid() {
  const int gated[] = {0, 1, 7, 8, 31, 32, 33, 64, 65, 100, 768, 1000, 4096, 4097, 8000}, ungated[] = {0, 1, 31, 32, 33, 64, 127, 128, 129, 768};
  const int64_t rows[] = {1, 255, 256, 257, 999999, 1000000, 3999999, 4000000};
  for (int g : gated)
    for (int u : ungated) {
      if (g + u == 0 || g + dlr_pad_of(g, g > 0) + u > 8192) continue;
      for (int64_t n : rows)
        for (int dense = -1; dense <= 1; ++dense)
          for (int gi8 = -1; gi8 <= 1; ++gi8)
            for (int buckets = 0; buckets <= 2; ++buckets)
              for (int dtype : {1, 3})        // DHR_IDX_U8, DHR_IDX_I16
                if (g > 0 || dtype == 1) check(input(n, g, u, dtype, buckets, dense, gi8));
    }
}

// hand-derived from dhr_index_create as it stood before the layout had a header of its own
static void check_table() {
  IndexLayout L = make_layout(cur = input(8840000, 768, 768, 1));
  CHECK(L.ts == 24 && L.td == 12 && L.kt == 1920 && L.ksteps == 30 && L.dense_i8 && L.gated_i8 && L.n_tiles == 34532 && L.tile_bytes() == (size_t)34532 * 442368);
  L = make_layout(cur = input(5000, 100, 8, 1));
  CHECK(L.dlr_pad == 4 && L.ts == 4 && L.td == 2 && L.kt == 320 && L.ksteps == 5 && L.k == 112 && L.k_rm == 128 && L.dense_i8 && !L.gated_i8 && L.tile_bytes() == (size_t)20 * 106496);
  L = make_layout(cur = input(999999, 0, 768, 0));
  CHECK(L.td == 24 && L.kt == 768 && !L.dense_only_trial && !L.dense_i8);
  L = make_layout(cur = input(1000000, 0, 768, 0));
  CHECK(L.dense_only_trial && L.dense_i8 && L.td == 12 && L.kt == 384);
  L = fp16_fallback(L);
  CHECK(!L.dense_only_trial && !L.dense_i8 && L.td == 24 && L.kt == 768 && L.ksteps == 12);
  L = make_layout(cur = input(5000, 0, 33, 0, 0, 0));
  CHECK(L.td == 2 && L.kt == 64 && L.ksteps == 1);
  L = make_layout(cur = input(5000000, 4104, 0, 1, 0, -1, 1));
  CHECK(!L.gated_i8 && !L.refine_lists() && L.dlr_pad == 0);
  // the trial's verdict: at most 0.45, and anything that is not a number rejects
  CHECK(trial_keeps_i8(256, 0.45f / 16.f, 1.f) && !trial_keeps_i8(256, 0.46f / 16.f, 1.f) && trial_keeps_i8(256, 0.f, 0.f));
  CHECK(!trial_keeps_i8(256, NAN, 1.f) && !trial_keeps_i8(256, 1.f, NAN) && !trial_keeps_i8(256, INFINITY, INFINITY) && !trial_keeps_i8(256, INFINITY, 1.f));
}

static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static uint32_t rng_state = 12345;
static float uniform() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) / 16777216.f; }

static void check_steps() {
  cur = LayoutInput();
  float before = 0.f;
  for (int i = 0; i <= 4096; ++i) {        // the factor: within [1/1024, 1], monotone in the ratio
    const float f = column_step_factor((float)i / 4096.f);
    CHECK(f >= 1.f / 1024.f && f <= 1.f && f >= before);
    before = f;
  }
  CHECK(column_step_factor(1.f) == 1.f && column_step_factor(0.f) == 1.f / 1024.f);
  for (int round = 0; round < 200; ++round) {
    const size_t n = 1 + (size_t)(uniform() * 300.f);
    const float top = std::ldexp(1.f + uniform(), (int)(uniform() * 24.f) - 12);
    std::vector<float> maxima(n);
    std::vector<uint32_t> cm(n);
    for (size_t j = 0; j < n; ++j) {        // a wide range of column maxima, some zero columns, one column at the top
      const float u = uniform();
      maxima[j] = j == n / 2 ? top : u < 0.1f ? 0.f : top * std::ldexp(uniform(), -(int)(uniform() * 20.f));
      cm[j] = bits_of(maxima[j]);
    }
    // ungated: the scale covers the largest column (or a larger gated value); no step exceeds it, and a column's values fit 127 of its steps (with the rule's own floor)
    const float i8_scale = std::max(top / 127.f, round % 3 ? 0.f : top / 100.f);
    const std::vector<float> cs = ungated_steps(cm, i8_scale);
    CHECK(cs.size() == n);
    for (size_t j = 0; j < n; ++j) {
      CHECK(cs[j] <= i8_scale && cs[j] >= i8_scale / 1024.f);
      if (maxima[j] == 0.f) CHECK(cs[j] == i8_scale);          // a zero column gets ratio 1
      CHECK(maxima[j] / cs[j] <= 127.f * 1.0001f);
    }
    const GatedSteps g = gated_steps(cm, top);
    CHECK(g.inv_cs.size() == n && g.w.size() == n && g.sref == top * (1.00001f / 127.f));
    for (size_t j = 0; j < n; ++j) {
      CHECK(maxima[j] * g.inv_cs[j] <= 127.f * 1.0001f);
      CHECK(g.w[j] >= 1.f / 1024.f && g.w[j] <= 1.000001f);
      if (maxima[j] == 0.f) CHECK(g.w[j] == 1.000001f && g.inv_cs[j] == 1.000001f / g.sref);
    }
  }
  const GatedSteps z = gated_steps(std::vector<uint32_t>(5, 0u), 0.f);          // an all-zero gated half
  CHECK(z.sref == 1.00001f / 127.f && z.w[0] == 1.000001f);
}

static void check_bucket_map() {
  cur = LayoutInput();
  const int d = 6;
  std::vector<float> hist((size_t)d * 256, 0.f);
  for (int v = 0; v < 256; ++v) {
    hist[1 * 256 + v] = 3.5f;                                   // slice 1: equal masses
    hist[2 * 256 + v] = v % 3 == 0 ? 1.f + (float)v : 0.f;      // slice 2: two thirds of the values unseen
    hist[3 * 256 + v] = uniform() * 100.f;                      // slices 3-5: random masses, some unseen, one dominant
    hist[4 * 256 + v] = uniform() < 0.5f ? 0.f : std::ldexp(uniform(), (int)(uniform() * 16.f));
    hist[5 * 256 + v] = v == 77 ? 1e6f : uniform();
  }
  for (int nb = 1; nb <= 2; ++nb) {
    std::vector<uint8_t> map;
    build_bucket_map(hist, d, nb, map);
    CHECK(map.size() == (size_t)d * 256);
    for (size_t i = 0; i < map.size(); ++i) CHECK(map[i] < nb);
    if (nb == 1) continue;
    for (int v = 0; v < 256; ++v) CHECK(map[v] == v % 2);              // slice 0: nothing seen, round robin in value order
    for (int v = 0; v < 256; ++v) CHECK(map[256 + v] == v % 2);        // slice 1: equal masses are dealt in value order, ties to the lowest bucket
    int unseen = 0;
    for (int v = 0; v < 256; ++v)
      if (hist[2 * 256 + v] == 0.f) CHECK(map[2 * 256 + v] == unseen++ % 2);      // unseen values alternate
    for (int j = 1; j < d; ++j) {
      double load[2] = {0.0, 0.0}, top = 0.0;
      for (int v = 0; v < 256; ++v) { load[map[(size_t)j * 256 + v]] += hist[(size_t)j * 256 + v]; top = std::max(top, (double)hist[(size_t)j * 256 + v]); }
      CHECK(std::fabs(load[0] - load[1]) <= top);
    }
  }
}

int main() {
  check_grid();
  check_table();
  check_steps();
  check_bucket_map();
  std::printf("index layout ok: %ld checks\n", n_checked);
  return 0;
}

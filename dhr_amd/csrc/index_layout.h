// The layout of one index, computed ONCE before the build touches the device: dhr_index_create (index_build.hip) copies an IndexLayout into the handle and derives nothing of
// it itself; the column-step rule of the two int8 images and the bucket deal are the build's other pure host parts.  Plain C++17, no HIP: tests/index_layout_check.cpp checks them on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
namespace dhr {
namespace layout {
// (the library's constants of the same names, dhr_internal.h: index_build.hip asserts that they agree)
constexpr int TILE_ROWS = 256, TILE_K = 64, HEAVY_KEY_STRIDE = 96;
constexpr int SP_STAGE_A = 16384 + 2048, S8_STAGE_A = 8192 + 2048, SP_DENSE = 16384;      // corpus bytes of a gated fp16 / gated int8 / ungated stage
// Rows from which an index gets the int8 gated image by default (_NARROW: where the ungated half is narrower than half the gated one), and a dense-only index the int8 image on trial
// (trial_keeps_i8): the measured break-even points, DESIGN.md section 3
constexpr int64_t GATED_I8_MIN_ROWS = 1000000, GATED_I8_MIN_ROWS_NARROW = 4000000, DENSE_ONLY_I8_MIN_ROWS = 1000000;
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int even_up(int v) { return v + (v & 1); }
inline float bits_to_float(uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; }      // (the build's kernels leave maxima of non-negative floats as bit patterns: atomicMax on u32)
inline int dlr_pad_of(int d_dlr, bool index_array) { return (d_dlr > 0 && index_array && d_dlr % 8) ? 8 - d_dlr % 8 : 0; }      // zero slices appended to the caller's gated half: its width becomes a multiple of 8 (16-byte operand chunks)
inline int dense_stages(int d_cls, bool i8) { return i8 ? 2 * ((d_cls + 127) / 128) : even_up((d_cls + 31) / 32); }      // ungated columns in 32-column fp16 stages or PAIRS of 64-column int8 stages
inline size_t tile_bytes(int64_t n_tiles, int ts, int td, bool gated_i8) { return (size_t)n_tiles * ((size_t)ts * (gated_i8 ? S8_STAGE_A : SP_STAGE_A) + (size_t)td * SP_DENSE); }
struct LayoutInput {
  int64_t n_rows = 0; int d_dlr = 0, d_cls = 0;   // the CALLER's widths (a valid descriptor: dhr_index_create has checked it)
  bool index_array = false; int idx_dtype = 0, idx_buckets = 0;      // the descriptor has an index pointer; its dhr_idx_dtype (0: none); 0 (default: 2), 1 or 2 buckets
  int want_dense_i8 = -1, want_gated_i8 = -1;     // the two image options, resolved (process option, then environment): -1 default, 0 never, 1 wherever the layout allows
};
struct IndexLayout {
  LayoutInput in;
  bool has_idx = false; int dlr_pad = 0, d_dlr = 0;      // a gated half (an index array with a dtype); dlr_pad_of the caller's gated width, and the PADDED gated width
  int k = 0, k_rm = 0;                 // columns of a record, and of a row of the row-major copy (k rounded up to 64)
  int64_t n_tiles = 0; int n_buckets = 1;      // index buckets per gated slice (idx_buckets = 1: every index value in bucket 0, the ungated bound)
  // ONE layout: stage images -- ts 2:4 sparse stages of 32 gated slices and td stages of 32 (fp16) / 64 (int8) ungated columns, an EVEN number of either kind: gated widths that are no
  // multiple of 64 and odd ungated stage counts are rounded up with all-zero stages (the tile builder and query_prep_kernel write zeros behind d_dlr / d_cls), so that every index runs
  // on the two 8-wave kernels.  ts == 0: a dense-only index.  kt: operand bytes / 2 per row (fp16: logical columns, two bucket columns per gated slice), ksteps: kt in steps of 64.
  int ts = 0, td = 0, kt = 0, ksteps = 0;
  // int8 image of the ungated columns (default: gated indexes, where the gated part dominates the spread of the scores and the int8 margin costs few extra candidates -- DESIGN.md section
  // 6b; dense-only indexes: explicitly, or -- large shards -- ON TRIAL: the build measures the margin the image needs and keeps the fp16 image where that is too large, trial_keeps_i8)
  bool dense_i8 = false, dense_only_trial = false;
  bool gated_i8 = false;      // gated half as int8 on the 2:4 int8 instruction (gemm_g8.hip): default for large shards whose ungated half (if any) is the int8 image too
  size_t tile_bytes() const { return layout::tile_bytes(n_tiles, ts, td, gated_i8); }
  // dense-only int8 index: residual image (four bits per value), where a row of it fits 512 bytes and the int8 image loses anything at all
  int resid_ld() const { return (int)round_up(in.d_cls, 256) / 2; }
  bool has_residual(float i8_ec) const { return dense_i8 && d_dlr == 0 && resid_ld() <= 512 && i8_ec > 0.f; }
  bool refine_lists() const { return has_idx && d_dlr <= 4096; }
  // most bits the gated int8 products of a query may be shifted up by: 255 * 127 * (columns of the gated stages) * 2^(shift + 1) stays within 2^30
  int g8_max_shift() const { int sh = 0; while (sh < 7 && 255.0 * 127.0 * (double)(ts * 32) * (double)(2 << sh) <= 1073741824.0) ++sh; return sh; }
};
inline IndexLayout make_layout(const LayoutInput& in) {
  IndexLayout L;
  L.in = in; L.has_idx = in.index_array && in.idx_dtype != 0;
  L.dlr_pad = dlr_pad_of(in.d_dlr, in.index_array); L.d_dlr = in.d_dlr + L.dlr_pad;
  L.k = L.d_dlr + in.d_cls; L.k_rm = (int)round_up(L.k, TILE_K);
  L.n_tiles = (in.n_rows + TILE_ROWS - 1) / TILE_ROWS;
  if (L.has_idx) {
    L.n_buckets = in.idx_buckets == 1 ? 1 : 2;
    L.ts = even_up((L.d_dlr + 31) / 32);
    L.dense_i8 = in.d_cls > 0 && in.want_dense_i8 != 0;
    int want_g8 = in.want_gated_i8;
    if (want_g8 < 0) want_g8 = in.n_rows >= (2 * in.d_cls >= L.d_dlr ? GATED_I8_MIN_ROWS : GATED_I8_MIN_ROWS_NARROW) ? 1 : 0;
    L.gated_i8 = want_g8 != 0 && L.n_buckets == 2 && (in.d_cls == 0 || L.dense_i8) && L.d_dlr <= 4096;
  } else {
    L.dense_only_trial = in.want_dense_i8 < 0 && in.n_rows >= DENSE_ONLY_I8_MIN_ROWS && in.d_cls >= 128;
    L.dense_i8 = in.want_dense_i8 > 0 || L.dense_only_trial;
  }
  L.td = dense_stages(in.d_cls, L.dense_i8);
  L.kt = L.ts * TILE_K + L.td * 32; L.ksteps = (L.kt + TILE_K - 1) / TILE_K;
  return L;
}
// The layout of a REJECTED dense-only trial: by definition make_layout of the same input with the ungated int8 image off
inline IndexLayout fp16_fallback(const IndexLayout& L) { LayoutInput off = L.in; off.want_dense_i8 = 0; return make_layout(off); }
// The verdict of the trial from the measured row error ec and row norm nc of the int8 image (a NaN rejects).  The filter margin of the image is ~ ||q|| ec while the scores of a dense-only index
// spread by ~ ||q|| ||d|| / sqrt(d_cls), and the candidates grow exponentially with the ratio of the two: at 0.36 the int8 search is still the faster one, much coarser keeps fp16.
inline bool trial_keeps_i8(int d_cls, float ec, float nc) { return std::sqrt((float)d_cls) * ec / std::max(nc, 1e-30f) <= 0.45f; }
// ---- the column-step rule of the two int8 images
// A column's step relative to the largest column's, from ratio = (its largest |value|) / (the largest of all): ratio^(3/4).  The exponent splits a column's dynamic range between the
// corpus image (finer steps for small columns) and the query weights (which then stay within ~two orders of magnitude) -- measured on anisotropic columns the margin is 1.8x smaller
// than with exponent 1 and 4-6x smaller than with one step for all columns; on iid columns all exponents are equal (tests/test_i8_bound.py)
inline float column_step_factor(float ratio) { return std::max(std::pow(ratio, 0.75f), 1.f / 1024.f); }
// Ungated columns (colmax_bits: what col_absmax_kernel leaves): column j is quantised in its own step cs_j <= scale, the query side carries cs_j / scale as a weight (query_prep_kernel)
// -- a few large columns (outlier dimensions of encoder outputs) then do not push every other column into a handful of int8 levels
inline std::vector<float> ungated_steps(const std::vector<uint32_t>& colmax_bits, float i8_scale) {
  std::vector<float> cs(colmax_bits.size());
  for (size_t j = 0; j < cs.size(); ++j) {
    const float m = bits_to_float(colmax_bits[j]);
    cs[j] = i8_scale * column_step_factor(m > 0.f ? std::min(m / (127.f * i8_scale), 1.f) : 1.f);
  }
  return cs;
}
// Gated columns: s_ref = (largest gated |value|) / 127, column j in s_ref * factor_j; inv_cs_j = 1 / step_j and w_j = step_j / s_ref, both with 1e-6 of head room
// (m / (s_ref f) = 127 ratio^(1/4) / 1.00001 <= 127)
struct GatedSteps { float sref = 0.f; std::vector<float> inv_cs, w; };
inline GatedSteps gated_steps(const std::vector<uint32_t>& colmax_bits, float gmax) {
  GatedSteps g;
  g.sref = (gmax > 0.f ? gmax : 1.f) * (1.00001f / 127.f); g.inv_cs.reserve(colmax_bits.size()); g.w.reserve(colmax_bits.size());
  for (const uint32_t bits : colmax_bits) {
    const float m = bits_to_float(bits);
    const float f = column_step_factor(m > 0.f ? std::min(m / gmax, 1.f) : 1.f);
    g.inv_cs.push_back(1.000001f / (g.sref * f));
    g.w.push_back(f * 1.000001f);
  }
  return g;
}
// Per-slice index-value -> bucket table, balanced by value MASS (greedy: heaviest value first into the lightest bucket;
// values that never occur with a non-zero entry are dealt round-robin).
inline void build_bucket_map(const std::vector<float>& hist, int d_dlr, int nb, std::vector<uint8_t>& map) {
  map.assign((size_t)d_dlr * 256, 0);
  std::vector<int> order(256);
  std::vector<double> load(nb);
  for (int j = 0; j < d_dlr; ++j) {
    const float* h = &hist[(size_t)j * 256];
    for (int v = 0; v < 256; ++v) order[v] = v;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h[a] > h[b]; });
    std::fill(load.begin(), load.end(), 0);
    int rr = 0;
    for (int v : order) {
      int best = 0;
      if (h[v] == 0) best = rr++ % nb;                   // unseen values: round robin
      else
        for (int b = 1; b < nb; ++b)
          if (load[b] < load[best]) best = b;
      map[(size_t)j * 256 + v] = (uint8_t)best;
      load[best] += h[v];
    }
  }
}
}  // namespace layout
}  // namespace dhr

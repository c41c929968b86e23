// Index handles of libdhr_hip.so (round 6: split out of api.hip): build (dhr_index_create), parameters and info, the index file.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "dhr_state.h"
#include "index_layout.h"
static_assert(layout::TILE_ROWS == TILE_ROWS && layout::TILE_K == TILE_K && layout::SP_STAGE_A == SP_STAGE_A && layout::S8_STAGE_A == S8_STAGE_A && layout::SP_DENSE == SP_DENSE && layout::HEAVY_KEY_STRIDE == HEAVY_KEY_STRIDE, "index_layout.h restates the tile geometry of dhr_internal.h");

extern "C" void dhr_index_destroy(dhr_index* ix) try {
  if (!ix) return;
  hipSetDevice(ix->device);
  free_ws(ix->ws);
  free_ws(ix->ws_fb[0]);
  free_ws(ix->ws_fb[1]);
  if (ix->s_aux) hipStreamDestroy(ix->s_aux);
  if (ix->s_gemm) hipStreamDestroy(ix->s_gemm);
  hipFree(ix->sh_arena);
  hipFree(ix->resid8); hipFree(ix->i8_col_scale); hipFree(ix->g8_inv_cs); hipFree(ix->g8_w); hipFree(ix->g8_rsum); hipFree(ix->tiles); hipFree(ix->c_idx); hipFree(ix->vals_rm); hipFree(ix->bucket_map); hipFree(ix->heavy_key);      // (heavy_val points into the heavy_key records)
  delete ix;
} DHR_CATCH_VOID

static int g_opt_dense_i8 = -1;      // -1: gated indexes with ungated columns only; 0: never; 1: dense-only indexes too
static int g_opt_gated_i8 = -1;      // int8 image of the gated half: -1 by corpus size (>= GATED_I8_MIN_ROWS rows; _NARROW where the ungated half is narrower than half the gated one), 0 never, 1 wherever the layout allows it
extern "C" int dhr_set_option(int32_t option, int64_t value) try {
  if (option == DHR_OPT_DENSE_I8) { g_opt_dense_i8 = value < 0 ? -1 : (value != 0); return DHR_OK; }
  if (option == DHR_OPT_GATED_I8) { g_opt_gated_i8 = value < 0 ? -1 : (value != 0); return DHR_OK; }
  return set_error(DHR_ERR_INVALID, "unknown option");
} DHR_CATCH_STATUS
extern "C" int dhr_index_get_info(const dhr_index* ix, int32_t what, double* out) try {
  if (!ix || !out) return set_error(DHR_ERR_INVALID, "null argument");
  switch (what) {
    case DHR_INFO_DENSE_I8: *out = ix->dense_i8 ? 1.0 : 0.0; return DHR_OK;
    case DHR_INFO_I8_SCALE: *out = ix->i8_scale; return DHR_OK;
    case DHR_INFO_I8_ROW_ERR: *out = ix->i8_ec; return DHR_OK;
    case DHR_INFO_I8_ROW_NORM: *out = ix->i8_nc; return DHR_OK;
    case DHR_INFO_ROW_NORM_MAX: *out = ix->dmax; return DHR_OK;
    case DHR_INFO_GATED_I8: *out = ix->gated_i8 ? 1.0 : 0.0; return DHR_OK;
    case DHR_INFO_GEMM_KERNEL: *out = (double)ix->last_gemm_kernel; return DHR_OK;
    case DHR_INFO_TILE_BYTES: *out = (double)layout::tile_bytes(ix->n_tiles, ix->ts, ix->td, ix->gated_i8); return DHR_OK;
  }
  return set_error(DHR_ERR_INVALID, "unknown info id");
} DHR_CATCH_STATUS

extern "C" int dhr_index_set_param(dhr_index* ix, int32_t param, int64_t value) try {
  if (!ix) return set_error(DHR_ERR_INVALID, "null index");
  switch (param) {
    case DHR_PARAM_CAND_CAP:
      if (value < DOC_GROUP * TILE_ROWS || value > (1 << 22)) return set_error(DHR_ERR_INVALID, "cand_cap must be in [1024, 4194304]");      // (>= the rows of a minimum chunk, as list_stride below)
      ix->cand_cap = value; return DHR_OK;
    case DHR_PARAM_FIRST_ROWS:
      if (value < 0) return set_error(DHR_ERR_INVALID, "first_rows must be >= 0");
      ix->first_rows = value; return DHR_OK;
    case DHR_PARAM_PROFILE: ix->profile = value != 0; return DHR_OK;
    case DHR_PARAM_SAMPLE_PERIOD:
      if (value < 0 || value > 256) return set_error(DHR_ERR_INVALID, "sample_period must be in [0,256] (0/1 = off)");
      ix->sample_period = (int)value; return DHR_OK;
    case DHR_PARAM_ASYNC_CONTROLLER: ix->async_ctl = value < 0 ? 0 : (value > 2 ? 2 : (int)value); return DHR_OK;
    case DHR_PARAM_LIST_STRIDE:
      // (>= the rows of the smallest chunk the host-driven controller can fall back to, DOC_GROUP tiles: a list that cannot hold every row of it could
      // overflow with nothing left to halve -- until round 6 the range began at 256, and such a chunk lost its entries beyond the stride SILENTLY
      // on corpora too small for the sampled controller; found by tools/stress_modes.py)
      if (value != 0 && (value < DOC_GROUP * TILE_ROWS || value > (1 << 22) || value % 256))
        return set_error(DHR_ERR_INVALID, "list_stride must be 0 (default) or a multiple of 256 in [1024, 4194304]");
      ix->list_stride = value; return DHR_OK;
    case DHR_PARAM_SAMPLE_SHARE:
      if (value < 1 || value > 4096) return set_error(DHR_ERR_INVALID, "sample_share must be in [1,4096]");
      ix->sample_share = (int)value; return DHR_OK;
    case DHR_PARAM_MAIN_CHUNKS:
      if (value < 1 || value > 64) return set_error(DHR_ERR_INVALID, "main_chunks must be in [1,64]");
      ix->main_chunks = (int)value; return DHR_OK;
    case DHR_PARAM_PROGRESSIVE_THR: ix->progressive_thr = value < 0 ? 0 : (value > 2 ? 2 : (int)value); return DHR_OK;
    case DHR_PARAM_AUX_CUS:
      if (value < 0 || value > 192 || value % 8) return set_error(DHR_ERR_INVALID, "aux_cus must be a multiple of 8 in [0,192]");
      ix->aux_cus = (int)value; return DHR_OK;
    case DHR_PARAM_GEMM_EXCLUSIVE: ix->gemm_exclusive = value != 0; return DHR_OK;
    case DHR_PARAM_OVERLAP_AUX: ix->overlap_aux = value < 0 ? -1 : value != 0; return DHR_OK;
    case DHR_PARAM_SEAT_QUERIES: ix->seat_queries = value < 0 ? -1 : 0; return DHR_OK;      // (-1 = on where it applies, 0 = off: there is no "forced on")
    case DHR_PARAM_GEMM_VARIANT:
#ifdef DHR_AB_VARIANTS
      if (value == 6) { ix->gemm_variant = 6; return DHR_OK; }      // A/B builds: persistent workgroups on gated_i8 indexes (tools/ab/gemm_g8p.hip)
#endif
      if (value != 4 && value != 5) return set_error(DHR_ERR_INVALID, "gemm_variant: 4 (4 waves, 128 x 128 wave tiles) or 5 (8 waves, 128 x 64 wave tiles; default) -- the fp16-gated kernel; integer (gated_i8) indexes have one kernel");
      ix->gemm_variant = (int)value; return DHR_OK;
    case DHR_PARAM_MAX_GROWTH:
      if (value < 1 || value > 1024) return set_error(DHR_ERR_INVALID, "max_growth must be in [1,1024] sixteenths");
      ix->max_growth16 = (int)value; return DHR_OK;
  }
  return set_error(DHR_ERR_INVALID, "unknown parameter");
} DHR_CATCH_STATUS

extern "C" int dhr_index_device(const dhr_index* ix) try { return ix ? ix->device : -1; } DHR_CATCH_VALUE(-1)
extern "C" void dhr_internal_index_arena(dhr_index* ix, void*** base, size_t** bytes) try { *base = &ix->sh_arena; *bytes = &ix->sh_arena_bytes; } DHR_CATCH_VOID
extern "C" int64_t dhr_index_device_bytes(const dhr_index* ix) try { return ix ? ix->index_bytes + ix->ws.bytes + ix->ws_fb[0].bytes + ix->ws_fb[1].bytes + (int64_t)ix->sh_arena_bytes : 0; } DHR_CATCH_VALUE(0)
extern "C" int dhr_get_stats(const dhr_index* ix, dhr_search_stats* out) try {
  if (!ix || !out) return set_error(DHR_ERR_INVALID, "null argument");
  *out = ix->stats;
  return DHR_OK;
} DHR_CATCH_STATUS

// ------------------------------------------------------------------------------------------ index build
// Pass 1 of the index build: the caller's rows (host rows staged block by block) -> row-major device copy vals_rm, norms and
// sign scan.  Everything else (bucket maps, operand tiles, refine lists) is derived from vals_rm / c_idx on the device.
static int ingest(dhr_index* ix, const dhr_index_desc* d, uint32_t* d_flags /* {max_sq, neg} */, void* stage, int64_t block_rows,
                  hipStream_t s) {
  const int64_t n = ix->n_rows;
  for (int64_t lo = 0; lo < n; lo += block_rows) {
    const int64_t rows = std::min(block_rows, n - lo);
    const __half* src;
    int64_t ld;
    if (ix->dlr_pad > 0) {        // [gated | ungated] of the caller -> [gated | zero slices | ungated] (the staging buffer was zeroed once)
      const hipMemcpyKind kind = d->mem_kind == DHR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
      const int d_in = ix->d_dlr - ix->dlr_pad;
      const char* base = (const char*)d->value + lo * d->ld_value * 2;
      HIP_TRY(hipMemcpy2DAsync(stage, (size_t)ix->k * 2, base, (size_t)d->ld_value * 2, (size_t)d_in * 2, (size_t)rows, kind, s));
      if (ix->d_cls > 0)
        HIP_TRY(hipMemcpy2DAsync((char*)stage + (size_t)ix->d_dlr * 2, (size_t)ix->k * 2, base + (size_t)d_in * 2, (size_t)d->ld_value * 2,
                                 (size_t)ix->d_cls * 2, (size_t)rows, kind, s));
      src = (const __half*)stage;
      ld = ix->k;
    } else if (d->mem_kind == DHR_MEM_HOST) {
      HIP_TRY(hipMemcpy2DAsync(stage, (size_t)ix->k * 2, (const char*)d->value + lo * d->ld_value * 2,
                               (size_t)d->ld_value * 2, (size_t)ix->k * 2, (size_t)rows, hipMemcpyHostToDevice, s));
      src = (const __half*)stage;
      ld = ix->k;
    } else {
      src = (const __half*)d->value + lo * d->ld_value;
      ld = d->ld_value;
    }
    HIP_TRY(launch_scan_rows(src, ld, rows, ix->d_dlr, ix->k, d_flags, d_flags + 1, s));
    HIP_TRY(launch_copy_rows(src, ld, rows, ix->k, ix->k_rm, ix->vals_rm + lo * ix->k_rm, s));
    if (d->mem_kind == DHR_MEM_HOST || ix->dlr_pad > 0) HIP_TRY(hipStreamSynchronize(s));   // the staging buffer is reused
  }
  return DHR_OK;
}
// Pass 2: the bound-GEMM operand tiles from the device copy (needs the bucket map and abs_mode).
static int build_tiles(dhr_index* ix, hipStream_t s) {
  const int64_t n = ix->n_rows, fill = ix->n_tiles * TILE_ROWS;
  // stage images: 2:4 sparse stages of 32 gated slices, then stages of 32 (fp16) / 64 (int8) ungated columns
  HIP_TRY(launch_tile_rows_sparse(ix->vals_rm, ix->k_rm, 0, n, fill, ix->d_dlr, ix->d_cls, ix->ts, ix->td, ix->c_idx, ix->idx_dtype,
                                  ix->bucket_map, ix->abs_mode, (char*)ix->tiles, ix->dense_i8 ? 1.f / ix->i8_scale : 0.f, ix->i8_col_scale,
                                  ix->gated_i8 ? ix->g8_inv_cs : nullptr, s));
  return DHR_OK;
}

// What a build holds until it reaches its end: every early return and every exception releases the scratch and the half-built handle
struct Build {
  dhr_index* ix = nullptr; layout::IndexLayout L; hipStream_t s = nullptr; const dhr_index_desc* d = nullptr;      // d: the CALLER's descriptor and widths: only the step that reads the caller's arrays (step_ingest) uses it
  void* stage = nullptr; uint32_t* d_flags = nullptr;
  uint32_t flags[4] = {0, 0, 0, 0};       // what scan_rows_kernel left, as bit patterns: max ||d||^2, any negative gated value, largest ungated / gated |value|
  ~Build() { (void)hipFree(stage); (void)hipFree(d_flags); if (ix) dhr_index_destroy(ix); }
};
#define STEP(call) do { const int _rc = (call); if (_rc != DHR_OK) return _rc; } while (0)
using layout::bits_to_float;
// One device array of a build; the `counted` ones are the index that dhr_index_device_bytes reports
template <class T> static int dev_array(dhr_index* ix, T** p, size_t bytes, bool counted, const char* what) {
  if (hipMalloc((void**)p, bytes) != hipSuccess) return set_error(DHR_ERR_HIP, "hipMalloc of " + std::to_string(bytes) + " bytes for " + what + " failed");
  ix->index_bytes += counted ? (int64_t)bytes : 0;
  return DHR_OK;
}
// Largest finite |value| of columns [first, first + n) of the device copy (bit patterns: layout::ungated_steps / gated_steps read them)
static int scan_col_max(const Build& b, int first, int n, std::vector<uint32_t>& cm) {
  DevMem d_cm;
  cm.assign((size_t)n, 0u);
  HIP_TRY(hipMalloc(&d_cm.p, cm.size() * 4));
  HIP_TRY(hipMemsetAsync(d_cm.p, 0, cm.size() * 4, b.s));
  HIP_TRY(launch_col_absmax(b.ix->vals_rm, b.ix->k_rm, b.ix->n_rows, first, n, (uint32_t*)d_cm.p, b.s));
  HIP_TRY(hipMemcpy(cm.data(), d_cm.p, cm.size() * 4, hipMemcpyDeviceToHost));
  return DHR_OK;
}
static void apply_layout(dhr_index* ix, const layout::IndexLayout& L) {
  ix->n_rows = L.in.n_rows; ix->n_tiles = L.n_tiles; ix->d_dlr = L.d_dlr; ix->d_cls = L.in.d_cls; ix->dlr_pad = L.dlr_pad; ix->k = L.k; ix->k_rm = L.k_rm;
  ix->idx_dtype = L.has_idx ? L.in.idx_dtype : DHR_IDX_NONE; ix->n_buckets = L.n_buckets;
  ix->ts = L.ts; ix->td = L.td; ix->kt = L.kt; ix->ksteps = L.ksteps; ix->dense_i8 = L.dense_i8; ix->gated_i8 = L.gated_i8;
}
// corpus copies: the index array as it is (zero slices appended), the values through pass 1 -- row-major device copy, norms and sign scan
static int step_ingest(Build& b) {
  dhr_index* ix = b.ix; const dhr_index_desc* d = b.d;
  STEP(dev_array(ix, &ix->vals_rm, (size_t)ix->n_rows * ix->k_rm * 2, true, "the row-major corpus copy"));
  STEP(dev_array(ix, &b.d_flags, 16, false, "the scan results"));
  HIP_TRY(hipMemsetAsync(b.d_flags, 0, 16, b.s));
  if (b.L.has_idx) {
    const size_t es = idx_esize(ix->idx_dtype), ib = (size_t)ix->n_rows * ix->d_dlr * es;
    STEP(dev_array(ix, &ix->c_idx, ib, true, "the index array"));
    if (ix->dlr_pad) HIP_TRY(hipMemsetAsync(ix->c_idx, 0, ib, b.s));
    HIP_TRY(hipMemcpy2DAsync(ix->c_idx, ix->d_dlr * es, d->index, d->ld_index * es, d->d_dlr * es, (size_t)ix->n_rows,
                             d->mem_kind == DHR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, b.s));
  }
  const int64_t block_rows = 65536, stage_bytes = std::min<int64_t>(block_rows, ix->n_rows) * ix->k * 2;
  if (d->mem_kind == DHR_MEM_HOST || ix->dlr_pad > 0) STEP(dev_array(ix, &b.stage, stage_bytes, false, "the staging buffer"));
  if (ix->dlr_pad > 0) HIP_TRY(hipMemsetAsync(b.stage, 0, stage_bytes, b.s));
  return ingest(ix, d, b.d_flags, b.stage, block_rows, b.s);
}
static int step_scan_results(Build& b) {
  HIP_TRY(hipMemcpy(b.flags, b.d_flags, 16, hipMemcpyDeviceToHost));
  b.ix->dmax = std::sqrt(bits_to_float(b.flags[0])) * 1.0005f + 1e-30f;
  b.ix->abs_mode = b.flags[1] != 0;     // negative gated values: the bound needs |q|.|d| on the gated half
  return DHR_OK;
}
// int8 image of the ungated columns: scale and column steps, the corpus-wide maxima of the row error and norm that the filter margin pays for, and -- a dense-only
// index on trial -- the verdict: a rejected trial continues as the fp16 layout
static int step_ungated_i8(Build& b) {
  dhr_index* ix = b.ix; if (!ix->dense_i8) return DHR_OK;
  const float amax = bits_to_float(b.flags[2]), gmax = bits_to_float(b.flags[3]);
  ix->i8_scale = std::max(amax > 0.f ? amax / 127.f : 1.f, gmax / 60000.f);      // gated values must fit fp16 in units of the scale
  std::vector<uint32_t> cm;
  STEP(scan_col_max(b, ix->d_dlr, ix->d_cls, cm));
  const std::vector<float> cs = layout::ungated_steps(cm, ix->i8_scale);
  STEP(dev_array(ix, &ix->i8_col_scale, cs.size() * 4, false, "the ungated column steps"));
  HIP_TRY(hipMemcpy(ix->i8_col_scale, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(b.d_flags, 0, 16, b.s));
  HIP_TRY(launch_i8_row_err(ix->vals_rm, ix->k_rm, ix->n_rows, ix->d_dlr, ix->d_cls, ix->i8_scale, ix->i8_col_scale, b.d_flags, b.s));
  uint32_t err[2] = {0, 0};
  HIP_TRY(hipMemcpy(err, b.d_flags, 8, hipMemcpyDeviceToHost));
  ix->i8_ec = std::sqrt(bits_to_float(err[0])) * 1.001f; ix->i8_nc = std::sqrt(bits_to_float(err[1])) * 1.001f;
  if (b.L.dense_only_trial && !layout::trial_keeps_i8(ix->d_cls, ix->i8_ec, ix->i8_nc)) {
    hipFree(ix->i8_col_scale); ix->i8_col_scale = nullptr; ix->i8_scale = ix->i8_ec = ix->i8_nc = 0.f;
    apply_layout(ix, b.L = layout::fp16_fallback(b.L));
  }
  return DHR_OK;
}
// Dense-only int8 index: residual image = the refine level between the filter and the exact rescoring.  The int8 margin is  ||q'|| ec (corpus rounding) + ||q' - q8'|| nc (query rounding); with the residuals the
// first term is MEASURED per candidate from 384 bytes (four bits per value) instead of bounded, and the candidates that only the corpus half of the margin let through never reach the 1.5 KB rows of the exact rescoring.
static int step_residual(Build& b) {
  dhr_index* ix = b.ix; if (!b.L.has_residual(ix->i8_ec)) return DHR_OK;
  ix->resid_ld = b.L.resid_ld();
  STEP(dev_array(ix, &ix->resid8, (size_t)ix->n_rows * ix->resid_ld, true, "the residual image"));
  ix->resid_ec2 = std::sqrt((float)ix->d_cls) * ix->i8_scale / 28.f;       // every residual is within half of 1/14 of its column's step: scale / 28 in the weighted space
  HIP_TRY(launch_resid_build(ix->vals_rm, ix->k_rm, ix->n_rows, ix->d_dlr, ix->d_cls, ix->i8_col_scale, ix->resid8, ix->resid_ld, b.s));
  return DHR_OK;
}
static int step_alloc_tiles(Build& b) { return dev_array(b.ix, &b.ix->tiles, b.L.tile_bytes(), true, "the corpus tiles"); }
// int8 image of the gated columns: their steps (layout::gated_steps), the shift range and the row sums that the integer GEMM starts from
static int step_gated_i8(Build& b) {
  dhr_index* ix = b.ix; if (!ix->gated_i8) return DHR_OK;
  std::vector<uint32_t> cm;
  STEP(scan_col_max(b, 0, ix->d_dlr, cm));
  const layout::GatedSteps g = layout::gated_steps(cm, bits_to_float(b.flags[3]));
  ix->g8_sref = g.sref; ix->g8_max_shift = b.L.g8_max_shift();
  STEP(dev_array(ix, &ix->g8_inv_cs, cm.size() * 4, false, "the gated column steps"));
  STEP(dev_array(ix, &ix->g8_w, cm.size() * 4, false, "the gated column weights"));
  HIP_TRY(hipMemcpy(ix->g8_inv_cs, g.inv_cs.data(), cm.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ix->g8_w, g.w.data(), cm.size() * 4, hipMemcpyHostToDevice));
  STEP(dev_array(ix, &ix->g8_rsum, (size_t)ix->n_tiles * TILE_ROWS * 4, true, "the gated row sums"));
  HIP_TRY(launch_g8_row_sum(ix->vals_rm, ix->k_rm, ix->n_rows, ix->n_tiles * TILE_ROWS, ix->d_dlr, ix->abs_mode, ix->g8_inv_cs, ix->g8_rsum, b.s));
  return DHR_OK;
}
// bucket maps: all-zero for idx_buckets = 1 (it serves 8- and 16-bit index dtypes alike: bucket_of reads map[j][value & 255]); two buckets of 8-bit index values are dealt by
// the value mass per (slice, index value) (layout::build_bucket_map); 16-bit ones have no map (value % 2)
static int step_bucket_maps(Build& b) {
  dhr_index* ix = b.ix;
  const size_t mb = (size_t)ix->d_dlr * 256;
  std::vector<uint8_t> map;
  if (!b.L.has_idx || (ix->n_buckets > 1 && idx_esize(ix->idx_dtype) != 1)) return DHR_OK;
  if (ix->n_buckets > 1) {
    DevMem d_hist;
    std::vector<float> hist(mb);
    HIP_TRY(hipMalloc(&d_hist.p, mb * 4));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, mb * 4, b.s));
    HIP_TRY(launch_idx_hist((const uint8_t*)ix->c_idx, ix->vals_rm, ix->k_rm, ix->n_rows, ix->d_dlr, (float*)d_hist.p, b.s));
    HIP_TRY(hipMemcpy(hist.data(), d_hist.p, mb * 4, hipMemcpyDeviceToHost));
    layout::build_bucket_map(hist, ix->d_dlr, ix->n_buckets, map);
  } else map.assign(mb, 0);
  STEP(dev_array(ix, &ix->bucket_map, mb, false, "the bucket map"));
  HIP_TRY(hipMemcpy(ix->bucket_map, map.data(), mb, hipMemcpyHostToDevice));
  return DHR_OK;
}
static int step_refine_lists(Build& b) {
  dhr_index* ix = b.ix; if (!b.L.refine_lists()) return DHR_OK;
  STEP(dev_array(ix, &ix->heavy_key, (size_t)ix->n_rows * HEAVY_KEY_STRIDE * 4, true, "the refine lists"));      // one 6 x HEAVY-byte record per row (layout: dhr_internal.h)
  ix->heavy_val = (__half*)ix->heavy_key;
  HIP_TRY(launch_heavy_build(ix->vals_rm, ix->k_rm, ix->c_idx, ix->idx_dtype, ix->n_rows, ix->d_dlr, ix->bucket_map, ix->n_buckets, ix->heavy_key, ix->heavy_val,
                             ix->gated_i8 ? ix->g8_inv_cs : nullptr, ix->abs_mode ? 1 : 0, b.s));
  return DHR_OK;
}
// The rules of a descriptor, each checked once, in the order in which a descriptor that breaks two of them reports the first (no device is touched)
static int check_desc(const dhr_index_desc* d, dhr_index** out) {
  if (!d || !out) return set_error(DHR_ERR_INVALID, "null argument");
  if (d->ld_value < (int64_t)d->d_dlr + d->d_cls) return set_error(DHR_ERR_INVALID, "bad value pointer / ld_value");
  const bool has_idx = d->index != nullptr && d->index_dtype != DHR_IDX_NONE;
  if (has_idx && d->ld_index < d->d_dlr) return set_error(DHR_ERR_INVALID, "bad ld_index");
  *out = nullptr;
  if (d->n_rows <= 0 || d->n_rows >= (int64_t)0xFFFFFF00ll) return set_error(DHR_ERR_INVALID, "n_rows must be in [1, 2^32-256)");
  if (d->d_dlr < 0 || d->d_cls < 0 || d->d_dlr + d->d_cls <= 0) return set_error(DHR_ERR_INVALID, "bad d_dlr/d_cls");
  if (!d->value) return set_error(DHR_ERR_INVALID, "bad value pointer / ld_value");
  if (has_idx != (d->d_dlr > 0)) return set_error(DHR_ERR_INVALID, "an index array is required iff d_dlr > 0 (dense-only: index=NULL, d_dlr=0)");
  if (has_idx && (d->index_dtype < DHR_IDX_U8 || d->index_dtype > DHR_IDX_I16)) return set_error(DHR_ERR_INVALID, "bad index_dtype");
  if (d->d_dlr + layout::dlr_pad_of(d->d_dlr, d->index != nullptr) + d->d_cls > 8192) return set_error(DHR_ERR_UNSUPPORTED, "more than 8192 columns");      // (the padded width)
  if (d->idx_buckets < 0 || d->idx_buckets > 2) return set_error(d->idx_buckets > 2 ? DHR_ERR_UNSUPPORTED : DHR_ERR_INVALID, "idx_buckets must be 0 (default: 2), 1 (ungated bound) or 2: the bucket-split operands of more than two buckets went with the K-step tile layout (round 6)");
  if (d->mem_kind != DHR_MEM_HOST && d->mem_kind != DHR_MEM_DEVICE) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  return DHR_OK;
}
// The two image options as -1 / 0 / 1: the process option (dhr_set_option), which the environment variable beats (DHR_DENSE_I8: default gated indexes only; DHR_GATED_I8=0 keeps the fp16 gated image)
static void resolve_options(layout::LayoutInput& in) {
  auto resolve = [](int v, const char* env) { if (const char* e = getenv(env)) v = atoi(e); return v < 0 ? -1 : (v != 0); };
  in.want_dense_i8 = resolve(g_opt_dense_i8, "DHR_DENSE_I8"); in.want_gated_i8 = resolve(g_opt_gated_i8, "DHR_GATED_I8");
}
extern "C" int dhr_index_create(const dhr_index_desc* d, dhr_index** out) try {
  STEP(check_desc(d, out));
  layout::LayoutInput in; resolve_options(in);
  in.n_rows = d->n_rows; in.d_dlr = d->d_dlr; in.d_cls = d->d_cls; in.index_array = d->index != nullptr; in.idx_dtype = d->index_dtype; in.idx_buckets = d->idx_buckets;
  dhr::alloc_checkpoint();
  HIP_TRY(hipSetDevice(d->device));
  Build b; b.d = d; b.L = layout::make_layout(in);
  dhr_index* ix = b.ix = new dhr_index();
  ix->device = d->device; ix->idx_buckets_req = d->idx_buckets; ix->row_offset = d->row_offset;
  { hipDeviceProp_t pr; HIP_TRY(hipGetDeviceProperties(&pr, d->device)); ix->n_cu = pr.multiProcessorCount; }
  apply_layout(ix, b.L);
  STEP(step_ingest(b));
  STEP(step_scan_results(b));
  STEP(step_ungated_i8(b));
  STEP(step_residual(b));
  STEP(step_alloc_tiles(b));
  STEP(step_gated_i8(b));
  STEP(step_bucket_maps(b));
  STEP(build_tiles(ix, b.s));        // pass 2: operand tiles (needs the bucket map and abs_mode)
  STEP(step_refine_lists(b));
  if (hipStreamSynchronize(b.s) != hipSuccess) return set_error(DHR_ERR_HIP, "index build failed on the device");
  b.ix = nullptr; *out = ix;          // the caller's from here on
  return DHR_OK;
} DHR_CATCH_STATUS

// ------------------------------------------------------------------------------------------ index file
// [4096-byte header][values: n_rows x k_rm fp16][slice indices: n_rows x d_dlr][caller blob], sections page-aligned.
// The file holds the corpus in the reference's own record layout (row-major fp16 values, row-major indices), NOT
// the device images: measured, re-tiling from device memory costs 0.06 s per 2 M rows while the images would
// double the file (15 vs 7.7 GB per 2 M rows) -- reading the extra bytes is slower than recomputing them.
// What the file removes is the monolithic pickle: no unpickling, no host copies, no fp32 cast; the mapping
// is streamed to the device block by block by the ordinary ingest path.
namespace {
struct FileHeader {
  char magic[8];
  uint32_t version, header_bytes;
  int64_t n_rows, row_offset;
  int32_t d_dlr, d_cls, k_rm, idx_dtype, idx_buckets, pad0;
  uint64_t val_offset, val_bytes, idx_offset, idx_bytes, blob_offset, blob_bytes;
};
static_assert(sizeof(FileHeader) <= 4096, "header must fit one page");
const char FILE_MAGIC[8] = {'D', 'H', 'R', 'I', 'D', 'X', '1', 0};
constexpr uint32_t FILE_VERSION = 1;

bool write_all(int fd, const void* p, size_t n) {
  const char* c = (const char*)p;
  while (n) {
    const ssize_t w = write(fd, c, n);
    if (w <= 0) return false;
    c += w; n -= (size_t)w;
  }
  return true;
}
int read_header(const char* path, FileHeader& h, int* fd_out) {
  if (!path) return set_error(DHR_ERR_INVALID, "null path");
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return set_error(DHR_ERR_INVALID, std::string("cannot open ") + path);
  char page[4096];
  const ssize_t got = pread(fd, page, sizeof(page), 0);
  if (got != (ssize_t)sizeof(page)) { close(fd); return set_error(DHR_ERR_INVALID, std::string(path) + " is not a device-ready index file (short header)"); }
  memcpy(&h, page, sizeof(h));
  if (memcmp(h.magic, FILE_MAGIC, 8) != 0 || h.header_bytes != 4096) { close(fd); return set_error(DHR_ERR_INVALID, std::string(path) + " is not a device-ready index file"); }
  if (h.version != FILE_VERSION) {
    close(fd);
    return set_error(DHR_ERR_UNSUPPORTED, std::string(path) + " has file format version " + std::to_string(h.version) + ", this library reads version " +
                                          std::to_string(FILE_VERSION));
  }
  if (fd_out) *fd_out = fd; else close(fd);
  return DHR_OK;
}
}  // namespace

extern "C" int dhr_index_save(const dhr_index* ix, const char* path, const void* blob, int64_t blob_bytes) try {
  if (!ix || !path || blob_bytes < 0 || (blob_bytes > 0 && !blob)) return set_error(DHR_ERR_INVALID, "null index / path or bad blob");
  HIP_TRY(hipSetDevice(ix->device));
  FileHeader h{};
  memcpy(h.magic, FILE_MAGIC, 8);
  h.version = FILE_VERSION; h.header_bytes = 4096;
  h.n_rows = ix->n_rows; h.row_offset = ix->row_offset;
  h.d_dlr = ix->d_dlr; h.d_cls = ix->d_cls; h.k_rm = ix->k_rm; h.idx_dtype = ix->idx_dtype; h.idx_buckets = ix->idx_buckets_req;
  h.pad0 = ix->dlr_pad;            // the file holds the padded records; a loaded index takes the caller's unpadded queries again
  h.val_offset = 4096; h.val_bytes = (uint64_t)ix->n_rows * ix->k_rm * 2;
  h.idx_offset = (h.val_offset + h.val_bytes + 4095) / 4096 * 4096;
  h.idx_bytes = ix->c_idx ? (uint64_t)ix->n_rows * ix->d_dlr * idx_esize(ix->idx_dtype) : 0;
  h.blob_offset = (h.idx_offset + h.idx_bytes + 4095) / 4096 * 4096;
  h.blob_bytes = (uint64_t)blob_bytes;
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return set_error(DHR_ERR_INVALID, std::string("cannot create ") + path);
  const size_t CH = (size_t)64 << 20;
  void* pin = nullptr;
  if (hipHostMalloc(&pin, CH, hipHostMallocDefault) != hipSuccess) { close(fd); return set_error(DHR_ERR_HIP, "hipHostMalloc failed"); }
  auto fail = [&](int code) { hipHostFree(pin); close(fd); unlink(path); return code; };
  char page[4096] = {0};
  memcpy(page, &h, sizeof(h));
  if (!write_all(fd, page, 4096)) return fail(set_error(DHR_ERR_INVALID, "write failed (header)"));
  const void* src[2] = {ix->vals_rm, ix->c_idx};
  const uint64_t off[2] = {h.val_offset, h.idx_offset}, bytes[2] = {h.val_bytes, h.idx_bytes};
  for (int i = 0; i < 2; ++i) {
    if (lseek(fd, (off_t)off[i], SEEK_SET) < 0) return fail(set_error(DHR_ERR_INVALID, "seek failed"));
    for (uint64_t done = 0; done < bytes[i]; done += CH) {
      const size_t n = (size_t)std::min<uint64_t>(CH, bytes[i] - done);
      if (hipMemcpy(pin, (const char*)src[i] + done, n, hipMemcpyDeviceToHost) != hipSuccess) return fail(set_error(DHR_ERR_HIP, "D2H copy failed while saving"));
      if (!write_all(fd, pin, n)) return fail(set_error(DHR_ERR_INVALID, "write failed (disk full?)"));
    }
  }
  if (lseek(fd, (off_t)h.blob_offset, SEEK_SET) < 0) return fail(set_error(DHR_ERR_INVALID, "seek failed"));
  if (blob_bytes > 0 && !write_all(fd, blob, (size_t)blob_bytes)) return fail(set_error(DHR_ERR_INVALID, "write failed (blob)"));
  if (blob_bytes == 0 && ftruncate(fd, (off_t)h.blob_offset) != 0) return fail(set_error(DHR_ERR_INVALID, "truncate failed"));
  hipHostFree(pin);
  if (close(fd) != 0) { unlink(path); return set_error(DHR_ERR_INVALID, "close failed"); }
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_index_file_info(const char* path, dhr_file_info* out) try {
  if (!out) return set_error(DHR_ERR_INVALID, "null output");
  FileHeader h;
  int rc = read_header(path, h, nullptr);
  if (rc) return rc;
  out->n_rows = h.n_rows; out->row_offset = h.row_offset; out->d_dlr = h.d_dlr - ((h.pad0 > 0 && h.pad0 < 8) ? h.pad0 : 0); out->d_cls = h.d_cls;
  out->index_dtype = h.idx_dtype; out->idx_buckets = h.idx_buckets; out->file_version = h.version; out->reserved = 0;
  out->payload_bytes = (int64_t)(h.val_bytes + h.idx_bytes);
  out->blob_offset = (int64_t)h.blob_offset; out->blob_bytes = (int64_t)h.blob_bytes;
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_index_load(const char* path, int32_t device, int64_t row_offset, dhr_index** out) try {
  if (!out) return set_error(DHR_ERR_INVALID, "null output");
  *out = nullptr;
  FileHeader h;
  int fd = -1;
  int rc = read_header(path, h, &fd);
  if (rc) return rc;
  struct stat sb;
  if (fstat(fd, &sb) != 0) { close(fd); return set_error(DHR_ERR_INVALID, "fstat failed"); }
  const int es = h.idx_bytes ? idx_esize(h.idx_dtype) : 0;
  if (h.val_offset + h.val_bytes > (uint64_t)sb.st_size || h.idx_offset + h.idx_bytes > (uint64_t)sb.st_size ||
      h.n_rows <= 0 || h.k_rm < h.d_dlr + h.d_cls || h.val_bytes != (uint64_t)h.n_rows * h.k_rm * 2 ||
      h.idx_bytes != (uint64_t)(es ? h.n_rows * h.d_dlr * es : 0)) {
    close(fd);
    return set_error(DHR_ERR_INVALID, std::string(path) + " is truncated or inconsistent");
  }
  void* map = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
  close(fd);
  if (map == MAP_FAILED) return set_error(DHR_ERR_INVALID, "mmap failed");
  (void)madvise(map, (size_t)sb.st_size, MADV_SEQUENTIAL);
  dhr_index_desc d{};
  d.device = device; d.mem_kind = DHR_MEM_HOST; d.n_rows = h.n_rows; d.d_dlr = h.d_dlr; d.d_cls = h.d_cls;
  d.value = (const char*)map + h.val_offset; d.ld_value = h.k_rm;
  d.index = h.idx_bytes ? (const char*)map + h.idx_offset : nullptr; d.index_dtype = h.idx_bytes ? h.idx_dtype : DHR_IDX_NONE;
  d.idx_buckets = h.idx_buckets; d.ld_index = h.d_dlr;
  d.row_offset = row_offset >= 0 ? row_offset : h.row_offset;
  rc = dhr_index_create(&d, out);
  munmap(map, (size_t)sb.st_size);
  if (rc == DHR_OK && h.pad0 > 0 && h.pad0 < 8) (*out)->dlr_pad = h.pad0;
  return rc;
} DHR_CATCH_STATUS


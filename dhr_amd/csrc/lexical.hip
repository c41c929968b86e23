// The lexical head of the DHR / Aggretriever encoders (tevatron/DHR/modeling.py:297-300,328-331, tevatron/Aggretriever/modeling.py:274-278,
// 306-310) fused with what the encoder driver does next to its output: densify (tevatron/DHR/utils.py:5-22 + encode.py:155-170,179-194) or
// aggregate (tevatron/Aggretriever/utils.py:16-44 + merge_reps + encode.py:149-153,174-178).  The reference materialises
//   p = softmax(logits[:, 1:])  (fp32, [B, L-1, V]),  reps = max_t (p * w) * mask  ([B, V])
// in three fp32 [B, L-1, V] temporaries; here two kernels read the logits (pass 1 twice per row, the second read mostly from L2) and write the
// index record directly:
//   lexical_stats_kernel  (lexical_common.h, shared with lexical_train.hip) one workgroup per (b, t) row: max_v x, then sum_v exp(x - max) (accumulated in fp64), as torch's softmax does; packs
//                         (max, sum, w, mask) per token.  Masked rows are not read.
//   lexical_fold_kernel   one workgroup per (b, block of output column pairs); the four / eight wave slices of a workgroup split the groups of
//                         the column.  A lane keeps two adjacent columns, walks tokens (coalesced along the vocabulary) inside each group and
//                         the groups in order, then the slices are folded in order through LDS and the epilogue (raw / densify / aggregate)
//                         writes the record.  The logits of masked tokens are not loaded.
// Semantics kept literally: every contribution is (p * w) * mask in fp32 (a masked token folds in a zero with the sign of w), ties keep the
// first token and the first group (torch.max on the device), aggregate(full) is pos * (pos > neg) - neg * (pos <= neg) with its signs of zero.
// NaN and +inf logits are out of scope (an unmasked row must hold a finite value).
#include "op_dispatch.h"
#include "lexical_common.h"

namespace {

struct FoldArgs {
  int64_t ld_batch, ld_token;
  int T, V;
  const float4* stats;       // [batch * T] (max, sum, w, mask); NULL: the input already is [batch, V] lexical reps (T = 1, no softmax)
  int remove;                // first vocabulary column of group 0 (>= 0); a negative remove pads -remove zero columns at the end instead
  int W, n_groups;           // group width (columns of the view [n_groups, W]) and count
  int GS, PB, n_pairs;       // group slices per workgroup, column pairs per workgroup (GS * PB = 256), column pairs of the output
  int64_t batch;
  void* out_val;
  int val_f32;
  int64_t ld_val;
  void* out_idx;
  int idx_i16;
  int64_t ld_idx;
};

template <typename TIN, int MODE>
__global__ void __launch_bounds__(256) lexical_fold_kernel(const TIN* __restrict__ logits, FoldArgs a) {
#pragma clang fp contract(off)
  __shared__ float sh_best[256][2];
  __shared__ int sh_arg[256][2];
  const int lp = threadIdx.x % a.PB, sl = threadIdx.x / a.PB;
  const int pair = blockIdx.x * a.PB + lp;
  const int c0 = 2 * pair;
  const bool live = pair < a.n_pairs;
  const bool has1 = live && c0 + 1 < a.W;
  const int g_lo = (int)((int64_t)sl * a.n_groups / a.GS), g_hi = (int)((int64_t)(sl + 1) * a.n_groups / a.GS);
  const int base = a.remove > 0 ? a.remove : 0;
  for (int64_t b = blockIdx.y; b < a.batch; b += gridDim.y) {
    const TIN* xb = logits + b * a.ld_batch;
    const float4* st = a.stats ? a.stats + b * a.T : nullptr;
    float best0 = 0.f, best1 = 0.f;
    int arg0 = 0, arg1 = 0;
    for (int g = g_lo; g < g_hi; ++g) {
      const int64_t v0 = (int64_t)base + (int64_t)g * a.W + c0;
      const bool in0 = live && v0 < a.V, in1 = has1 && v0 + 1 < a.V;
      // the pair is one aligned load when the group's first column is aligned to the pair (uniform across the workgroup)
      const bool vec = in1 && ((((uintptr_t)(xb + base + (int64_t)g * a.W)) | (uintptr_t)(a.ld_token * sizeof(TIN))) % (2 * sizeof(TIN)) == 0);
      float r0 = 0.f, r1 = 0.f;
      for (int t = 0; t < a.T; ++t) {
        float x0 = 0.f, x1 = 0.f;
        const float4 s = st ? st[t] : make_float4(0.f, 1.f, 1.f, 1.f);
        if (s.w != 0.f) {
          const TIN* p = xb + (int64_t)t * a.ld_token + v0;
          if (vec) {
            const typename Pair<TIN>::type v = *reinterpret_cast<const typename Pair<TIN>::type*>(p);
            x0 = (float)v.x; x1 = (float)v.y;
          } else {
            if (in0) x0 = (float)p[0];
            if (in1) x1 = (float)p[1];
          }
        }
        float c0v, c1v;
        if (st) {
          const float p0 = s.w != 0.f ? expf(x0 - s.x) / s.y : 0.f;
          const float p1 = s.w != 0.f ? expf(x1 - s.x) / s.y : 0.f;
          c0v = (p0 * s.z) * s.w;
          c1v = (p1 * s.z) * s.w;
        } else {
          c0v = x0; c1v = x1;
        }
        if (t == 0 || c0v > r0) r0 = c0v;                 // first token wins a tie (the sign of a zero maximum)
        if (t == 0 || c1v > r1) r1 = c1v;
      }
      if (!in0) r0 = 0.f;                                  // a padded column (aggregate with a negative remove) is +0
      if (!in1) r1 = 0.f;
      if (g == g_lo || r0 > best0) { best0 = r0; arg0 = g; }   // first group wins a tie
      if (g == g_lo || r1 > best1) { best1 = r1; arg1 = g; }
    }
    if (a.GS > 1) {
      sh_best[threadIdx.x][0] = best0; sh_best[threadIdx.x][1] = best1;
      sh_arg[threadIdx.x][0] = arg0; sh_arg[threadIdx.x][1] = arg1;
      __syncthreads();
      if (sl == 0) {
        for (int k = 1; k < a.GS; ++k) {                    // slices in group order: the earlier one keeps a tie
          const int o = k * a.PB + lp;
          if (sh_best[o][0] > best0) { best0 = sh_best[o][0]; arg0 = sh_arg[o][0]; }
          if (sh_best[o][1] > best1) { best1 = sh_best[o][1]; arg1 = sh_arg[o][1]; }
        }
      }
      __syncthreads();
    }
    if (sl != 0 || !live) continue;
    if (MODE == MODE_AGG_FULL) {
      const float pos = best0, neg = best1;
      const float tok = agg_full_value(pos, neg);
      if (a.val_f32) ((float*)a.out_val)[b * a.ld_val + pair] = tok;
      else ((__half*)a.out_val)[b * a.ld_val + pair] = __float2half(tok);
      continue;
    }
    if (a.val_f32) {
      ((float*)a.out_val)[b * a.ld_val + c0] = best0;
      if (has1) ((float*)a.out_val)[b * a.ld_val + c0 + 1] = best1;
    } else {
      ((__half*)a.out_val)[b * a.ld_val + c0] = __float2half(best0);
      if (has1) ((__half*)a.out_val)[b * a.ld_val + c0 + 1] = __float2half(best1);
    }
    if (MODE == MODE_DENSIFY) {
      if (a.idx_i16) {
        ((int16_t*)a.out_idx)[b * a.ld_idx + c0] = (int16_t)arg0;
        if (has1) ((int16_t*)a.out_idx)[b * a.ld_idx + c0 + 1] = (int16_t)arg1;
      } else {
        ((uint8_t*)a.out_idx)[b * a.ld_idx + c0] = (uint8_t)arg0;
        if (has1) ((uint8_t*)a.out_idx)[b * a.ld_idx + c0 + 1] = (uint8_t)arg1;
      }
    }
  }
}

// the [CLS] reps into the record columns [col0, col0 + cls_dim) (merge_reps; the fp16 cast of encode.py)
__global__ void __launch_bounds__(256) lexical_cls_kernel(const void* __restrict__ cls, int cls_f32, int64_t ld_cls, int cls_dim, int64_t batch,
                                                          void* __restrict__ out, int out_f32, int64_t ld_out, int col0) {
  const int64_t n = batch * cls_dim;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / cls_dim;
    const int j = (int)(i - b * cls_dim);
    const float v = cls_f32 ? ((const float*)cls)[b * ld_cls + j] : (float)((const _Float16*)cls)[b * ld_cls + j];
    if (out_f32) ((float*)out)[b * ld_out + col0 + j] = v;
    else ((__half*)out)[b * ld_out + col0 + j] = __float2half(v);
  }
}

hipError_t launch_fold(const void* logits, int in_dtype, int mode, const FoldArgs& a0, hipStream_t s) {
  FoldArgs a = a0;
  a.GS = a.n_groups >= 8 ? 8 : a.n_groups >= 4 ? 4 : a.n_groups >= 2 ? 2 : 1;
  a.PB = 256 / a.GS;
  a.n_pairs = mode == MODE_AGG_FULL ? a.W / 2 : (a.W + 1) / 2;
  const dim3 grid((unsigned)((a.n_pairs + a.PB - 1) / a.PB), (unsigned)std::min<int64_t>(a.batch, 65535));
  with_value_type_bf16(in_dtype, [&](auto t) { with_int<MODE_RAW, MODE_DENSIFY, MODE_AGG_FULL, MODE_AGG_SEMI>(mode, [&](auto m) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((lexical_fold_kernel<T, decltype(m)::value>), grid, dim3(256), 0, s, (const T*)logits, a);
  }); });
  return hipGetLastError();
}

}  // namespace

// declared in lexical_common.h: the epilogues above on fp32 reps that another translation unit computed (lexical_proj.hip)
hipError_t dhr::lexical_record_from_reps(const float* reps, int64_t ld_reps, int mode, int64_t batch, int vocab, int out_cols, int W, int n_groups,
                                         int remove, void* out_val, int val_f32, int64_t ld_val, void* out_idx, int idx_i16, int64_t ld_idx,
                                         const void* cls, int cls_f32, int64_t ld_cls, int cls_dim, hipStream_t s) {
  if (reps) {
    FoldArgs a{};
    a.ld_batch = ld_reps; a.ld_token = vocab; a.T = 1; a.V = vocab; a.stats = nullptr;
    a.remove = remove; a.W = W; a.n_groups = n_groups; a.batch = batch;
    a.out_val = out_val; a.val_f32 = val_f32; a.ld_val = ld_val; a.out_idx = out_idx; a.idx_i16 = idx_i16; a.ld_idx = ld_idx;
    const hipError_t e = launch_fold(reps, DHR_VAL_F32, mode, a, s);
    if (e != hipSuccess) return e;
  }
  if (cls_dim > 0) {
    const unsigned blocks = (unsigned)std::min<int64_t>((batch * cls_dim + 255) / 256, 4096);
    hipLaunchKernelGGL(lexical_cls_kernel, dim3(blocks), dim3(256), 0, s, cls, cls_f32, ld_cls, cls_dim, batch, out_val, val_f32, ld_val, out_cols);
  }
  return hipGetLastError();
}

extern "C" int dhr_lexical_head(int32_t device, int32_t mem_kind, int32_t mode, const void* logits, int32_t logits_dtype, int64_t batch,
                                int32_t n_tokens, int32_t vocab, int64_t ld_batch, int64_t ld_token, const float* term_weights, int64_t ld_weights,
                                const float* mask, int64_t ld_mask, int32_t dims, int32_t remove_dims, void* out_value, int32_t out_value_dtype,
                                int64_t ld_value, void* out_index, int32_t index_dtype, int64_t ld_index, const void* cls, int32_t cls_dtype,
                                int64_t ld_cls, int32_t cls_dim, void* workspace, void* stream) try {
  dhr::alloc_checkpoint();
  if (!logits || !term_weights || !mask || !out_value) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!val_ok_bf16(logits_dtype) || !val_ok(out_value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (batch < 0 || n_tokens <= 0 || vocab <= 0 || ld_token < vocab || ld_batch < (int64_t)(n_tokens - 1) * ld_token + vocab ||
      ld_weights < n_tokens || ld_mask < n_tokens || cls_dim < 0 || (int64_t)batch * n_tokens > ((int64_t)1 << 31) - 1)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  Geometry geo;
  int rc = check_record(mode, vocab, dims, remove_dims, ld_value, out_index, index_dtype, ld_index, cls, cls_dtype, ld_cls, cls_dim, geo);
  if (rc) return rc;
  if (batch == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int ies = val_esize(logits_dtype), oes = val_esize(out_value_dtype), xes = index_dtype == DHR_IDX_I16 ? 2 : 1, ces = val_esize(cls_dtype);
  const int T = n_tokens;
  FoldArgs a{};
  a.T = T; a.V = vocab; a.remove = geo.remove; a.W = geo.W; a.n_groups = geo.n_groups;
  a.val_f32 = out_value_dtype == DHR_VAL_F32; a.idx_i16 = index_dtype == DHR_IDX_I16;
  auto run = [&](const void* lg, int64_t ldb, int64_t ldt, const float* w, int64_t ldw, const float* m, int64_t ldm, int64_t rows, float4* stats,
                 void* val, int64_t ldv, void* idx, int64_t ldi, const void* c, int64_t ldc) -> int {
    with_value_type_bf16(logits_dtype, [&](auto t) {
      using TIN = typename decltype(t)::type;
      hipLaunchKernelGGL(lexical_stats_kernel<TIN>, dim3((unsigned)(rows * T)), dim3(256), 0, s, (const TIN*)lg, ldb, ldt, T, vocab, w, ldw, m, ldm,
                         stats);
    });
    HIP_TRY(hipGetLastError());
    FoldArgs f = a;
    f.ld_batch = ldb; f.ld_token = ldt; f.stats = stats; f.batch = rows;
    f.out_val = val; f.ld_val = ldv; f.out_idx = idx; f.ld_idx = ldi;
    HIP_TRY(launch_fold(lg, logits_dtype, mode, f, s));
    if (cls_dim > 0) {
      const unsigned blocks = (unsigned)std::min<int64_t>((rows * cls_dim + 255) / 256, 4096);
      hipLaunchKernelGGL(lexical_cls_kernel, dim3(blocks), dim3(256), 0, s, c, cls_dtype == DHR_VAL_F32, ldc, cls_dim, rows, val,
                         out_value_dtype == DHR_VAL_F32, ldv, geo.out_cols);
      HIP_TRY(hipGetLastError());
    }
    return DHR_OK;
  };
  if (mem_kind == DHR_MEM_DEVICE) {
    DevMem ws_mem;
    void* ws = workspace;
    if (!ws) HIP_TRY(dev_alloc(ws_mem, batch * T * (int64_t)sizeof(float4)));
    if (!ws) ws = ws_mem.p;
    rc = run(logits, ld_batch, ld_token, term_weights, ld_weights, mask, ld_mask, batch, (float4*)ws, out_value, ld_value, out_index, ld_index, cls, ld_cls);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return DHR_OK;
  }
  // host arrays: stage blocks of rows through the device (logits packed [rows, T, vocab])
  const int64_t per_row = (int64_t)T * vocab * ies;
  const int64_t block = std::max<int64_t>(1, std::min<int64_t>(batch, ((int64_t)256 << 20) / per_row));
  const int64_t ldv = geo.out_cols + cls_dim;
  DevMem m_in, m_w, m_m, m_st, m_val, m_idx, m_cls;
  HIP_TRY(dev_alloc(m_in, block * per_row));
  HIP_TRY(dev_alloc(m_w, block * T * 4));
  HIP_TRY(dev_alloc(m_m, block * T * 4));
  HIP_TRY(dev_alloc(m_st, block * T * (int64_t)sizeof(float4)));
  HIP_TRY(dev_alloc(m_val, block * ldv * oes));
  if (mode == MODE_DENSIFY) HIP_TRY(dev_alloc(m_idx, block * geo.out_cols * xes));
  if (cls_dim > 0) HIP_TRY(dev_alloc(m_cls, block * cls_dim * ces));
  for (int64_t lo = 0; lo < batch; lo += block) {
    const int64_t rows = std::min(block, batch - lo);
    for (int64_t r = 0; r < rows; ++r)
      HIP_TRY(copy_in((char*)m_in.p + r * per_row, (const char*)logits + (lo + r) * ld_batch * ies, ld_token, T, vocab, ies, s));
    HIP_TRY(copy_in(m_w.p, term_weights + lo * ld_weights, ld_weights, rows, T, 4, s));
    HIP_TRY(copy_in(m_m.p, mask + lo * ld_mask, ld_mask, rows, T, 4, s));
    if (cls_dim > 0) HIP_TRY(copy_in(m_cls.p, (const char*)cls + lo * ld_cls * ces, ld_cls, rows, cls_dim, ces, s));
    rc = run(m_in.p, (int64_t)T * vocab, vocab, (const float*)m_w.p, T, (const float*)m_m.p, T, rows, (float4*)m_st.p, m_val.p, ldv, m_idx.p, geo.out_cols,
             m_cls.p, cls_dim);
    if (rc) return rc;
    HIP_TRY(stage_out((char*)out_value + lo * ld_value * oes, ld_value, m_val.p, rows, ldv, oes, s));
    if (mode == MODE_DENSIFY) HIP_TRY(stage_out((char*)out_index + lo * ld_index * xes, ld_index, m_idx.p, rows, geo.out_cols, xes, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_aggregate(int32_t device, int32_t mem_kind, const void* lexical, int32_t value_dtype, int64_t ld, int64_t batch, int32_t vocab,
                             int32_t dims, int32_t remove_dims, int32_t full, void* out, int32_t out_dtype, int64_t ld_out, void* stream) try {
  dhr::alloc_checkpoint();
  if (!lexical || !out) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!val_ok(value_dtype) || !val_ok(out_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (batch < 0 || vocab <= 0 || ld < vocab || ld_out < dims) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  const int mode = full ? MODE_AGG_FULL : MODE_AGG_SEMI;
  Geometry geo;
  if (int rc = geometry(mode, vocab, dims, remove_dims, geo)) return rc;
  if (batch == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int ies = val_esize(value_dtype), oes = val_esize(out_dtype);
  FoldArgs a{};
  a.ld_batch = ld; a.ld_token = vocab; a.T = 1; a.V = vocab; a.stats = nullptr;
  a.remove = geo.remove; a.W = geo.W; a.n_groups = geo.n_groups; a.val_f32 = out_dtype == DHR_VAL_F32;
  if (mem_kind == DHR_MEM_DEVICE) {
    a.batch = batch; a.out_val = out; a.ld_val = ld_out;
    HIP_TRY(launch_fold(lexical, value_dtype, mode, a, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DHR_OK;
  }
  const int64_t block = std::max<int64_t>(1, std::min<int64_t>(batch, ((int64_t)256 << 20) / ((int64_t)vocab * ies)));
  DevMem m_in, m_out;
  HIP_TRY(dev_alloc(m_in, block * vocab * ies));
  HIP_TRY(dev_alloc(m_out, block * dims * oes));
  a.ld_batch = vocab; a.out_val = m_out.p; a.ld_val = dims;
  for (int64_t lo = 0; lo < batch; lo += block) {
    const int64_t rows = std::min(block, batch - lo);
    a.batch = rows;
    HIP_TRY(copy_in(m_in.p, (const char*)lexical + lo * ld * ies, ld, rows, vocab, ies, s));
    HIP_TRY(launch_fold(m_in.p, value_dtype, mode, a, s));
    HIP_TRY(stage_out((char*)out + lo * ld_out * oes, ld_out, m_out.p, rows, dims, oes, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DHR_OK;
} DHR_CATCH_STATUS

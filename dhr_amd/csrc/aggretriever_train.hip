// The two stretches of an Aggretriever TRAINING step that follow the encoder, forward and backward: aggregate under autograd
// (tevatron/Aggretriever/utils.py:16-44, called at modeling.py:173-174) and the head without the MLM logits (--skip_mlm, modeling.py:279-284,
// 311-316).  Both are selections: every output is an input value, its negation or zero, so there is no rounding anywhere.
//   aggregate_route_kernel            the aggregate fold of lexical.hip on [B, V] reps (no tokens, no softmax) -- the same comparisons in the same
//                                     order and agg_full_value of lexical_common.h, so the values are bit-identical to dhr_aggregate -- which
//                                     also writes route (int16): the first group that attains the maximum and, for aggregate(full), which of
//                                     the two signed columns was taken.  A workgroup owns (b, a block of column pairs); its wave slices split
//                                     the groups and are folded in group order through LDS.
//   aggregate_backward_kernel         the whole [B, V] gradient row in one pass: a thread owns 8 adjacent vocabulary columns, looks up the route of
//                                     the output column each belongs to and stores +G, -G or zero.  Every column is written exactly by its owner:
//                                     no memset, no atomics.  A winner in the zero padding has no column, so nothing is written for it.
//   term_weight_head_kernel           reps[b][v] = max(0, max over {t : ids[b][t] == v} of w[b][t]) without the [B, L, V] tensor.  A workgroup owns
//                                     (b, 4096 columns): one 64-bit key per column in LDS, zero = "the zero wins"; every token with a strictly
//                                     positive weight whose id falls into the block folds (weight bits, 65535 - t) into its column's key with an
//                                     LDS maximum.  The bits of positive floats order like the floats, so the largest key is the largest weight
//                                     at its lowest position whatever the order of the tokens: two runs are bit-identical.  The block's columns
//                                     of reps (fp32) and tok (int16) are then written in full by vector stores.  Ids outside [0, vocab) match no
//                                     block and are never used as an index.
//   term_weight_head_backward_kernel  the gather: dw[b][t] = grad[b][v] where tok[b][v] == t (v = ids[b][t] inside the vocabulary), else zero.
// Everything is enqueued on the caller's stream; nothing is allocated.
#include "host_stage.h"
#include "op_dispatch.h"
#include "lexical_common.h"

namespace {

constexpr int MAX_TOKENS = 32767;
constexpr int MAX_GROUPS = 16383;   // 2 * g + 1 must fit the int16 route
constexpr int BC = 8;               // adjacent columns per thread of the row-writing passes
constexpr int CH = 4096;            // columns per workgroup of the term-weight head (32 KB of keys)

struct AggArgs {
  int64_t ld;
  int V, remove, W, n_groups;
  int GS, PB, n_pairs;       // group slices per workgroup, column pairs per workgroup (GS * PB = 256), column pairs of a group
  int64_t batch;
  void* out;
  int out_f32;
  int64_t ld_out;
  int16_t* route;            // may be NULL
  int64_t ld_route;
};

// lexical_fold_kernel<TIN, MODE_AGG_FULL / MODE_AGG_SEMI> without tokens (stats == NULL, T = 1), keeping the winners
template <typename TIN, bool FULL>
__global__ void __launch_bounds__(256) aggregate_route_kernel(const TIN* __restrict__ reps, AggArgs a) {
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
    const TIN* xb = reps + b * a.ld;
    float best0 = 0.f, best1 = 0.f;
    int arg0 = 0, arg1 = 0;
    for (int g = g_lo; g < g_hi; ++g) {
      const int64_t v0 = (int64_t)base + (int64_t)g * a.W + c0;
      const bool in0 = live && v0 < a.V, in1 = has1 && v0 + 1 < a.V;
      float r0 = 0.f, r1 = 0.f;                                // a padded column (a negative remove) is +0
      if (in1 && (uintptr_t)(xb + v0) % (2 * sizeof(TIN)) == 0) {
        const typename Pair<TIN>::type v = *reinterpret_cast<const typename Pair<TIN>::type*>(xb + v0);
        r0 = (float)v.x; r1 = (float)v.y;
      } else {
        if (in0) r0 = (float)xb[v0];
        if (in1) r1 = (float)xb[v0 + 1];
      }
      if (g == g_lo || r0 > best0) { best0 = r0; arg0 = g; }   // first group wins a tie
      if (g == g_lo || r1 > best1) { best1 = r1; arg1 = g; }
    }
    if (a.GS > 1) {
      sh_best[threadIdx.x][0] = best0; sh_best[threadIdx.x][1] = best1;
      sh_arg[threadIdx.x][0] = arg0; sh_arg[threadIdx.x][1] = arg1;
      __syncthreads();
      if (sl == 0) {
        for (int k = 1; k < a.GS; ++k) {                        // slices in group order: the earlier one keeps a tie
          const int o = k * a.PB + lp;
          if (sh_best[o][0] > best0) { best0 = sh_best[o][0]; arg0 = sh_arg[o][0]; }
          if (sh_best[o][1] > best1) { best1 = sh_best[o][1]; arg1 = sh_arg[o][1]; }
        }
      }
      __syncthreads();
    }
    if (sl != 0 || !live) continue;
    if (FULL) {
      const float pos = best0, neg = best1;
      const float tok = agg_full_value(pos, neg);
      if (a.out_f32) ((float*)a.out)[b * a.ld_out + pair] = tok;
      else ((__half*)a.out)[b * a.ld_out + pair] = __float2half(tok);
      if (a.route) a.route[b * a.ld_route + pair] = (int16_t)(pos > neg ? 2 * arg0 : 2 * arg1 + 1);
      continue;
    }
    if (a.out_f32) {
      ((float*)a.out)[b * a.ld_out + c0] = best0;
      if (has1) ((float*)a.out)[b * a.ld_out + c0 + 1] = best1;
    } else {
      ((__half*)a.out)[b * a.ld_out + c0] = __float2half(best0);
      if (has1) ((__half*)a.out)[b * a.ld_out + c0 + 1] = __float2half(best1);
    }
    if (a.route) {
      a.route[b * a.ld_route + c0] = (int16_t)arg0;
      if (has1) a.route[b * a.ld_route + c0 + 1] = (int16_t)arg1;
    }
  }
}

// grad_lexical[b][v] for every v in [0, V): vocabulary column base + g * W + c belongs to output column c (c / 2 with sign c & 1 for FULL)
template <typename TG, bool FULL, bool VEC>
__global__ void __launch_bounds__(256) aggregate_backward_kernel(const TG* __restrict__ grad, int64_t ld_grad, const int16_t* __restrict__ route,
                                                                 int64_t ld_route, int64_t batch, int V, int base, int W, TG* __restrict__ dx,
                                                                 int64_t ld_dx) {
  int c0 = (blockIdx.x * 256 + threadIdx.x) * BC;
  if (c0 >= V) return;
  if (VEC) c0 = min(c0, V - BC);       // the last thread of a row steps back to whole vectors (it rewrites up to BC - 1 columns with the same values)
  const int n = VEC ? BC : min(BC, V - c0);
  const int u0 = max(c0 - base, 0);    // the first of this thread's columns that lies in a group, counted from the first group
  const int g0 = u0 / W, r0 = u0 - g0 * W;
  for (int64_t b = blockIdx.y; b < batch; b += gridDim.y) {
    const TG* gb = grad + b * ld_grad;
    const int16_t* rb = route + b * ld_route;
    TG o[BC];
    int g = g0, c = r0;
#pragma unroll
    for (int i = 0; i < BC; ++i) {
      TG val = (TG)0.f;
      if (i < n && c0 + i >= base) {                     // (the removed leading columns are zeros)
        const int j = FULL ? c >> 1 : c;
        const int want = FULL ? 2 * g + (c & 1) : g;
        if ((int)rb[j] == want) val = FULL && (c & 1) ? -gb[j] : gb[j];
        if (++c == W) { c = 0; ++g; }
      }
      o[i] = val;
    }
    store_cols<TG, VEC>(dx + b * ld_dx + c0, n, o);
  }
}

// ids / w point at the first token that takes part
template <typename TID, typename TW, bool VEC>
__global__ void __launch_bounds__(256) term_weight_head_kernel(const TID* __restrict__ ids, int64_t ld_ids, const TW* __restrict__ w, int64_t ld_w,
                                                               int64_t batch, int T, int V, float* __restrict__ reps, int64_t ld_reps,
                                                               int16_t* __restrict__ tok, int64_t ld_tok) {
  __shared__ unsigned long long key[CH];
  const int v_lo = blockIdx.x * CH, v_hi = min(v_lo + CH, V);
  for (int64_t b = blockIdx.y; b < batch; b += gridDim.y) {
    for (int i = threadIdx.x; i < CH; i += 256) key[i] = 0ull;
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += 256) {
      const int64_t id = (int64_t)ids[b * ld_ids + t];
      const float x = (float)w[b * ld_w + t];
      if (id >= v_lo && id < v_hi && x > 0.f)              // (an id outside the vocabulary is in no block's range)
        atomicMax(&key[(int)(id - v_lo)], ((unsigned long long)__float_as_uint(x) << 16) | (unsigned long long)(65535 - t));
    }
    __syncthreads();
    for (int c = threadIdx.x * BC; v_lo + c < v_hi; c += 256 * BC) {
      const int n = min(BC, v_hi - v_lo - c);
      float r[BC];
      int16_t k[BC];
#pragma unroll
      for (int i = 0; i < BC; ++i) {
        const unsigned long long q = key[c + i];           // (c + i < CH: c is a multiple of BC below CH)
        r[i] = q ? __uint_as_float((unsigned)(q >> 16)) : 0.f;
        k[i] = q ? (int16_t)(65535 - (int)(q & 0xffffull)) : (int16_t)-1;
      }
      store_cols<float, true>(reps + b * ld_reps + v_lo + c, n, r);
      store_cols<int16_t, VEC>(tok + b * ld_tok + v_lo + c, n, k);
    }
    __syncthreads();
  }
}

template <typename TID, typename TW>
__global__ void __launch_bounds__(256) term_weight_head_backward_kernel(const TID* __restrict__ ids, int64_t ld_ids, int64_t batch, int T, int V,
                                                                        const float* __restrict__ grad, int64_t ld_grad,
                                                                        const int16_t* __restrict__ tok, int64_t ld_tok, TW* __restrict__ dw,
                                                                        int64_t ld_dw) {
  const int64_t n = batch * T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / T;
    const int t = (int)(i - b * T);
    const int64_t id = (int64_t)ids[b * ld_ids + t];
    float val = 0.f;
    if (id >= 0 && id < V && (int)tok[b * ld_tok + id] == t) val = grad[b * ld_grad + id];
    dw[b * ld_dw + t] = (TW)val;
  }
}

// the checks the two aggregate entry points share
int check_aggregate(int32_t mem_kind, int64_t batch, int32_t vocab, int32_t dims, int32_t remove_dims, int32_t full, const char* what, Geometry& geo) {
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (batch <= 0 || vocab <= 0) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  int rc = geometry(full ? MODE_AGG_FULL : MODE_AGG_SEMI, vocab, dims, remove_dims, geo);
  if (rc) return rc;
  if (geo.n_groups > MAX_GROUPS) return set_error(DHR_ERR_UNSUPPORTED, "more than 16383 groups (the route is int16 and holds 2 * group + 1)");
  if (mem_kind != DHR_MEM_DEVICE)
    return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": host arrays are not staged, training tensors live on the device (DHR_MEM_DEVICE)");
  return DHR_OK;
}

// the checks the two entry points of the term-weight head share: n_tokens counts the tokens after the skipped ones
int check_term_head(const void* input_ids, int32_t mem_kind, int32_t id_bytes, int64_t ld_ids, int64_t batch, int32_t n_tokens, int32_t skip_tokens,
                    int32_t vocab, const char* what) {
  if (!input_ids) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (id_bytes != 4 && id_bytes != 8) return set_error(DHR_ERR_INVALID, "input ids must be int32 or int64 (id_bytes 4 or 8)");
  if (batch <= 0 || n_tokens <= 0 || vocab <= 0 || skip_tokens < 0 || skip_tokens > MAX_TOKENS || ld_ids < (int64_t)skip_tokens + n_tokens ||
      batch * n_tokens > ((int64_t)1 << 31) - 1)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (n_tokens > MAX_TOKENS) return set_error(DHR_ERR_UNSUPPORTED, "more than 32767 tokens (the token index is int16)");
  if (mem_kind != DHR_MEM_DEVICE)
    return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": host arrays are not staged, training tensors live on the device (DHR_MEM_DEVICE)");
  return DHR_OK;
}

}  // namespace

extern "C" int dhr_aggregate_train(int32_t device, int32_t mem_kind, const void* lexical, int32_t value_dtype, int64_t ld, int64_t batch,
                                   int32_t vocab, int32_t dims, int32_t remove_dims, int32_t full, void* out, int32_t out_dtype, int64_t ld_out,
                                   int16_t* route, int64_t ld_route, void* stream) try {
  dhr::alloc_checkpoint();
  if (!lexical || !out) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!val_ok(value_dtype) || !val_ok(out_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (ld < vocab || ld_out < dims || (route && ld_route < dims)) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  Geometry geo;
  int rc = check_aggregate(mem_kind, batch, vocab, dims, remove_dims, full, "dhr_aggregate_train", geo);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  AggArgs a{};
  a.ld = ld; a.V = vocab; a.remove = geo.remove; a.W = geo.W; a.n_groups = geo.n_groups;
  a.GS = a.n_groups >= 8 ? 8 : a.n_groups >= 4 ? 4 : a.n_groups >= 2 ? 2 : 1;       // (the launch geometry of dhr_aggregate)
  a.PB = 256 / a.GS;
  a.n_pairs = full ? a.W / 2 : (a.W + 1) / 2;
  a.batch = batch; a.out = out; a.out_f32 = out_dtype == DHR_VAL_F32; a.ld_out = ld_out; a.route = route; a.ld_route = ld_route;
  const dim3 grid((unsigned)((a.n_pairs + a.PB - 1) / a.PB), (unsigned)std::min<int64_t>(batch, 65535));
  with_value_type(value_dtype, [&](auto t) { with_flag(full != 0, [&](auto f) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((aggregate_route_kernel<T, decltype(f)::value>), grid, dim3(256), 0, s, (const T*)lexical, a);
  }); });
  HIP_TRY(hipGetLastError());
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_aggregate_backward(int32_t device, int32_t mem_kind, const void* grad_out, int32_t grad_dtype, int64_t ld_grad_out,
                                      const int16_t* route, int64_t ld_route, int64_t batch, int32_t vocab, int32_t dims, int32_t remove_dims,
                                      int32_t full, void* grad_lexical, int64_t ld_grad, void* stream) try {
  dhr::alloc_checkpoint();
  if (!grad_out || !route || !grad_lexical) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!val_ok(grad_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (ld_grad < vocab || ld_grad_out < dims || ld_route < dims) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  Geometry geo;
  int rc = check_aggregate(mem_kind, batch, vocab, dims, remove_dims, full, "dhr_aggregate_backward", geo);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int es = grad_dtype == DHR_VAL_F32 ? 4 : 2;
  // multi-dword stores need every row of the gradient (and the stepped-back last vector) at a multiple of 4 bytes
  const bool vec = vocab >= BC && (int64_t)vocab * es % 4 == 0 && ((uintptr_t)grad_lexical | (uintptr_t)(ld_grad * es)) % 4 == 0;
  const int base = geo.remove > 0 ? geo.remove : 0;
  const dim3 grid((unsigned)((vocab + 256 * BC - 1) / (256 * BC)), (unsigned)std::min<int64_t>(batch, 65535));
  with_value_type(grad_dtype, [&](auto t) { with_flag(full != 0, [&](auto f) { with_flag(vec, [&](auto v) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((aggregate_backward_kernel<T, decltype(f)::value, decltype(v)::value>), grid, dim3(256), 0, s, (const T*)grad_out, ld_grad_out,
                       route, ld_route, batch, vocab, base, geo.W, (T*)grad_lexical, ld_grad);
  }); }); });
  HIP_TRY(hipGetLastError());
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_term_weight_head(int32_t device, int32_t mem_kind, const void* input_ids, int32_t id_bytes, int64_t ld_ids,
                                    const void* term_weights, int32_t value_dtype, int64_t ld_weights, int64_t batch, int32_t n_tokens,
                                    int32_t skip_tokens, int32_t vocab, float* out_reps, int64_t ld_reps, int16_t* out_tokens, int64_t ld_tokens,
                                    void* stream) try {
  dhr::alloc_checkpoint();
  if (!term_weights || !out_reps || !out_tokens) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!val_ok(value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (ld_weights < n_tokens || ld_reps < vocab || ld_tokens < vocab) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  int rc = check_term_head(input_ids, mem_kind, id_bytes, ld_ids, batch, n_tokens, skip_tokens, vocab, "dhr_term_weight_head");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  // the int16 row of tok takes multi-dword stores when every row starts at a multiple of 4 bytes (a workgroup's columns start at a multiple of 8)
  const bool vec = ((uintptr_t)out_tokens | (uintptr_t)(ld_tokens * 2)) % 4 == 0;
  const dim3 grid((unsigned)((vocab + CH - 1) / CH), (unsigned)std::min<int64_t>(batch, 65535));
  with_id_type(id_bytes, [&](auto i) { with_value_type(value_dtype, [&](auto w) { with_flag(vec, [&](auto v) {
    using I = typename decltype(i)::type;
    using W = typename decltype(w)::type;
    hipLaunchKernelGGL((term_weight_head_kernel<I, W, decltype(v)::value>), grid, dim3(256), 0, s, (const I*)input_ids + skip_tokens, ld_ids,
                       (const W*)term_weights, ld_weights, batch, n_tokens, vocab, out_reps, ld_reps, out_tokens, ld_tokens);
  }); }); });
  HIP_TRY(hipGetLastError());
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_term_weight_head_backward(int32_t device, int32_t mem_kind, const void* input_ids, int32_t id_bytes, int64_t ld_ids, int64_t batch,
                                             int32_t n_tokens, int32_t skip_tokens, int32_t vocab, const float* grad_reps, int64_t ld_grad_reps,
                                             const int16_t* tokens, int64_t ld_tokens, void* grad_weights, int32_t grad_dtype,
                                             int64_t ld_grad_weights, void* stream) try {
  dhr::alloc_checkpoint();
  if (!grad_reps || !tokens || !grad_weights) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!val_ok(grad_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (ld_grad_reps < vocab || ld_tokens < vocab || ld_grad_weights < n_tokens) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  int rc = check_term_head(input_ids, mem_kind, id_bytes, ld_ids, batch, n_tokens, skip_tokens, vocab, "dhr_term_weight_head_backward");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)std::min<int64_t>((batch * n_tokens + 255) / 256, 4096));
  with_id_type(id_bytes, [&](auto i) { with_value_type(grad_dtype, [&](auto w) {
    using I = typename decltype(i)::type;
    using W = typename decltype(w)::type;
    hipLaunchKernelGGL((term_weight_head_backward_kernel<I, W>), grid, dim3(256), 0, s, (const I*)input_ids + skip_tokens, ld_ids, batch, n_tokens,
                       vocab, grad_reps, ld_grad_reps, tokens, ld_tokens, (W*)grad_weights, ld_grad_weights);
  }); });
  HIP_TRY(hipGetLastError());
  return DHR_OK;
} DHR_CATCH_STATUS

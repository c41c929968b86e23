// The lexical head of a DHR / Aggretriever TRAINING step, forward and backward (tevatron/DHR/modeling.py:294-300, 325-331,
// tevatron/Aggretriever/modeling.py:274-278, 306-310).  The reference keeps softmax(logits[:, 1:]) and two more fp32 [B, L-1, V] tensors for
// autograd; here nothing of that size exists besides the logits and their gradient.  With p = softmax_v(x), c = (p * w) * m,
// r[b][v] = max_t c[b][t][v] at the first maximising token tok[b][v] and g = dL/dr:
//   A[b][t]     = sum over {v : tok[b][v] == t} of g[b][v] * p[b][t][v]
//   dL/dw[b][t] = m * A,   D[b][t] = w * m * A,   dL/dx[b][t][v] = p * ([tok[b][v] == t] * g[b][v] * w * m - D)
// Kernels:
//   lexical_stats_kernel      (lexical_common.h, shared with the encoding head) per-token (max, sum, w, m); the sum in fp64
//   lexical_fold_tok_kernel   the raw fold of lexical.hip -- same expressions in the same order, so the reps are bit-identical to
//                             dhr_lexical_head(DHR_LEX_RAW) -- which also writes tok (int16)
//   lexical_route_sum_kernel  A: one workgroup per (b, 16 tokens; 4 on small problems) scans the row's tok; thread i takes the columns i, i + 256,
//                             ... in that order, eight at a time (their loads are unconditional at clamped addresses, so they are in flight
//                             together; what is not routed to the tile is dropped) and adds g * p into its own fp64 slot of the token; the
//                             256 slots of a token are then added in a fixed order (four in sequence per lane, a 64-lane butterfly).
//                             Accumulation is fp64, rounded to fp32 once; there are no atomics, so two runs are bit-identical.
//   lexical_dx_kernel         the streaming pass: a workgroup owns (b, 8 tokens, 2048 columns); a thread keeps g and tok of 8 adjacent columns
//                             in registers and walks the tokens: one 16-byte load of the logits (two for fp32), one store of the gradient in the
//                             logits' dtype (fp16 / bf16: rounded once from fp32, to nearest even).  p is recomputed from the saved (max, sum).  Rows of skipped and masked tokens are written as
//                             zeros without being read.  Rows that are not 4-byte aligned (fp16 with an odd stride) take element-wise accesses.
// Both passes take the model's full [B, L, V] logits and skip_tokens (the reference drops token 0): the gradient of the whole tensor is
// written, so autograd never pads the gradient of a [:, 1:] view.  Everything is enqueued on the caller's stream; nothing is allocated.
#include "host_stage.h"
#include "op_dispatch.h"
#include "lexical_common.h"

namespace {

constexpr int RT_BIG = 16;    // tokens per workgroup of the reduction pass ...
constexpr int RT_SMALL = 4;   // ... and where 16 would leave most of the 256 CUs without a workgroup (the choice depends on the shape alone)
constexpr int DT = 8;         // tokens per workgroup of the streaming pass
constexpr int DC = 8;         // adjacent columns per thread of the streaming pass
constexpr int MAX_TOKENS = 32767;

// the raw mode of lexical_fold_kernel (one group, no slices) with the argmax token
template <typename TIN>
__global__ void __launch_bounds__(256) lexical_fold_tok_kernel(const TIN* __restrict__ logits, int64_t ld_batch, int64_t ld_token, int T, int V,
                                                               int64_t batch, const float4* __restrict__ stats, float* __restrict__ reps,
                                                               int64_t ld_reps, int16_t* __restrict__ tok, int64_t ld_tok) {
#pragma clang fp contract(off)
  const int c0 = 2 * (blockIdx.x * 256 + threadIdx.x);
  const bool in0 = c0 < V, in1 = c0 + 1 < V;
  for (int64_t b = blockIdx.y; b < batch; b += gridDim.y) {
    const TIN* xb = logits + b * ld_batch;
    const float4* st = stats + b * T;
    const bool vec = in1 && (((uintptr_t)xb | (uintptr_t)(ld_token * sizeof(TIN))) % (2 * sizeof(TIN)) == 0);
    float r0 = 0.f, r1 = 0.f;
    int a0 = 0, a1 = 0;
    for (int t = 0; t < T; ++t) {
      float x0 = 0.f, x1 = 0.f;
      const float4 s = st[t];
      if (s.w != 0.f) {
        const TIN* p = xb + (int64_t)t * ld_token + c0;
        if (vec) {
          const typename Pair<TIN>::type v = *reinterpret_cast<const typename Pair<TIN>::type*>(p);
          x0 = (float)v.x; x1 = (float)v.y;
        } else {
          if (in0) x0 = (float)p[0];
          if (in1) x1 = (float)p[1];
        }
      }
      const float p0 = s.w != 0.f ? expf(x0 - s.x) / s.y : 0.f;
      const float p1 = s.w != 0.f ? expf(x1 - s.x) / s.y : 0.f;
      const float c0v = (p0 * s.z) * s.w, c1v = (p1 * s.z) * s.w;
      if (t == 0 || c0v > r0) { r0 = c0v; a0 = t; }       // first token wins a tie
      if (t == 0 || c1v > r1) { r1 = c1v; a1 = t; }
    }
    if (in0) { reps[b * ld_reps + c0] = r0; tok[b * ld_tok + c0] = (int16_t)a0; }
    if (in1) { reps[b * ld_reps + c0 + 1] = r1; tok[b * ld_tok + c0 + 1] = (int16_t)a1; }
  }
}

// A[b][t] and dL/dw[b][t] = m * A.  logits points at token skip_tokens of the model's tensor.  RT tokens per workgroup.
template <typename TIN, int RT>
__global__ void __launch_bounds__(256) lexical_route_sum_kernel(const TIN* __restrict__ logits, int64_t ld_batch, int64_t ld_token, int T, int V,
                                                                const float4* __restrict__ stats, const float* __restrict__ g, int64_t ld_g,
                                                                const int16_t* __restrict__ tok, int64_t ld_tok, float* __restrict__ A,
                                                                float* __restrict__ dw, int64_t ld_dw) {
  constexpr int U = 8;                                   // columns a thread has in flight
  __shared__ double acc[RT][256];
  __shared__ float4 sh_st[RT];
  const int64_t b = blockIdx.y;
  const int t0 = blockIdx.x * RT;
  const int nt = min(RT, T - t0);
#pragma unroll
  for (int k = 0; k < RT; ++k) acc[k][threadIdx.x] = 0.0;
  if ((int)threadIdx.x < RT) sh_st[threadIdx.x] = (int)threadIdx.x < nt ? stats[b * T + t0 + threadIdx.x] : make_float4(0.f, 1.f, 0.f, 0.f);
  __syncthreads();
  const TIN* xb = logits + b * ld_batch + (int64_t)t0 * ld_token;
  const float* gb = g + b * ld_g;
  const int16_t* tb = tok + b * ld_tok;
  for (int base = threadIdx.x; base < V; base += 256 * U) {
    // every load is unconditional at a clamped address (a column past the end repeats the last one, a token of another tile or a masked
    // one reads the tile's first row): the U gathers of a thread are in flight together, and what is not routed here is dropped below
    int k[U];
    float x[U], gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) k[u] = (int)tb[min(base + 256 * u, V - 1)] - t0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = base + 256 * u;
      const int kc = min(max(k[u], 0), RT - 1);
      if (v >= V || k[u] != kc || sh_st[kc].w == 0.f) k[u] = -1;     // (masked: m * A and w * m * A are zero whatever A is)
      x[u] = (float)xb[(int64_t)(k[u] < 0 ? 0 : kc) * ld_token + min(v, V - 1)];
      gv[u] = gb[min(v, V - 1)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {                          // a thread's columns in increasing order
      if (k[u] < 0) continue;
      const float4 s = sh_st[k[u]];
      const float p = expf(x[u] - s.x) / s.y;
      acc[k[u]][threadIdx.x] += (double)gv[u] * (double)p;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < nt; k += 4) {
    double s = ((acc[k][lane] + acc[k][lane + 64]) + acc[k][lane + 128]) + acc[k][lane + 192];
    s = wave_sum(s);
    if (lane == 0) {
      const float a = (float)s;
      A[b * T + t0 + k] = a;
      if (dw) dw[b * ld_dw + t0 + k] = sh_st[k].w * a;
    }
  }
}

// dL/dx of the whole [batch, skip + T, V] tensor.  logits / dx point at token 0 of the model's tensor.
template <typename TIN, bool VEC>
__global__ void __launch_bounds__(256) lexical_dx_kernel(const TIN* __restrict__ logits, int64_t ld_batch, int64_t ld_token, int skip, int T, int V,
                                                         const float4* __restrict__ stats, const float* __restrict__ A, const float* __restrict__ g,
                                                         int64_t ld_g, const int16_t* __restrict__ tok, int64_t ld_tok, TIN* __restrict__ dx,
                                                         int64_t ld_dbatch, int64_t ld_dtoken) {
  const int64_t b = blockIdx.z;
  const int l0 = blockIdx.y * DT;
  int c0 = (blockIdx.x * 256 + threadIdx.x) * DC;
  if (c0 >= V) return;
  if (VEC) c0 = min(c0, V - DC);       // the last thread of a row steps back to whole vectors (it rewrites up to DC - 1 columns with the same values)
  const int n = VEC ? DC : min(DC, V - c0);
  float gv[DC];
  int16_t tv[DC];
  load_cols<float, VEC>(g + b * ld_g + c0, n, gv);
  load_cols<int16_t, VEC>(tok + b * ld_tok + c0, n, tv);
  const TIN* xb = logits + b * ld_batch + c0;
  TIN* db = dx + b * ld_dbatch + c0;
  const int L = skip + T;
  bool all_live = l0 >= skip && l0 + DT <= L;
#pragma unroll
  for (int i = 0; i < DT; ++i) all_live = all_live && stats[b * T + (all_live ? l0 + i - skip : 0)].w != 0.f;
  auto row = [&](int l, const TIN (&x)[DC]) {
    const int t = l - skip;
    const float4 s = stats[b * T + t];
    const float coef = s.z * s.w, D = coef * A[b * T + t], inv = 1.f / s.y;
    TIN o[DC];
#pragma unroll
    for (int u = 0; u < DC; ++u) {
      const float p = expf((float)x[u] - s.x) * inv;
      o[u] = (TIN)(p * (((int)tv[u] == t ? gv[u] * coef : 0.f) - D));
    }
    store_cols<TIN, VEC>(db + (int64_t)l * ld_dtoken, n, o);
  };
  if (all_live) {                                        // the common tile: its rows are requested first and consumed afterwards
    TIN x[DT][DC];
#pragma unroll
    for (int i = 0; i < DT; ++i) load_cols<TIN, VEC>(xb + (int64_t)(l0 + i) * ld_token, n, x[i]);
#pragma unroll
    for (int i = 0; i < DT; ++i) row(l0 + i, x[i]);
    return;
  }
#pragma unroll 1
  for (int l = l0; l < min(l0 + DT, L); ++l) {
    TIN x[DC];
    if (l >= skip && stats[b * T + l - skip].w != 0.f) {
      load_cols<TIN, VEC>(xb + (int64_t)l * ld_token, n, x);
      row(l, x);
    } else {                                             // a skipped or masked token: zeros, the logits are not read
#pragma unroll
      for (int u = 0; u < DC; ++u) x[u] = (TIN)0.f;
      store_cols<TIN, VEC>(db + (int64_t)l * ld_dtoken, n, x);
    }
  }
}

// the checks the forward and the backward share: n_tokens counts the tokens after the skipped ones
int check_head(const void* logits, int32_t mem_kind, int32_t value_dtype, int64_t batch, int32_t n_tokens, int32_t skip_tokens, int32_t vocab,
               int64_t ld_batch, int64_t ld_token, const void* workspace, const char* what) {
  if (!logits || !workspace) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!val_ok_bf16(value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (batch < 0 || n_tokens <= 0 || vocab <= 0 || skip_tokens < 0 || skip_tokens > MAX_TOKENS || ld_token < vocab ||
      ld_batch < (int64_t)(n_tokens + skip_tokens - 1) * ld_token + vocab || batch * n_tokens > ((int64_t)1 << 31) - 1)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (n_tokens > MAX_TOKENS) return set_error(DHR_ERR_UNSUPPORTED, "more than 32767 tokens (the token index is int16)");
  if (mem_kind != DHR_MEM_DEVICE)
    return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": host arrays are not staged, training tensors live on the device (DHR_MEM_DEVICE)");
  return DHR_OK;
}

}  // namespace

extern "C" int64_t dhr_lexical_head_train_workspace(int64_t batch, int32_t n_tokens) try {
  if (batch <= 0 || n_tokens <= 0 || n_tokens > MAX_TOKENS || batch * n_tokens > ((int64_t)1 << 31) - 1) return 0;
  return batch * n_tokens * (int64_t)(sizeof(float4) + sizeof(float));     // (max, sum, w, m) per token, then A per token
} DHR_CATCH_VALUE(0)

extern "C" int dhr_lexical_head_train(int32_t device, int32_t mem_kind, const void* logits, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                                      int32_t skip_tokens, int32_t vocab, int64_t ld_batch, int64_t ld_token, const float* term_weights,
                                      int64_t ld_weights, const float* mask, int64_t ld_mask, float* out_reps, int64_t ld_reps, int16_t* out_tokens,
                                      int64_t ld_tokens, void* workspace, void* stream) try {
  dhr::alloc_checkpoint();
  if (!term_weights || !mask || !out_reps || !out_tokens) return set_error(DHR_ERR_INVALID, "null pointer");
  int rc = check_head(logits, mem_kind, value_dtype, batch, n_tokens, skip_tokens, vocab, ld_batch, ld_token, workspace, "dhr_lexical_head_train");
  if (rc) return rc;
  if (ld_weights < n_tokens || ld_mask < n_tokens || ld_reps < vocab || ld_tokens < vocab) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (batch == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int T = n_tokens;
  float4* stats = (float4*)workspace;
  const dim3 g_stats((unsigned)(batch * T)), g_fold((unsigned)((vocab + 511) / 512), (unsigned)std::min<int64_t>(batch, 65535));
  return with_value_type_bf16(value_dtype, [&](auto t) -> int {
    using TIN = typename decltype(t)::type;
    const TIN* x = (const TIN*)logits + (int64_t)skip_tokens * ld_token;
    hipLaunchKernelGGL(lexical_stats_kernel<TIN>, g_stats, dim3(256), 0, s, x, ld_batch, ld_token, T, vocab, term_weights, ld_weights, mask, ld_mask,
                       stats);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lexical_fold_tok_kernel<TIN>, g_fold, dim3(256), 0, s, x, ld_batch, ld_token, T, vocab, batch, (const float4*)stats, out_reps,
                       ld_reps, out_tokens, ld_tokens);
    HIP_TRY(hipGetLastError());
    return DHR_OK;
  });
} DHR_CATCH_STATUS

extern "C" int dhr_lexical_head_backward(int32_t device, int32_t mem_kind, const void* logits, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                                         int32_t skip_tokens, int32_t vocab, int64_t ld_batch, int64_t ld_token, const float* grad_reps,
                                         int64_t ld_grad_reps, const int16_t* tokens, int64_t ld_tokens, void* workspace, void* grad_logits,
                                         int64_t ld_grad_batch, int64_t ld_grad_token, float* grad_weights, int64_t ld_grad_weights,
                                         void* stream) try {
  dhr::alloc_checkpoint();
  if (!grad_reps || !tokens) return set_error(DHR_ERR_INVALID, "null pointer");
  int rc = check_head(logits, mem_kind, value_dtype, batch, n_tokens, skip_tokens, vocab, ld_batch, ld_token, workspace, "dhr_lexical_head_backward");
  if (rc) return rc;
  if (ld_grad_reps < vocab || ld_tokens < vocab || (grad_weights && ld_grad_weights < n_tokens) ||
      (grad_logits && (ld_grad_token < vocab || ld_grad_batch < (int64_t)(n_tokens + skip_tokens - 1) * ld_grad_token + vocab)))
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (batch == 0 || (!grad_logits && !grad_weights)) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int T = n_tokens, L = n_tokens + skip_tokens;
  const float4* stats = (const float4*)workspace;
  float* A = (float*)((char*)workspace + (size_t)batch * T * sizeof(float4));
  const int es = value_dtype == DHR_VAL_F32 ? 4 : 2;
  // multi-dword accesses need every row of the logits, of their gradient and of tok (and the stepped-back last vector) at a multiple of 4 bytes
  const bool vec = vocab >= DC && (int64_t)vocab * es % 4 == 0 &&
                   ((uintptr_t)logits | (uintptr_t)grad_logits | (uintptr_t)(ld_batch * es) | (uintptr_t)(ld_token * es) | (uintptr_t)(ld_grad_batch * es) |
                    (uintptr_t)(ld_grad_token * es) | (uintptr_t)tokens | (uintptr_t)(ld_tokens * 2)) % 4 == 0;
  const bool small = (int64_t)((T + RT_BIG - 1) / RT_BIG) * batch < 512;
  const int rt = small ? RT_SMALL : RT_BIG;
  for (int64_t lo = 0; lo < batch; lo += 65535) {           // (grid y / z limits)
    const int64_t rows = std::min<int64_t>(65535, batch - lo);
    const dim3 g_sum((unsigned)((T + rt - 1) / rt), (unsigned)rows);
    const dim3 g_dx((unsigned)((vocab + 256 * DC - 1) / (256 * DC)), (unsigned)((L + DT - 1) / DT), (unsigned)rows);
    rc = with_value_type_bf16(value_dtype, [&](auto t) -> int {
      using TIN = typename decltype(t)::type;
      const TIN* x = (const TIN*)logits + lo * ld_batch;
      with_int<RT_SMALL, RT_BIG>(rt, [&](auto r) {
        hipLaunchKernelGGL((lexical_route_sum_kernel<TIN, decltype(r)::value>), g_sum, dim3(256), 0, s, x + (int64_t)skip_tokens * ld_token, ld_batch,
                           ld_token, T, vocab, stats + lo * T, grad_reps + lo * ld_grad_reps, ld_grad_reps, tokens + lo * ld_tokens, ld_tokens,
                           A + lo * T, grad_weights ? grad_weights + lo * ld_grad_weights : nullptr, ld_grad_weights);
      });
      HIP_TRY(hipGetLastError());
      if (grad_logits) {
        TIN* d = (TIN*)grad_logits + lo * ld_grad_batch;
        with_flag(vec, [&](auto v) {
          hipLaunchKernelGGL((lexical_dx_kernel<TIN, decltype(v)::value>), g_dx, dim3(256), 0, s, x, ld_batch, ld_token, skip_tokens, T, vocab,
                             stats + lo * T, (const float*)A + lo * T, grad_reps + lo * ld_grad_reps, ld_grad_reps, tokens + lo * ld_tokens, ld_tokens,
                             d, ld_grad_batch, ld_grad_token);
        });
        HIP_TRY(hipGetLastError());
      }
      return DHR_OK;
    });
    if (rc) return rc;
  }
  return DHR_OK;
} DHR_CATCH_STATUS

// The loss of a training step and its gradient with respect to the score matrices, in one launch plus a row sum: the tail of
// tevatron/DHR/modeling.py:170-197, Aggretriever/modeling.py:184-213, ColBERT/modeling.py:146-160 and Dense/modeling.py:134-140.  The reference
// runs one fusion, three log_softmax, three scaled softmax of the teacher, three KLDivLoss(batchmean) and the weighted sum as some twenty small
// launches forward and more backward, with a dozen [R, C] temporaries kept for autograd.  Here, with fused = lexical + lamb * semantic and the
// target of term k either P_k = softmax(teacher * temperature * split[k]) or the one-hot at column r * label_stride:
//   loss = (1/R) sum_r [ w0 KL_r(fused, P_0) + w1 KL_r(semantic, P_1) + w2 KL_r(lexical, P_2) ],   KL_r(s, P) = sum_c P (log P - log_softmax(s))
//   train_loss_kernel      one 256-thread workgroup per row, a thread 4 consecutive columns per step (one 16-byte load of fp32, 8 bytes of fp16,
//                          where the base pointer and the row stride allow it; element by element otherwise).  Three passes over the row, which
//                          stays in the cache after the first: (A) the maxima of the three students and of the teacher, (B) with those, the sums
//                          of exponentials of the three students and the three targets (the targets share the teacher's maximum: the scales are
//                          positive), (C) softmax, log_softmax, P and log P = scaled teacher - logsumexp per element: fused scores, both gradients
//                          and the row's loss.  A term whose weight is zero is not computed.
//   train_loss_sum_kernel  one workgroup adds the R row losses in index order and writes loss = sum / R.
// exp and log are fp32, every exp has its maximum subtracted first (scores of magnitude 1e4 neither overflow nor give NaN).  Reductions are wave
// butterflies followed by the four wave results in wave order: no atomics, two runs on the same inputs are bit-identical.  Inputs must be finite.
#include "host_stage.h"

namespace {

constexpr int64_t MAX_ROWS = (int64_t)1 << 31, MAX_COLS = (int64_t)1 << 30;

struct Mat {
  const void* x;   // NULL: absent
  int64_t ld;
  int f32;         // else fp16
  int vec;         // 4 columns in one aligned load
};

struct Out {
  void* x;         // NULL: not wanted
  int64_t ld;
  int f32;
  int vec;
};

struct LossArgs {
  Mat lex, sem, tea;
  int C;
  int64_t label_stride;
  float lamb;
  float a[3];      // temperature * split[k]
  float w[3];      // weight of term k in the loss (0: the term is skipped)
  float gw[3];     // w[k] / R
  Out scores, glex, gsem;
  float* row_loss; // [R]
};

// columns c0 .. c0 + 3 of a row as floats; beyond C: `pad`
__device__ __forceinline__ float4 load4(const Mat& m, int64_t r, int c0, int C, float pad) {
  if (m.f32) {
    const float* row = (const float*)m.x + r * m.ld;
    if (m.vec && c0 + 4 <= C) return *reinterpret_cast<const float4*>(row + c0);
    return make_float4(c0 < C ? row[c0] : pad, c0 + 1 < C ? row[c0 + 1] : pad, c0 + 2 < C ? row[c0 + 2] : pad, c0 + 3 < C ? row[c0 + 3] : pad);
  }
  const _Float16* row = (const _Float16*)m.x + r * m.ld;
  if (m.vec && c0 + 4 <= C) {
    union { uint2 u; _Float16 h[4]; } v;
    v.u = *reinterpret_cast<const uint2*>(row + c0);
    return make_float4((float)v.h[0], (float)v.h[1], (float)v.h[2], (float)v.h[3]);
  }
  return make_float4(c0 < C ? (float)row[c0] : pad, c0 + 1 < C ? (float)row[c0 + 1] : pad, c0 + 2 < C ? (float)row[c0 + 2] : pad,
                     c0 + 3 < C ? (float)row[c0 + 3] : pad);
}

__device__ __forceinline__ void store4(const Out& o, int64_t r, int c0, int C, const float (&v)[4]) {
  if (o.f32) {
    float* row = (float*)o.x + r * o.ld;
    if (o.vec && c0 + 4 <= C) {
      *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
      return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + e < C) row[c0 + e] = v[e];
    return;
  }
  _Float16* row = (_Float16*)o.x + r * o.ld;
  if (o.vec && c0 + 4 <= C) {
    union { uint2 u; _Float16 h[4]; } p;
#pragma unroll
    for (int e = 0; e < 4; ++e) p.h[e] = (_Float16)v[e];
    *reinterpret_cast<uint2*>(row + c0) = p.u;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (c0 + e < C) row[c0 + e] = (_Float16)v[e];
}

// N values per thread -> the same N values in every thread: a butterfly within the wave (both partners add the same two numbers), then the four
// wave results in wave order.  `slot` is LDS of this reduction alone.
template <int N, bool MAX>
__device__ __forceinline__ void block_reduce(float (&v)[N], float (*slot)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float other = __shfl_xor(v[k], o, 64);
      v[k] = MAX ? fmaxf(v[k], other) : v[k] + other;
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) slot[wave][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float acc = slot[0][k];
#pragma unroll
    for (int w = 1; w < 4; ++w) acc = MAX ? fmaxf(acc, slot[w][k]) : acc + slot[w][k];
    v[k] = acc;
  }
}

__device__ __forceinline__ float at(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// grid: rows.  Student 0 is the fused score, 1 the semantic, 2 the lexical one; on[k]: term k has a weight (wave-uniform).
__global__ void __launch_bounds__(256) train_loss_kernel(LossArgs g) {
  __shared__ float s_max[4][4], s_sum[4][6], s_loss[4][1];
  const int64_t r = blockIdx.x;
  const int C = g.C;
  const bool has_sem = g.sem.x != nullptr, has_tea = g.tea.x != nullptr;
  const bool on[3] = {g.w[0] != 0.f, g.w[1] != 0.f, g.w[2] != 0.f};
  const float NEG = -INFINITY;

  // (A) maxima: students 0..2, teacher
  float mx[4] = {NEG, NEG, NEG, NEG};
  for (int c0 = threadIdx.x * 4; c0 < C; c0 += 1024) {
    const float4 l = load4(g.lex, r, c0, C, NEG);
    mx[2] = fmaxf(mx[2], fmaxf(fmaxf(l.x, l.y), fmaxf(l.z, l.w)));
    if (has_sem) {
      const float4 s = load4(g.sem, r, c0, C, NEG);
      mx[1] = fmaxf(mx[1], fmaxf(fmaxf(s.x, s.y), fmaxf(s.z, s.w)));
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < C) mx[0] = fmaxf(mx[0], fmaf(g.lamb, at(s, e), at(l, e)));
    }
    if (has_tea) {
      const float4 t = load4(g.tea, r, c0, C, NEG);
      mx[3] = fmaxf(mx[3], fmaxf(fmaxf(t.x, t.y), fmaxf(t.z, t.w)));
    }
  }
  block_reduce<4, true>(mx, s_max);
  if (!has_sem) mx[0] = mx[2];

  // (B) sums of exponentials: students 0..2, targets 0..2
  float z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c0 = threadIdx.x * 4; c0 < C; c0 += 1024) {
    const float4 l = load4(g.lex, r, c0, C, 0.f);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = s;
    if (has_sem) s = load4(g.sem, r, c0, C, 0.f);
    if (has_tea) t = load4(g.tea, r, c0, C, 0.f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e >= C) break;
      const float le = at(l, e), se = at(s, e);
      if (on[0]) z[0] += expf((has_sem ? fmaf(g.lamb, se, le) : le) - mx[0]);
      if (on[1]) z[1] += expf(se - mx[1]);
      if (on[2]) z[2] += expf(le - mx[2]);
      if (has_tea) {
        const float d = at(t, e) - mx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (on[k]) z[3 + k] += expf(g.a[k] * d);
      }
    }
  }
  block_reduce<6, false>(z, s_sum);
  float iz[6], lz[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const bool used = on[k % 3] && (k < 3 || has_tea);       // an unused sum is 0: keep its 1 / 0 and log 0 out of the arithmetic
    iz[k] = used ? 1.0f / z[k] : 0.f;
    lz[k] = used ? logf(z[k]) : 0.f;
  }

  // (C) per element: softmax and log_softmax of each student, P and log P of each target; outputs and the row's loss
  const int64_t label = has_tea ? -1 : r * g.label_stride;
  float loss[1] = {0.f};
  for (int c0 = threadIdx.x * 4; c0 < C; c0 += 1024) {
    const float4 l = load4(g.lex, r, c0, C, 0.f);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = s;
    if (has_sem) s = load4(g.sem, r, c0, C, 0.f);
    if (has_tea) t = load4(g.tea, r, c0, C, 0.f);
    float fused[4], gl[4], gs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      fused[e] = gl[e] = gs[e] = 0.f;
      if (c0 + e >= C) continue;
      const float le = at(l, e), se = at(s, e);
      fused[e] = has_sem ? fmaf(g.lamb, se, le) : le;
      const float st[3] = {fused[e], se, le};
      const float d = has_tea ? at(t, e) - mx[3] : 0.f;
      const bool hit = (int64_t)(c0 + e) == label;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (!on[k]) continue;
        const float x = st[k] - mx[k];
        const float q = expf(x) * iz[k], lsm = x - lz[k];
        float P;
        if (has_tea) {
          const float y = g.a[k] * d;
          P = expf(y) * iz[3 + k];
          loss[0] += g.w[k] * (P * ((y - lz[3 + k]) - lsm));
        } else {
          P = hit ? 1.f : 0.f;
          if (hit) loss[0] -= g.w[k] * lsm;
        }
        const float gk = g.gw[k] * (q - P);
        if (k == 0) { gl[e] += gk; gs[e] += g.lamb * gk; }
        else if (k == 1) gs[e] += gk;
        else gl[e] += gk;
      }
    }
    if (g.scores.x) store4(g.scores, r, c0, C, fused);
    if (g.glex.x) store4(g.glex, r, c0, C, gl);
    if (g.gsem.x) store4(g.gsem, r, c0, C, gs);
  }
  block_reduce<1, false>(loss, s_loss);
  if (threadIdx.x == 0) g.row_loss[r] = loss[0];
}

// one workgroup: the row losses in index order, 256 at a time through LDS
__global__ void __launch_bounds__(256) train_loss_sum_kernel(const float* row_loss, int64_t R, float* loss) {
  __shared__ float buf[256];
  float acc = 0.f;
  for (int64_t base = 0; base < R; base += 256) {
    const int64_t i = base + threadIdx.x;
    buf[threadIdx.x] = i < R ? row_loss[i] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = (int)std::min<int64_t>(256, R - base);
      for (int j = 0; j < n; ++j) acc += buf[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = acc / (float)R;
}

int vec_ok(const void* x, int64_t ld, int f32) {
  const int es = f32 ? 4 : 2;
  return (uintptr_t)x % (4 * es) == 0 && (ld * es) % (4 * es) == 0;
}

Mat make_mat(const void* x, int64_t ld, int dtype) {
  const int f32 = dtype == DHR_VAL_F32;
  return Mat{x, ld, f32, x ? vec_ok(x, ld, f32) : 0};
}

Out make_out(void* x, int64_t ld, int f32) { return Out{x, ld, f32, x ? vec_ok(x, ld, f32) : 0}; }

hipError_t launch(const LossArgs& a, int64_t R, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(train_loss_kernel, dim3((unsigned)R), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(train_loss_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)a.row_loss, R, loss);
  return hipGetLastError();
}

// a host [rows][cols] matrix with a row stride -> a packed device copy
hipError_t stage_mat(DevMem& m, Mat& a, int64_t rows, int64_t cols, hipStream_t s) {
  if (!a.x) return hipSuccess;
  const hipError_t e = stage_in(m, a.x, a.ld, rows, cols, a.f32 ? 4 : 2, s);
  a = Mat{m.p, cols, a.f32, vec_ok(m.p, cols, a.f32)};
  return e;
}

}  // namespace

extern "C" int64_t dhr_train_loss_workspace(int64_t rows) try {
  return rows > 0 && rows < MAX_ROWS ? rows * 4 : 0;
} DHR_CATCH_VALUE(0)

extern "C" int dhr_train_loss(int32_t device, int32_t mem_kind, const void* lexical, int32_t lexical_dtype, int64_t ld_lexical, const void* semantic,
                              int32_t semantic_dtype, int64_t ld_semantic, const void* teacher, int32_t teacher_dtype, int64_t ld_teacher,
                              int64_t rows, int64_t cols, int64_t label_stride, float lamb, float temperature, const float* weights,
                              const float* teacher_split, float* loss, float* scores_out, int64_t ld_scores, void* grad_lexical,
                              int64_t ld_grad_lexical, void* grad_semantic, int64_t ld_grad_semantic, void* workspace, int64_t workspace_bytes,
                              void* stream) try {
  dhr::alloc_checkpoint();
  if (!lexical || !loss || !weights) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (rows < 0 || cols < 0) return set_error(DHR_ERR_INVALID, "bad sizes");
  if (!val_ok(lexical_dtype) || (semantic && !val_ok(semantic_dtype)) || (teacher && !val_ok(teacher_dtype)))
    return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (ld_lexical < cols || (semantic && ld_semantic < cols) || (teacher && ld_teacher < cols) || (scores_out && ld_scores < cols) ||
      (grad_lexical && ld_grad_lexical < cols) || (grad_semantic && ld_grad_semantic < cols))
    return set_error(DHR_ERR_INVALID, "a row stride is shorter than a row of scores");
  if (!(lamb == lamb) || std::isinf(lamb) || !(weights[0] == weights[0]) || !(weights[1] == weights[1]) || !(weights[2] == weights[2]) ||
      std::isinf(weights[0]) || std::isinf(weights[1]) || std::isinf(weights[2]))
    return set_error(DHR_ERR_INVALID, "train loss: lamb and the weights must be finite");
  if (!semantic && weights[1] != 0.f) return set_error(DHR_ERR_INVALID, "train loss: the semantic term has a weight but there are no semantic scores");
  if (!semantic && grad_semantic) return set_error(DHR_ERR_INVALID, "train loss: a semantic gradient without semantic scores");
  if (teacher) {
    // the three targets share the teacher's row maximum, which needs positive scales
    if (!teacher_split) return set_error(DHR_ERR_INVALID, "null pointer");
    if (!(temperature > 0.f) || std::isinf(temperature)) return set_error(DHR_ERR_INVALID, "train loss: temperature must be positive and finite");
    for (int k = 0; k < 3; ++k)
      if (!(teacher_split[k] > 0.f) || std::isinf(teacher_split[k]))
        return set_error(DHR_ERR_INVALID, "train loss: every teacher split must be positive and finite");
  } else if (rows > 0 && cols > 0) {
    if (label_stride < 0 || (rows > 1 && label_stride > (cols - 1) / (rows - 1)))
      return set_error(DHR_ERR_INVALID, "train loss: label column " + std::to_string(rows - 1) + " x " + std::to_string(label_stride) + " is outside " +
                                            std::to_string(cols) + " columns");
  }
  if (rows >= MAX_ROWS || cols > MAX_COLS) return set_error(DHR_ERR_UNSUPPORTED, "train loss: more than 2^31 - 1 rows or 2^30 columns");
  hipStream_t s = (hipStream_t)stream;
  if (rows == 0 || cols == 0) {                          // loss 0, nothing else is touched
    if (mem_kind == DHR_MEM_HOST) { *loss = 0.f; return DHR_OK; }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemsetAsync(loss, 0, 4, s));
    return DHR_OK;
  }
  if (mem_kind == DHR_MEM_DEVICE && (!workspace || workspace_bytes < rows * 4))
    return set_error(DHR_ERR_INVALID, "train loss: device arrays need dhr_train_loss_workspace(rows) bytes of workspace");

  LossArgs a{};
  a.lex = make_mat(lexical, ld_lexical, lexical_dtype);
  a.sem = make_mat(semantic, ld_semantic, semantic_dtype);
  a.tea = make_mat(teacher, ld_teacher, teacher_dtype);
  a.C = (int)cols;
  a.label_stride = label_stride;
  a.lamb = semantic ? lamb : 0.f;
  for (int k = 0; k < 3; ++k) {
    a.a[k] = teacher ? (float)((double)temperature * (double)teacher_split[k]) : 0.f;
    a.w[k] = weights[k];
    a.gw[k] = (float)((double)weights[k] / (double)rows);
  }
  if (teacher)
    for (int k = 0; k < 3; ++k)
      if (!(a.a[k] > 0.f) || std::isinf(a.a[k])) return set_error(DHR_ERR_INVALID, "train loss: temperature x split must be positive and finite");
  HIP_TRY(hipSetDevice(device));
  if (mem_kind == DHR_MEM_DEVICE) {
    a.scores = make_out(scores_out, ld_scores, 1);
    a.glex = make_out(grad_lexical, ld_grad_lexical, a.lex.f32);
    a.gsem = make_out(grad_semantic, ld_grad_semantic, a.sem.f32);
    a.row_loss = (float*)workspace;
    HIP_TRY(launch(a, rows, loss, s));
    return DHR_OK;
  }
  DevMem m_lex, m_sem, m_tea, m_scores, m_glex, m_gsem, m_ws;
  HIP_TRY(stage_mat(m_lex, a.lex, rows, cols, s));
  HIP_TRY(stage_mat(m_sem, a.sem, rows, cols, s));
  HIP_TRY(stage_mat(m_tea, a.tea, rows, cols, s));
  const int les = a.lex.f32 ? 4 : 2, ses = a.sem.f32 ? 4 : 2;
  if (scores_out) HIP_TRY(dev_alloc(m_scores, rows * cols * 4));
  if (grad_lexical) HIP_TRY(dev_alloc(m_glex, rows * cols * les));
  if (grad_semantic) HIP_TRY(dev_alloc(m_gsem, rows * cols * ses));
  HIP_TRY(dev_alloc(m_ws, rows * 4 + 4));
  a.scores = make_out(m_scores.p, cols, 1);
  a.glex = make_out(m_glex.p, cols, a.lex.f32);
  a.gsem = make_out(m_gsem.p, cols, a.sem.f32);
  a.row_loss = (float*)m_ws.p;
  float* d_loss = (float*)m_ws.p + rows;
  HIP_TRY(launch(a, rows, d_loss, s));
  HIP_TRY(hipMemcpyAsync(loss, d_loss, 4, hipMemcpyDeviceToHost, s));
  if (scores_out) HIP_TRY(stage_out(scores_out, ld_scores, m_scores.p, rows, cols, 4, s));
  if (grad_lexical) HIP_TRY(stage_out(grad_lexical, ld_grad_lexical, m_glex.p, rows, cols, les, s));
  if (grad_semantic) HIP_TRY(stage_out(grad_semantic, ld_grad_semantic, m_gsem.p, rows, cols, ses, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

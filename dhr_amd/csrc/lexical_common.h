// What the two translation units of the lexical head share (lexical.hip: encoding, lexical_train.hip: training): the 16-byte row walk and
// lexical_stats_kernel, the per-token softmax statistics.  One definition, so the training forward is bit-identical to the encoding one.
#pragma once
#include "dhr_state.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

template <typename TIN> struct Vec;
template <> struct Vec<_Float16> { typedef half8 type; static constexpr int n = 8; };
template <> struct Vec<float> { typedef float4 type; static constexpr int n = 4; };

// f(v) for every element of x[0, n): a scalar head up to the first 16-byte boundary, 16-byte vector loads, a scalar tail
template <typename TIN, typename F>
__device__ __forceinline__ void row_for_each(const TIN* __restrict__ x, int n, F&& f) {
  constexpr int VN = Vec<TIN>::n;
  const int head = min(n, (int)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(TIN)));
  if ((int)threadIdx.x < head) f((float)x[threadIdx.x]);
  const int n_vec = (n - head) / VN;
  const typename Vec<TIN>::type* xv = reinterpret_cast<const typename Vec<TIN>::type*>(x + head);
#pragma unroll 4
  for (int i = threadIdx.x; i < n_vec; i += 256) {
    const typename Vec<TIN>::type v = xv[i];
#pragma unroll
    for (int u = 0; u < VN; ++u) f((float)v[u]);
  }
  const int tail = head + n_vec * VN;
  if (tail + (int)threadIdx.x < n) f((float)x[tail + threadIdx.x]);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename TIN>
__global__ void __launch_bounds__(256) lexical_stats_kernel(const TIN* __restrict__ logits, int64_t ld_batch, int64_t ld_token, int T, int V,
                                                            const float* __restrict__ w, int64_t ld_w, const float* __restrict__ mk, int64_t ld_m,
                                                            float4* __restrict__ stats) {
  __shared__ float red[4];
  __shared__ double red_d[4];
  const int64_t row = blockIdx.x;
  const int64_t b = row / T;
  const int t = (int)(row - b * T);
  const float wt = w[b * ld_w + t], mt = mk[b * ld_m + t];
  if (mt == 0.f) {                                  // a masked token: its logits never take part (lexical_fold_kernel folds (0 * w) * 0)
    if (threadIdx.x == 0) stats[row] = make_float4(0.f, 1.f, wt, mt);
    return;
  }
  const TIN* x = logits + b * ld_batch + (int64_t)t * ld_token;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -INFINITY;
  row_for_each(x, V, [&](float v) { m = fmaxf(m, v); });
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  double s = 0.0;                                   // the normaliser is accumulated in fp64: fp32 rounded once, whatever the summation order
  row_for_each(x, V, [&](float v) { s += (double)expf(v - m); });
  s = wave_sum(s);
  if (lane == 0) red_d[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) stats[row] = make_float4(m, (float)((red_d[0] + red_d[1]) + (red_d[2] + red_d[3])), wt, mt);
}

}  // namespace

// What the translation units of the lexical head share (lexical.hip: encoding, lexical_train.hip: training, aggretriever_train.hip: the
// Aggretriever training ops): the 16-byte row walk and lexical_stats_kernel, the per-token softmax statistics; the geometry of the grouped
// views and the signed fold of aggregate(full); the 4-byte-aligned column vectors of the streaming passes; check_record, the record rules of
// the two encoding heads (lexical.hip, lexical_proj.hip).  One definition each, so the training forwards are bit-identical to the encoding ones.
#pragma once
#include "host_stage.h"

namespace dhr {
// lexical.hip: its record epilogues (lexical_fold_kernel without statistics, lexical_cls_kernel) on fp32 reps [batch, vocab] (row stride
// ld_reps) that the caller computed on the device: raw / densify / aggregate into the record's value and index rows, then the [CLS] columns
// at out_cols.  reps == NULL: the reps already are the fp32 value rows (raw), only the [CLS] columns are written.  Enqueues on s.
hipError_t lexical_record_from_reps(const float* reps, int64_t ld_reps, int mode, int64_t batch, int vocab, int out_cols, int W, int n_groups,
                                    int remove, void* out_val, int val_f32, int64_t ld_val, void* out_idx, int idx_i16, int64_t ld_idx,
                                    const void* cls, int cls_f32, int64_t ld_cls, int cls_dim, hipStream_t s);
}  // namespace dhr

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename TIN> struct Vec;
template <> struct Vec<_Float16> { typedef half8 type; static constexpr int n = 8; };
template <> struct Vec<__bf16> { typedef bf16x8 type; static constexpr int n = 8; };
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

// two adjacent columns of a row as one load
template <typename TIN> struct Pair;
template <> struct Pair<_Float16> { typedef _Float16 type __attribute__((ext_vector_type(2))); };
template <> struct Pair<__bf16> { typedef __bf16 type __attribute__((ext_vector_type(2))); };
template <> struct Pair<float> { typedef float type __attribute__((ext_vector_type(2))); };

template <typename T_, int N> struct VecA4;     // N elements, aligned to 4 bytes (what a multi-dword global access needs)
template <int N> struct VecA4<_Float16, N> { typedef _Float16 type __attribute__((ext_vector_type(N), aligned(4))); };
template <int N> struct VecA4<__bf16, N> { typedef __bf16 type __attribute__((ext_vector_type(N), aligned(4))); };
template <int N> struct VecA4<float, N> { typedef float type __attribute__((ext_vector_type(N), aligned(4))); };
template <int N> struct VecA4<int16_t, N> { typedef int16_t type __attribute__((ext_vector_type(N), aligned(4))); };

// N adjacent columns of a row: one multi-dword access where VEC and all N are inside the row, element-wise otherwise
template <typename T_, bool VEC, int N>
__device__ __forceinline__ void load_cols(const T_* __restrict__ p, int n, T_ (&out)[N]) {
  if (VEC && n == N) {
    const typename VecA4<T_, N>::type v = *reinterpret_cast<const typename VecA4<T_, N>::type*>(p);
#pragma unroll
    for (int u = 0; u < N; ++u) out[u] = v[u];
  } else {
#pragma unroll
    for (int u = 0; u < N; ++u) out[u] = u < n ? p[u] : (T_)0;
  }
}
template <typename T_, bool VEC, int N>
__device__ __forceinline__ void store_cols(T_* __restrict__ p, int n, const T_ (&in)[N]) {
  if (VEC && n == N) {
    typename VecA4<T_, N>::type v;
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = in[u];
    *reinterpret_cast<typename VecA4<T_, N>::type*>(p) = v;
  } else {
#pragma unroll
    for (int u = 0; u < N; ++u)
      if (u < n) p[u] = in[u];
  }
}

// aggregate(full) of tevatron/Aggretriever/utils.py:32-37 on the maxima of an even / odd column pair, with its signs of zero
__device__ __forceinline__ float agg_full_value(float pos, float neg) {
#pragma clang fp contract(off)
  return pos * (float)(pos > neg) - neg * (float)(pos <= neg);
}

enum { MODE_RAW = 0, MODE_DENSIFY = 1, MODE_AGG_FULL = 2, MODE_AGG_SEMI = 3 };

struct Geometry {
  int out_cols, W, n_groups, remove;
};

// validates mode / dims / remove against the vocabulary; the geometry of the view the epilogue folds
inline int geometry(int mode, int vocab, int dims, int remove, Geometry& g) {
  if (mode == MODE_RAW) { g = {vocab, vocab, 1, 0}; return DHR_OK; }
  if (mode != MODE_DENSIFY && mode != MODE_AGG_FULL && mode != MODE_AGG_SEMI) return set_error(DHR_ERR_INVALID, "bad lexical mode");
  if (dims <= 0) return set_error(DHR_ERR_INVALID, "dims must be > 0");
  if (mode == MODE_AGG_FULL && dims > (1 << 29)) return set_error(DHR_ERR_INVALID, "dims too large");
  const int64_t W = mode == MODE_AGG_FULL ? 2 * (int64_t)dims : dims;
  if (remove < 0 && mode != MODE_AGG_FULL) return set_error(DHR_ERR_INVALID, "remove_dims must be >= 0 (negative values pad, aggregate(full) only)");
  const int64_t cols = remove >= 0 ? (int64_t)vocab - remove : (int64_t)vocab - (int64_t)remove;
  if (cols <= 0 || cols % W != 0) {
    if (mode == MODE_DENSIFY) return set_error(DHR_ERR_INVALID, "Input lexical representation cannot be densified, please fix dims or remove_dims");
    return set_error(DHR_ERR_INVALID, "the vocabulary after remove_dims is not a whole number of groups");
  }
  if (cols / W > 32767) return set_error(DHR_ERR_UNSUPPORTED, "more than 32767 groups");
  g = {dims, (int)W, (int)(cols / W), remove};
  return DHR_OK;
}

// The record rules of the encoding heads (dhr_lexical_head, dhr_lexical_proj_head): geometry() first, then the value rows with their [CLS]
// columns, then -- densify alone -- the index rows.  Fills g.
inline int check_record(int mode, int vocab, int dims, int remove, int64_t ld_value, const void* out_index, int index_dtype, int64_t ld_index,
                        const void* cls, int cls_dtype, int64_t ld_cls, int cls_dim, Geometry& g) {
  if (int rc = geometry(mode, vocab, dims, remove, g)) return rc;
  if (ld_value < (int64_t)g.out_cols + cls_dim) return set_error(DHR_ERR_INVALID, "ld_value is smaller than the record's columns");
  if (cls_dim > 0 && (!cls || !val_ok(cls_dtype) || ld_cls < cls_dim)) return set_error(DHR_ERR_INVALID, "bad cls reps");
  if (mode != MODE_DENSIFY) return DHR_OK;
  if (!out_index) return set_error(DHR_ERR_INVALID, "null index pointer");
  if (index_dtype != DHR_IDX_U8 && index_dtype != DHR_IDX_I16) return set_error(DHR_ERR_INVALID, "index dtype must be uint8 or int16");
  if (index_dtype == DHR_IDX_U8 && g.n_groups > 256) return set_error(DHR_ERR_UNSUPPORTED, "more than 256 groups need the int16 index dtype");
  if (ld_index < g.out_cols) return set_error(DHR_ERR_INVALID, "ld_index < dims");
  return DHR_OK;
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

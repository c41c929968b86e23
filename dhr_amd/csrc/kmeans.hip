// k-means over whole fp16 rows with thousands of centroids (dhr_kmeans_assign, dhr_kmeans_update, dhr_kmeans): the clustering behind the
// query-cluster files of topic-aware sampling (tevatron/data.py:205-215).  DESIGN.md section 4n.
//   kmeans_split_kernel    once per round: every fp32 centroid c -> two fp16 images, hi = fp16(c) (0 where that would be subnormal) and
//                          lo = fp16((c - hi) * 2^11), rows padded to 128 columns and to 32 centroids with zeros, and h[j] = 1/2 |c_j|^2
//                          summed in float64 in a fixed tree and rounded once.
//   kmeans_assign_kernel   a workgroup owns 128 rows, a wave 32 of them: the wave's row block is the B operand of v_mfma_f32_32x32x16_f16 (in
//                          registers for d <= 128, re-read per 128-column chunk beyond), tiles of 32 centroids x 128 columns of both images go
//                          through LDS (rows padded to 272 bytes, as in maxsim.hip) as the A operand, hi and lo into an accumulator each, both
//                          kept across the K loop over the chunks.  Every product is exact in fp32.  A lane then holds one row against 16
//                          centroids: t = acc_hi + 2^-11 acc_lo - h[j], running (t, j) with strict > in increasing j, the two lane halves merged
//                          with the lower j winning a tie: the answer does not depend on the tiling.  No [n, K] array exists anywhere.
//   update                 stable radix sort of (assign, row) (hipCUB), segment starts by binary search, then one thread per (centroid, column)
//                          adds its members in increasing row order in fp32 and divides once.  No atomics.  An empty cluster keeps its centroid.
//   kmeans_stats_kernel    objective (float64, fixed order) and the number of changed rows of a round, one workgroup.
// Every output is a function of the arguments alone: two calls give the same bits.
#include <hipcub/hipcub.hpp>

#include "host_stage.h"
#include "op_dispatch.h"

namespace {

constexpr int KC = 128;                    // columns per chunk: 256 bytes of fp16
constexpr int ROW_PITCH = 256 + 16;        // LDS pitch of a centroid row of one chunk
constexpr int TILE = 32;                   // centroids per tile, rows per wave
constexpr int WG_ROWS = 4 * TILE;
constexpr int MAX_D = 4096, MAX_K = 65536;
constexpr float LO_SCALE = 2048.f, LO_UNSCALE = 1.f / 2048.f;
constexpr float F16_MIN_NORMAL = 6.103515625e-05f;
constexpr int STATS_THREADS = 1024;

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

struct AssignArgs {
  const _Float16* x;
  int64_t ld, n;
  int d, K, n_chunks, n_tiles, d_pad;
  const _Float16 *chi, *clo;   // [K_pad][d_pad]
  const float* half_norm;      // [K_pad]
  int32_t* assign;
  float* dist;                 // or NULL
};

// grid: K_pad centroids.  (c - hi is exact in fp32: hi is c rounded to 11 bits, or 0.)
__global__ void __launch_bounds__(256) kmeans_split_kernel(const float* __restrict__ c, int K, int d, int d_pad, _Float16* __restrict__ chi,
                                                           _Float16* __restrict__ clo, float* __restrict__ half_norm) {
  __shared__ double part[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int col = tid; col < d_pad; col += 256) {
    const float v = j < K && col < d ? c[(int64_t)j * d + col] : 0.f;
    _Float16 hi = (_Float16)v;
    if (fabsf((float)hi) < F16_MIN_NORMAL) hi = (_Float16)0.f;
    chi[(int64_t)j * d_pad + col] = hi;
    clo[(int64_t)j * d_pad + col] = (_Float16)((v - (float)hi) * LO_SCALE);
    s += (double)v * (double)v;
  }
  part[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) half_norm[j] = (float)(0.5 * part[0]);
}

// 8 fp16 of a row starting at col0: one aligned load, or element by element with zeros beyond d
template <bool VEC>
__device__ __forceinline__ uint4 load8(const _Float16* row, int col0, int d) {
  if (VEC && col0 + 8 <= d) return *reinterpret_cast<const uint4*>(row + col0);
  half8 f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = col0 + e < d ? row[col0 + e] : (_Float16)0.f;
  return __builtin_bit_cast(uint4, f);
}

__device__ __forceinline__ float sum_squares(const uint4 (&f)[8], float s) {
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const half8 a = __builtin_bit_cast(half8, f[v]);
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf((float)a[e], (float)a[e], s);
  }
  return s;
}

// grid: blocks of 128 rows.  VEC: rows may be read 16 bytes at a time; MULTI: d spans more than one chunk.
template <bool VEC, bool MULTI>
__global__ void __launch_bounds__(256) kmeans_assign_kernel(AssignArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[2 * TILE * ROW_PITCH];   // the hi image, then the lo image
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t i = (int64_t)blockIdx.x * WG_ROWS + wave * TILE + r;
  const bool real = i < g.n;
  const _Float16* row = g.x + (real ? i : 0) * g.ld;
  const int d = g.d, d_pad = g.d_pad, n_chunks = g.n_chunks, K = g.K;
  const _Float16 *chi = g.chi, *clo = g.clo;
  const float* half_norm = g.half_norm;
  // staging: thread t moves slot t & 15 of rows t >> 4 and 16 + (t >> 4) of both images of a step
  const int st_row = threadIdx.x >> 4, st_slot = threadIdx.x & 15;
  uint4 st_hi0, st_hi1, st_lo0, st_lo1;
  auto fetch = [&](int j0, int chunk) {
    const int64_t at = (int64_t)(j0 + st_row) * d_pad + chunk * KC + st_slot * 8;
    st_hi0 = *reinterpret_cast<const uint4*>(chi + at);
    st_hi1 = *reinterpret_cast<const uint4*>(chi + at + (int64_t)16 * d_pad);
    st_lo0 = *reinterpret_cast<const uint4*>(clo + at);
    st_lo1 = *reinterpret_cast<const uint4*>(clo + at + (int64_t)16 * d_pad);
  };
  uint4 xf[8];
  auto load_x = [&](int chunk) {
#pragma unroll
    for (int v = 0; v < 8; ++v) xf[v] = real ? load8<VEC>(row, chunk * KC + (2 * v + h) * 8, d) : make_uint4(0u, 0u, 0u, 0u);
  };
  float norm = 0.f;
  if constexpr (!MULTI) {
    load_x(0);
    norm = sum_squares(xf, norm);
  }
  float best_v = -INFINITY;
  int best_j = 0;
  float16v acc_hi, acc_lo;
  const int n_steps = g.n_tiles * n_chunks;
  fetch(0, 0);
  for (int step = 0; step < n_steps; ++step) {
    const int j0 = (step / n_chunks) * TILE, chunk = step % n_chunks;
    unsigned char* dst = tile + st_row * ROW_PITCH + st_slot * 16;
    *reinterpret_cast<uint4*>(dst) = st_hi0;
    *reinterpret_cast<uint4*>(dst + 16 * ROW_PITCH) = st_hi1;
    *reinterpret_cast<uint4*>(dst + TILE * ROW_PITCH) = st_lo0;
    *reinterpret_cast<uint4*>(dst + (TILE + 16) * ROW_PITCH) = st_lo1;
    __syncthreads();
    if (step + 1 < n_steps) fetch(((step + 1) / n_chunks) * TILE, (step + 1) % n_chunks);
    if (chunk == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) { acc_hi[k] = 0.f; acc_lo[k] = 0.f; }
    }
    if constexpr (MULTI) {
      load_x(chunk);
      if (step < n_chunks) norm = sum_squares(xf, norm);      // the first tile's pass over the row
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const half8 b = __builtin_bit_cast(half8, xf[v]);
      const half8 a_hi = *reinterpret_cast<const half8*>(tile + r * ROW_PITCH + (2 * v + h) * 16);
      const half8 a_lo = *reinterpret_cast<const half8*>(tile + TILE * ROW_PITCH + r * ROW_PITCH + (2 * v + h) * 16);
      acc_hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b, acc_hi, 0, 0, 0);
      acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b, acc_lo, 0, 0, 0);
    }
#endif
    if (chunk == n_chunks - 1) {
      // this lane: row i against centroids j0 + 4h + (k & 3) + 8 (k >> 2), increasing in k: strict > keeps the lowest j of equal values
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int jq = j0 + 4 * h + 8 * q;
        typedef float float4v __attribute__((ext_vector_type(4)));
        const float4v hn = *reinterpret_cast<const float4v*>(half_norm + jq);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = fmaf(acc_lo[4 * q + e], LO_UNSCALE, acc_hi[4 * q + e]) - hn[e];
          if (jq + e < K && t > best_v) { best_v = t; best_j = jq + e; }       // (the padded centroids of the last tile never win)
        }
      }
    }
    __syncthreads();
  }
  // the two lane halves hold interleaved centroids of the same row
  const float ov = __shfl_xor(best_v, 32, 64);
  const int oj = __shfl_xor(best_j, 32, 64);
  if (ov > best_v || (ov == best_v && oj < best_j)) { best_v = ov; best_j = oj; }
  norm += __shfl_xor(norm, 32, 64);
  if (real && h == 0) {
    g.assign[i] = best_j;
    if (g.dist) g.dist[i] = norm - 2.f * best_v;
  }
}

// ---- update
// sort key of row i: its cluster, or K for an entry outside [0, K) (such rows join no cluster)
__global__ void __launch_bounds__(256) kmeans_keys_kernel(const int32_t* __restrict__ assign, int64_t n, int K, uint32_t* __restrict__ keys,
                                                          int32_t* __restrict__ rows) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t a = (uint32_t)assign[i];
    keys[i] = a < (uint32_t)K ? a : (uint32_t)K;
    rows[i] = (int32_t)i;
  }
}

// start[j] = first position of the sorted keys with key >= j, j in [0, K]
__global__ void __launch_bounds__(256) kmeans_starts_kernel(const uint32_t* __restrict__ keys, int64_t n, int K, int32_t* __restrict__ start) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > K) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < (uint32_t)j) lo = mid + 1; else hi = mid;
  }
  start[j] = (int32_t)lo;
}

__global__ void __launch_bounds__(256) kmeans_counts_kernel(const int32_t* __restrict__ start, int K, int64_t* __restrict__ counts) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < K) counts[j] = (int64_t)start[j + 1] - start[j];
}

// grid: (centroid j, block of 256 columns).  The members of j are rows[start[j] .. start[j + 1]), increasing.
__global__ void __launch_bounds__(256) kmeans_mean_kernel(const _Float16* __restrict__ x, int64_t ld, int d, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ start, float* __restrict__ centroids) {
  const int j = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
  const int lo = start[j], hi = start[j + 1];
  if (col >= d || hi == lo) return;                       // an empty cluster keeps its centroid
  float s = 0.f;
  int m = lo;
  for (; m + 4 <= hi; m += 4) {                           // four gathers in flight, added in row order
    const float v0 = (float)x[(int64_t)rows[m] * ld + col], v1 = (float)x[(int64_t)rows[m + 1] * ld + col];
    const float v2 = (float)x[(int64_t)rows[m + 2] * ld + col], v3 = (float)x[(int64_t)rows[m + 3] * ld + col];
    s += v0; s += v1; s += v2; s += v3;
  }
  for (; m < hi; ++m) s += (float)x[(int64_t)rows[m] * ld + col];
  centroids[(int64_t)j * d + col] = __fdiv_rn(s, (float)(hi - lo));
}

// one workgroup: objective = sum of dist (float64: a thread adds its strided elements in order, then a fixed tree), changed = rows whose
// assignment differs from prev (all of them in the first round); prev <- assign
__global__ void __launch_bounds__(STATS_THREADS) kmeans_stats_kernel(const float* __restrict__ dist, const int32_t* __restrict__ assign,
                                                                     int32_t* __restrict__ prev, int64_t n, int first, double* __restrict__ objective,
                                                                     int64_t* __restrict__ changed) {
  __shared__ double part[STATS_THREADS];
  __shared__ int64_t moved[STATS_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  int64_t c = 0;
  for (int64_t i = tid; i < n; i += STATS_THREADS) {
    s += (double)dist[i];
    const int32_t a = assign[i];
    c += first || a != prev[i];
    prev[i] = a;
  }
  part[tid] = s;
  moved[tid] = c;
  __syncthreads();
  for (int o = STATS_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { part[tid] += part[tid + o]; moved[tid] += moved[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { *objective = part[0]; *changed = moved[0]; }
}

// ---- host side
int64_t up(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
int key_bits(int K) { int b = 1; while (((int64_t)1 << b) <= K) ++b; return b; }

// Stream-ordered scratch of a call on device arrays (nothing waits); a call on host arrays synchronises before it returns, so the same serves it.
struct Scratch {
  char* p = nullptr;
  hipStream_t s = nullptr;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { if (p) (void)hipFreeAsync(p, s); }
  hipError_t alloc(int64_t bytes, hipStream_t stream) { s = stream; return hipMallocAsync((void**)&p, (size_t)std::max<int64_t>(bytes, 256), stream); }
};

struct Layout {
  int64_t n;
  int d, K, d_pad, K_pad;
  // byte offsets
  int64_t chi, clo, half_norm, keys, keys2, rows, rows2, start, sort_tmp, dist, prev, total;
  size_t sort_bytes;
};

hipError_t sort_pairs(void* tmp, size_t& bytes, const uint32_t* k_in, uint32_t* k_out, const int32_t* v_in, int32_t* v_out, int64_t n, int K, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, (int)n, 0, key_bits(K), s);
}

// what: 1 = assignment, 2 = update, 4 = the per-round arrays of dhr_kmeans
hipError_t make_layout(int64_t n, int d, int K, int what, Layout& l) {
  l.n = n; l.d = d; l.K = K;
  l.d_pad = (d + KC - 1) / KC * KC;
  l.K_pad = (K + TILE - 1) / TILE * TILE;
  int64_t at = 0;
  auto take = [&](int64_t bytes, bool on) { const int64_t o = at; if (on) at += up(bytes); return o; };
  l.chi = take((int64_t)l.K_pad * l.d_pad * 2, what & 1);
  l.clo = take((int64_t)l.K_pad * l.d_pad * 2, what & 1);
  l.half_norm = take((int64_t)l.K_pad * 4, what & 1);
  l.sort_bytes = 0;
  if (what & 2) {
    const hipError_t e = sort_pairs(nullptr, l.sort_bytes, nullptr, nullptr, nullptr, nullptr, n, K, nullptr);
    if (e != hipSuccess) return e;
  }
  l.keys = take(n * 4, what & 2);
  l.keys2 = take(n * 4, what & 2);
  l.rows = take(n * 4, what & 2);
  l.rows2 = take(n * 4, what & 2);
  l.start = take((int64_t)(K + 1) * 4, what & 2);
  l.sort_tmp = take((int64_t)l.sort_bytes, what & 2);
  l.dist = take(n * 4, what & 4);
  l.prev = take(n * 4, what & 4);
  l.total = at;
  return hipSuccess;
}

bool vec_ok(const void* x, int64_t ld) { return (uintptr_t)x % 16 == 0 && (ld * 2) % 16 == 0; }

hipError_t launch_assign(const Layout& l, char* ws, const _Float16* x, int64_t ld, const float* centroids, int32_t* assign, float* dist, hipStream_t s) {
  _Float16 *chi = (_Float16*)(ws + l.chi), *clo = (_Float16*)(ws + l.clo);
  float* hn = (float*)(ws + l.half_norm);
  hipLaunchKernelGGL(kmeans_split_kernel, dim3((unsigned)l.K_pad), dim3(256), 0, s, centroids, l.K, l.d, l.d_pad, chi, clo, hn);
  AssignArgs a{x, ld, l.n, l.d, l.K, l.d_pad / KC, l.K_pad / TILE, l.d_pad, chi, clo, hn, assign, dist};
  const dim3 grid((unsigned)((l.n + WG_ROWS - 1) / WG_ROWS));
  with_flag(vec_ok(x, ld), [&](auto v) { with_flag(a.n_chunks > 1, [&](auto m) {
    hipLaunchKernelGGL((kmeans_assign_kernel<decltype(v)::value, decltype(m)::value>), grid, dim3(256), 0, s, a);
  }); });
  return hipGetLastError();
}

// the member order of every cluster: rows2 sorted by (assign, row), start[j] the first member of cluster j
hipError_t launch_segments(const Layout& l, char* ws, const int32_t* assign, hipStream_t s) {
  uint32_t *keys = (uint32_t*)(ws + l.keys), *keys2 = (uint32_t*)(ws + l.keys2);
  int32_t *rows = (int32_t*)(ws + l.rows), *rows2 = (int32_t*)(ws + l.rows2), *start = (int32_t*)(ws + l.start);
  const unsigned blocks = (unsigned)std::min<int64_t>((l.n + 255) / 256, 65536);
  hipLaunchKernelGGL(kmeans_keys_kernel, dim3(blocks), dim3(256), 0, s, assign, l.n, l.K, keys, rows);
  size_t bytes = l.sort_bytes;
  const hipError_t e = sort_pairs(ws + l.sort_tmp, bytes, keys, keys2, rows, rows2, l.n, l.K, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kmeans_starts_kernel, dim3((unsigned)(l.K / 256 + 1)), dim3(256), 0, s, (const uint32_t*)keys2, l.n, l.K, start);
  return hipGetLastError();
}

hipError_t launch_counts(const Layout& l, char* ws, int64_t* counts, hipStream_t s) {
  hipLaunchKernelGGL(kmeans_counts_kernel, dim3((unsigned)((l.K + 255) / 256)), dim3(256), 0, s, (const int32_t*)(ws + l.start), l.K, counts);
  return hipGetLastError();
}

hipError_t launch_update(const Layout& l, char* ws, const _Float16* x, int64_t ld, const int32_t* assign, float* centroids, int64_t* counts, hipStream_t s) {
  hipError_t e = launch_segments(l, ws, assign, s);
  if (e != hipSuccess) return e;
  if ((e = launch_counts(l, ws, counts, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(kmeans_mean_kernel, dim3((unsigned)l.K, (unsigned)((l.d + 255) / 256)), dim3(256), 0, s, x, ld, l.d, (const int32_t*)(ws + l.rows2),
                     (const int32_t*)(ws + l.start), centroids);
  return hipGetLastError();
}

int check_rows(int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t K) {
  if (!values) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (n < 1 || n >= ((int64_t)1 << 31)) return set_error(DHR_ERR_INVALID, "kmeans: n must be in [1, 2^31), got " + std::to_string(n));
  if (d < 1 || d > MAX_D) return set_error(DHR_ERR_INVALID, "kmeans: d must be in [1, 4096], got " + std::to_string(d));
  if (K < 1 || K > MAX_K) return set_error(DHR_ERR_INVALID, "kmeans: K must be in [1, 65536], got " + std::to_string(K));
  if (ld < d) return set_error(DHR_ERR_INVALID, "kmeans: ld is shorter than a row of d values");
  return DHR_OK;
}

}  // namespace

extern "C" int dhr_kmeans_assign(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, const float* centroids, int32_t K,
                                 int32_t* assign, float* dist, void* stream) try {
  dhr::alloc_checkpoint();
  if (!centroids || !assign) return set_error(DHR_ERR_INVALID, "null pointer");
  if (int rc = check_rows(mem_kind, values, ld, n, d, K)) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  Layout l;
  HIP_TRY(make_layout(n, d, K, 1, l));
  Scratch ws;
  HIP_TRY(ws.alloc(l.total, s));
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_assign(l, ws.p, (const _Float16*)values, ld, centroids, assign, dist, s));
    return DHR_OK;
  }
  DevMem m_x, m_c, m_a, m_d;
  HIP_TRY(stage_in(m_x, values, ld, n, d, 2, s));
  HIP_TRY(stage_in(m_c, centroids, (size_t)K * d * 4, s));
  HIP_TRY(dev_alloc(m_a, n * 4));
  if (dist) HIP_TRY(dev_alloc(m_d, n * 4));
  HIP_TRY(launch_assign(l, ws.p, (const _Float16*)m_x.p, d, (const float*)m_c.p, (int32_t*)m_a.p, (float*)m_d.p, s));
  HIP_TRY(stage_out(assign, m_a.p, (size_t)n * 4, s));
  if (dist) HIP_TRY(stage_out(dist, m_d.p, (size_t)n * 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_kmeans_update(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, const int32_t* assign, int32_t K,
                                 float* centroids, int64_t* counts, void* stream) try {
  dhr::alloc_checkpoint();
  if (!assign || !centroids || !counts) return set_error(DHR_ERR_INVALID, "null pointer");
  if (int rc = check_rows(mem_kind, values, ld, n, d, K)) return rc;
  if (mem_kind == DHR_MEM_HOST)                             // (a device array is not read back: the kernels leave such a row out of every cluster)
    for (int64_t i = 0; i < n; ++i)
      if (assign[i] < 0 || assign[i] >= K)
        return set_error(DHR_ERR_INVALID, "kmeans update: assign[" + std::to_string(i) + "] = " + std::to_string(assign[i]) + " is outside [0, " +
                                              std::to_string(K) + ")");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  Layout l;
  HIP_TRY(make_layout(n, d, K, 2, l));
  Scratch ws;
  HIP_TRY(ws.alloc(l.total, s));
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_update(l, ws.p, (const _Float16*)values, ld, assign, centroids, counts, s));
    return DHR_OK;
  }
  DevMem m_x, m_c, m_a, m_n;
  HIP_TRY(stage_in(m_x, values, ld, n, d, 2, s));
  HIP_TRY(stage_in(m_c, centroids, (size_t)K * d * 4, s));
  HIP_TRY(stage_in(m_a, assign, (size_t)n * 4, s));
  HIP_TRY(dev_alloc(m_n, (int64_t)K * 8));
  HIP_TRY(launch_update(l, ws.p, (const _Float16*)m_x.p, d, (const int32_t*)m_a.p, (float*)m_c.p, (int64_t*)m_n.p, s));
  HIP_TRY(stage_out(centroids, m_c.p, (size_t)K * d * 4, s));
  HIP_TRY(stage_out(counts, m_n.p, (size_t)K * 8, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_kmeans(int32_t device, int32_t mem_kind, const void* values, int64_t ld, int64_t n, int32_t d, int32_t K, int32_t iters, float* centroids,
                          int32_t* assign, int64_t* counts, double* objective, int64_t* changed, void* stream) try {
  dhr::alloc_checkpoint();
  if (!centroids || !assign || !counts || !objective || !changed) return set_error(DHR_ERR_INVALID, "null pointer");
  if (int rc = check_rows(mem_kind, values, ld, n, d, K)) return rc;
  if (iters < 0) return set_error(DHR_ERR_INVALID, "kmeans: iters must be >= 0, got " + std::to_string(iters));
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  Layout l;
  HIP_TRY(make_layout(n, d, K, 7, l));
  Scratch ws;
  HIP_TRY(ws.alloc(l.total, s));
  const bool host = mem_kind == DHR_MEM_HOST;
  DevMem m_x, m_c, m_a, m_n, m_o, m_ch;
  const _Float16* x = (const _Float16*)values;
  float* c = centroids;
  int32_t* a = assign;
  int64_t *cnt = counts, *chg = changed;
  double* obj = objective;
  if (host) {
    HIP_TRY(stage_in(m_x, values, ld, n, d, 2, s));
    HIP_TRY(stage_in(m_c, centroids, (size_t)K * d * 4, s));
    HIP_TRY(dev_alloc(m_a, n * 4));
    HIP_TRY(dev_alloc(m_n, (int64_t)K * 8));
    HIP_TRY(dev_alloc(m_o, (int64_t)(iters + 1) * 8));
    HIP_TRY(dev_alloc(m_ch, (int64_t)(iters + 1) * 8));
    x = (const _Float16*)m_x.p; ld = d; c = (float*)m_c.p; a = (int32_t*)m_a.p; cnt = (int64_t*)m_n.p; obj = (double*)m_o.p; chg = (int64_t*)m_ch.p;
  }
  float* dist = (float*)(ws.p + l.dist);
  int32_t* prev = (int32_t*)(ws.p + l.prev);
  for (int t = 0; t <= iters; ++t) {
    HIP_TRY(launch_assign(l, ws.p, x, ld, c, a, dist, s));
    hipLaunchKernelGGL(kmeans_stats_kernel, dim3(1), dim3(STATS_THREADS), 0, s, (const float*)dist, (const int32_t*)a, prev, n, (int)(t == 0), obj + t, chg + t);
    HIP_TRY(hipGetLastError());
    if (t < iters) {
      HIP_TRY(launch_update(l, ws.p, x, ld, a, c, cnt, s));
    } else {                                                // the counts of the final assignment
      HIP_TRY(launch_segments(l, ws.p, a, s));
      HIP_TRY(launch_counts(l, ws.p, cnt, s));
    }
  }
  if (host) {
    HIP_TRY(stage_out(centroids, m_c.p, (size_t)K * d * 4, s));
    HIP_TRY(stage_out(assign, m_a.p, (size_t)n * 4, s));
    HIP_TRY(stage_out(counts, m_n.p, (size_t)K * 8, s));
    HIP_TRY(stage_out(objective, m_o.p, (size_t)(iters + 1) * 8, s));
    HIP_TRY(stage_out(changed, m_ch.p, (size_t)(iters + 1) * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DHR_OK;
} DHR_CATCH_STATUS

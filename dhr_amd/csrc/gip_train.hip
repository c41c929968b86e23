// The gated inner product of a training step and of the in-model reranker, with its gradient (tevatron/DHR/modeling.py:161-170, 212-226,
// 250-285).  The reference densifies both sides, repeats the whole passage batch once per query, builds the [n_q, n_p, dims] equality mask,
// multiplies and runs a batched matmul; autograd keeps those tensors.  Here nothing of that size exists:
//   gip_fwd_kernel        one workgroup per (tile of 16*RQ queries x 16*RP passages, slice of dims): stages {value, index} pairs of both sides
//                         through LDS 32 dims at a time, a thread keeps RQ x RP sums in registers.  Small problems split dims over workgroups
//                         (partials in the caller's workspace, folded in slice order by gip_fold_kernel), so the grid fills the device.
//   gip_pair_fwd_kernel   pairwise form: one wave per (query, own passage), lanes along dims, a fixed butterfly.
//   gip_bwd_kernel        owner-computes: a thread owns (R rows, d) of one side's gradient and walks the rows of the other side (loads
//                         coalesced along d, dL/dS read at wave-uniform addresses); the four waves of a workgroup walk a quarter each and
//                         are added in wave order.  gip_pair_bwd_kernel: the same over the query's own block, one wave.
//   densify_bwd_kernel    the whole [batch, vocab] gradient row of densify in one pass: dv at the group the index names, zero elsewhere.
// Every sum has a fixed order (no atomics): two runs on the same inputs are bit-identical.  Products and sums are fp32.
#include "host_stage.h"
#include "op_dispatch.h"

namespace {

constexpr int DK = 32;          // dims staged per step
constexpr int FWD_TARGET = 512; // workgroups the forward aims at before it stops splitting dims
constexpr int MAX_ROWS = 1 << 24;
constexpr int MAX_LIST_QUERIES = 1 << 19;   // the forward's grid: 16 queries per workgroup along y

struct alignas(8) ValIdx {
  float v;
  int i;
};

struct FwdArgs {
  const void *qv, *qi, *pv, *pi;
  int64_t ld_qv, ld_qi, ld_pv, ld_pi;
  int n_q, n_p, dims, chunk;     // chunk: dims per slice (a multiple of DK)
  float* out;                    // slice s writes out + s * slice_stride
  int64_t ld_out, slice_stride;
};

template <typename TV, typename TI, int RQ, int RP>
__global__ void __launch_bounds__(256) gip_fwd_kernel(FwdArgs a) {
  constexpr int TQ = 16 * RQ, TP = 16 * RP;
  __shared__ ValIdx sq[DK][TQ + 1], sp[DK][TP + 1];     // [d][row]: a wave reads 16 consecutive passages, the query is a broadcast
  const int q0 = blockIdx.y * TQ, p0 = blockIdx.x * TP;
  const int d_lo = blockIdx.z * a.chunk, d_hi = min(a.dims, d_lo + a.chunk);
  const int tp = threadIdx.x & 15, tq = threadIdx.x >> 4;
  const int ld_d = threadIdx.x & 31, ld_r = threadIdx.x >> 5;
  const TV *qv = (const TV*)a.qv, *pv = (const TV*)a.pv;
  const TI *qi = (const TI*)a.qi, *pi = (const TI*)a.pi;
  float acc[RQ][RP];
#pragma unroll
  for (int i = 0; i < RQ; ++i)
#pragma unroll
    for (int j = 0; j < RP; ++j) acc[i][j] = 0.f;
  // the next step's elements wait in registers while this step's are multiplied out of LDS
  ValIdx rq[TQ / 8], rp[TP / 8];
  auto fetch = [&](int d0) {
    const int d = d0 + ld_d;
#pragma unroll
    for (int u = 0; u < TQ / 8; ++u) {
      const int64_t row = q0 + ld_r + 8 * u;
      rq[u] = ValIdx{0.f, 0};
      if (row < a.n_q && d < d_hi) { rq[u].v = (float)qv[row * a.ld_qv + d]; rq[u].i = (int)qi[row * a.ld_qi + d]; }
    }
#pragma unroll
    for (int u = 0; u < TP / 8; ++u) {
      const int64_t row = p0 + ld_r + 8 * u;
      rp[u] = ValIdx{0.f, 0};
      if (row < a.n_p && d < d_hi) { rp[u].v = (float)pv[row * a.ld_pv + d]; rp[u].i = (int)pi[row * a.ld_pi + d]; }
    }
  };
  fetch(d_lo);
  for (int d0 = d_lo; d0 < d_hi; d0 += DK) {
#pragma unroll
    for (int u = 0; u < TQ / 8; ++u) sq[ld_d][ld_r + 8 * u] = rq[u];
#pragma unroll
    for (int u = 0; u < TP / 8; ++u) sp[ld_d][ld_r + 8 * u] = rp[u];
    __syncthreads();
    if (d0 + DK < d_hi) fetch(d0 + DK);
#pragma unroll 8
    for (int k = 0; k < DK; ++k) {
      ValIdx q[RQ], p[RP];
#pragma unroll
      for (int i = 0; i < RQ; ++i) q[i] = sq[k][tq + 16 * i];
#pragma unroll
      for (int j = 0; j < RP; ++j) p[j] = sp[k][tp + 16 * j];
#pragma unroll
      for (int i = 0; i < RQ; ++i)
#pragma unroll
        for (int j = 0; j < RP; ++j) acc[i][j] = fmaf(q[i].v, q[i].i == p[j].i ? p[j].v : 0.f, acc[i][j]);
    }
    __syncthreads();
  }
  float* out = a.out + (int64_t)blockIdx.z * a.slice_stride;
#pragma unroll
  for (int i = 0; i < RQ; ++i)
#pragma unroll
    for (int j = 0; j < RP; ++j) {
      const int64_t q = q0 + tq + 16 * i, p = p0 + tp + 16 * j;
      if (q < a.n_q && p < a.n_p) out[q * a.ld_out + p] = acc[i][j];
    }
}

// out[q][p] = sum over slices, in slice order
__global__ void __launch_bounds__(256) gip_fold_kernel(const float* __restrict__ part, int n_slices, int64_t n_q, int64_t n_p, float* __restrict__ out,
                                                       int64_t ld_out) {
  const int64_t n = n_q * n_p;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float s = part[i];
    for (int k = 1; k < n_slices; ++k) s += part[(int64_t)k * n + i];
    out[i / n_p * ld_out + i % n_p] = s;
  }
}

template <typename TV, typename TI>
__global__ void __launch_bounds__(256) gip_pair_fwd_kernel(const TV* __restrict__ qv, int64_t ld_qv, const TI* __restrict__ qi, int64_t ld_qi,
                                                           const TV* __restrict__ pv, int64_t ld_pv, const TI* __restrict__ pi, int64_t ld_pi,
                                                           int64_t n_p, int group, int dims, float* __restrict__ out, int64_t ld_out) {
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);    // passage row b * group + j
  if (p >= n_p) return;
  const int lane = threadIdx.x & 63;
  const int64_t b = p / group;
  float acc = 0.f;
  for (int d = lane; d < dims; d += 64)
    acc = fmaf((float)qv[b * ld_qv + d], (int)qi[b * ld_qi + d] == (int)pi[p * ld_pi + d] ? (float)pv[p * ld_pv + d] : 0.f, acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[b * ld_out + (p - b * group)] = acc;
}

// own side: the rows whose gradient is written; other side: the rows walked.  dL/dS of (own r, other o) is G[r * gs_own + o * gs_oth].
// The four waves of a workgroup own the same (R rows, 64 dims) and walk a quarter of the other side each; wave 0 adds the four partial sums
// in wave order (the split depends on the shape alone).
template <typename TV, typename TI, int R>
__global__ void __launch_bounds__(256) gip_bwd_kernel(const TI* __restrict__ own_i, int64_t ld_oi, int64_t n_own, const TV* __restrict__ oth_v,
                                                      int64_t ld_tv, const TI* __restrict__ oth_i, int64_t ld_ti, int64_t n_oth, int dims,
                                                      const float* __restrict__ G, int64_t gs_own, int64_t gs_oth, float* __restrict__ out,
                                                      int64_t ld_out) {
  __shared__ float part[3][R][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: dL/dS is read by scalar loads)
  const int d = min(blockIdx.y * 64 + lane, dims - 1);     // (a lane past the end repeats the last column and is not written)
  const int64_t r0 = (int64_t)blockIdx.x * R;
  int oi[R];
  float acc[R];
  int64_t g_row[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t r = min(r0 + k, n_own - 1);         // (a row past the end repeats the last one and is not written)
    oi[k] = (int)own_i[r * ld_oi + d];
    g_row[k] = r * gs_own;
    acc[k] = 0.f;
  }
  const int64_t per_wave = (n_oth + 3) / 4;
  const int64_t o_hi = min(n_oth, (wave + 1) * per_wave);
#pragma unroll 8
  for (int64_t o = wave * per_wave; o < o_hi; ++o) {
    const int ti = (int)oth_i[o * ld_ti + d];
    const float tv = (float)oth_v[o * ld_tv + d];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = fmaf(G[g_row[k] + o * gs_oth], oi[k] == ti ? tv : 0.f, acc[k]);
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < R; ++k) part[wave - 1][k][lane] = acc[k];
  }
  __syncthreads();
  if (wave > 0 || blockIdx.y * 64 + lane >= dims) return;
#pragma unroll
  for (int k = 0; k < R; ++k)
    if (r0 + k < n_own) out[(r0 + k) * ld_out + d] = ((acc[k] + part[0][k][lane]) + part[1][k][lane]) + part[2][k][lane];
}

// pairwise: blockIdx.z == side; a NULL output skips its side
template <typename TV, typename TI>
__global__ void __launch_bounds__(64) gip_pair_bwd_kernel(const TV* __restrict__ qv, int64_t ld_qv, const TI* __restrict__ qi, int64_t ld_qi,
                                                          int64_t n_q, const TV* __restrict__ pv, int64_t ld_pv, const TI* __restrict__ pi,
                                                          int64_t ld_pi, int group, int dims, const float* __restrict__ G, int64_t ld_g,
                                                          float* __restrict__ dq, int64_t ld_dq, float* __restrict__ dp, int64_t ld_dp) {
  const int d = blockIdx.y * 64 + threadIdx.x;
  if (d >= dims) return;
  const int64_t row = blockIdx.x;
  if (blockIdx.z == 0) {
    if (!dq || row >= n_q) return;
    const int own = (int)qi[row * ld_qi + d];
    float acc = 0.f;
    for (int j = 0; j < group; ++j) {
      const int64_t p = row * group + j;
      acc = fmaf(G[row * ld_g + j], own == (int)pi[p * ld_pi + d] ? (float)pv[p * ld_pv + d] : 0.f, acc);
    }
    dq[row * ld_dq + d] = acc;
  } else {
    if (!dp) return;                                   // row < n_q * group by the grid
    const int64_t b = row / group;
    dp[row * ld_dp + d] = G[b * ld_g + (row - b * group)] * ((int)pi[row * ld_pi + d] == (int)qi[b * ld_qi + d] ? (float)qv[b * ld_qv + d] : 0.f);
  }
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(256) densify_bwd_kernel(const float* __restrict__ dv, int64_t ld_dv, const TI* __restrict__ idx, int64_t ld_idx,
                                                          int64_t batch, int remove, int dims, int n_groups, TO* __restrict__ out, int64_t ld_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  for (int64_t b = blockIdx.y; b < batch; b += gridDim.y) {
    TO* row = out + b * ld_out;
    if (blockIdx.x == 0)
      for (int c = threadIdx.x; c < remove; c += 256) row[c] = (TO)0.f;
    if (j >= dims) continue;
    const float v = dv[b * ld_dv + j];
    const int g0 = (int)idx[b * ld_idx + j];
    TO* col = row + remove + j;
    for (int g = 0; g < n_groups; ++g) col[(int64_t)g * dims] = (TO)(g == g0 ? v : 0.f);
  }
}

// how the forward tiles a listwise problem: thread tile, dims per slice, slices
struct FwdPlan {
  int small, chunk, slices;
};
FwdPlan plan_fwd(int64_t n_q, int64_t n_p, int dims, bool may_split) {
  const int steps = (dims + DK - 1) / DK;
  const int64_t big_tiles = ((n_q + 31) / 32) * ((n_p + 63) / 64);
  FwdPlan pl;
  pl.small = big_tiles * steps < FWD_TARGET / 2;       // even one step per slice leaves 32 x 64 tiles short of the device: 16 x 16 tiles
  const int64_t tiles = pl.small ? ((n_q + 15) / 16) * ((n_p + 15) / 16) : big_tiles;
  int want = may_split ? (int)std::min<int64_t>(steps, std::max<int64_t>(1, FWD_TARGET / tiles)) : 1;
  const int steps_per = (steps + want - 1) / want;
  pl.chunk = steps_per * DK;
  pl.slices = (steps + steps_per - 1) / steps_per;
  return pl;
}

struct Sides {
  const void *qv, *qi, *pv, *pi;
  int64_t ld_qv, ld_qi, ld_pv, ld_pi, n_q, n_p;
  int dims, val_dt, idx_dt, group;
};

// f(tag of the value type, tag of the index type) of the two sides
template <class F>
auto with_side_types(const Sides& x, F&& f) {
  return with_value_type(x.val_dt, [&](auto v) { return with_index_type(x.idx_dt, [&](auto i) { return f(v, i); }); });
}

hipError_t launch_scores(const Sides& x, float* out, int64_t ld_out, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (x.group > 0) {
    const dim3 grid((unsigned)((x.n_p + 3) / 4));
    with_side_types(x, [&](auto v, auto i) {
      using TV = typename decltype(v)::type;
      using TI = typename decltype(i)::type;
      hipLaunchKernelGGL((gip_pair_fwd_kernel<TV, TI>), grid, dim3(256), 0, s, (const TV*)x.qv, x.ld_qv, (const TI*)x.qi, x.ld_qi, (const TV*)x.pv,
                         x.ld_pv, (const TI*)x.pi, x.ld_pi, x.n_p, x.group, x.dims, out, ld_out);
    });
    return hipGetLastError();
  }
  FwdPlan pl = plan_fwd(x.n_q, x.n_p, x.dims, ws != nullptr);
  if (pl.slices > 1 && ws_bytes < (int64_t)pl.slices * x.n_q * x.n_p * 4) pl = plan_fwd(x.n_q, x.n_p, x.dims, false);
  FwdArgs a{x.qv, x.qi, x.pv, x.pi, x.ld_qv, x.ld_qi, x.ld_pv, x.ld_pi, (int)x.n_q, (int)x.n_p, x.dims, pl.chunk, out, ld_out, 0};
  if (pl.slices > 1) { a.out = (float*)ws; a.ld_out = x.n_p; a.slice_stride = x.n_q * x.n_p; }
  const int tq = pl.small ? 16 : 32, tp = pl.small ? 16 : 64;
  const dim3 grid((unsigned)((x.n_p + tp - 1) / tp), (unsigned)((x.n_q + tq - 1) / tq), (unsigned)pl.slices);
  with_side_types(x, [&](auto v, auto i) { with_flag(pl.small != 0, [&](auto small) {
    using TV = typename decltype(v)::type;
    using TI = typename decltype(i)::type;
    constexpr int RQ = decltype(small)::value ? 1 : 2, RP = decltype(small)::value ? 1 : 4;   // the thread tile: 16 x 16 or 32 x 64 per workgroup
    hipLaunchKernelGGL((gip_fwd_kernel<TV, TI, RQ, RP>), grid, dim3(256), 0, s, a);
  }); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || pl.slices == 1) return e;
  const unsigned blocks = (unsigned)std::min<int64_t>((x.n_q * x.n_p + 255) / 256, 4096);
  hipLaunchKernelGGL(gip_fold_kernel, dim3(blocks), dim3(256), 0, s, (const float*)ws, pl.slices, x.n_q, x.n_p, out, ld_out);
  return hipGetLastError();
}

template <typename TV, typename TI>
hipError_t launch_bwd_side(const void* own_i, int64_t ld_oi, int64_t n_own, const void* oth_v, int64_t ld_tv, const void* oth_i, int64_t ld_ti,
                           int64_t n_oth, int dims, const float* G, int64_t gs_own, int64_t gs_oth, float* out, int64_t ld_out, hipStream_t s) {
  const int d_blocks = (dims + 63) / 64;
  const int R = (n_own + 3) / 4 * d_blocks >= 256 ? 4 : (n_own + 1) / 2 * d_blocks >= 256 ? 2 : 1;   // four-wave workgroups against the device's 256 CUs
  const dim3 grid((unsigned)((n_own + R - 1) / R), (unsigned)d_blocks);
  with_int<4, 2, 1>(R, [&](auto r) {
    hipLaunchKernelGGL((gip_bwd_kernel<TV, TI, decltype(r)::value>), grid, dim3(256), 0, s, (const TI*)own_i, ld_oi, n_own, (const TV*)oth_v, ld_tv,
                       (const TI*)oth_i, ld_ti, n_oth, dims, G, gs_own, gs_oth, out, ld_out);
  });
  return hipGetLastError();
}

hipError_t launch_scores_bwd(const Sides& x, const float* G, int64_t ld_g, float* dq, int64_t ld_dq, float* dp, int64_t ld_dp, hipStream_t s) {
  if (x.group > 0) {
    const dim3 grid((unsigned)x.n_p, (unsigned)((x.dims + 63) / 64), 2);       // n_p >= n_q rows cover both sides
    with_side_types(x, [&](auto v, auto i) {
      using TV = typename decltype(v)::type;
      using TI = typename decltype(i)::type;
      hipLaunchKernelGGL((gip_pair_bwd_kernel<TV, TI>), grid, dim3(64), 0, s, (const TV*)x.qv, x.ld_qv, (const TI*)x.qi, x.ld_qi, x.n_q,
                         (const TV*)x.pv, x.ld_pv, (const TI*)x.pi, x.ld_pi, x.group, x.dims, G, ld_g, dq, ld_dq, dp, ld_dp);
    });
    return hipGetLastError();
  }
  return with_side_types(x, [&](auto v, auto i) {
    using TV = typename decltype(v)::type;
    using TI = typename decltype(i)::type;
    hipError_t e = hipSuccess;
    if (dq) e = launch_bwd_side<TV, TI>(x.qi, x.ld_qi, x.n_q, x.pv, x.ld_pv, x.pi, x.ld_pi, x.n_p, x.dims, G, ld_g, 1, dq, ld_dq, s);
    if (dp && e == hipSuccess) e = launch_bwd_side<TV, TI>(x.pi, x.ld_pi, x.n_p, x.qv, x.ld_qv, x.qi, x.ld_qi, x.n_q, x.dims, G, 1, ld_g, dp, ld_dp, s);
    return e;
  });
}

hipError_t launch_densify_bwd(const float* dv, int64_t ld_dv, const void* idx, int idx_dt, int64_t ld_idx, int64_t batch, int remove, int dims,
                              int n_groups, void* out, int out_dt, int64_t ld_out, hipStream_t s) {
  const dim3 grid((unsigned)((dims + 255) / 256), (unsigned)std::min<int64_t>(batch, 65535));
  with_value_type(out_dt, [&](auto o) { with_index_type(idx_dt, [&](auto i) {
    using TO = typename decltype(o)::type;
    using TI = typename decltype(i)::type;
    hipLaunchKernelGGL((densify_bwd_kernel<TI, TO>), grid, dim3(256), 0, s, dv, ld_dv, (const TI*)idx, ld_idx, batch, remove, dims, n_groups, (TO*)out,
                       ld_out);
  }); });
  return hipGetLastError();
}

// the checks the forward and the backward share; fills x
int check_sides(const void* qv, int64_t ld_qv, const void* qi, int64_t ld_qi, int64_t n_q, const void* pv, int64_t ld_pv, const void* pi,
                int64_t ld_pi, int64_t n_p, int32_t dims, int32_t value_dtype, int32_t index_dtype, int32_t group, int32_t mem_kind, Sides& x) {
  if (!qv || !qi || !pv || !pi) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!val_ok(value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (!idx_ok(index_dtype)) return set_error(DHR_ERR_INVALID, "index dtype must be uint8, int8 or int16");
  if (n_q < 0 || n_p < 0 || n_q > MAX_ROWS || n_p > MAX_ROWS || dims <= 0 || group < 0 || ld_qv < dims || ld_qi < dims || ld_pv < dims || ld_pi < dims)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (group == 0 && n_q > MAX_LIST_QUERIES) return set_error(DHR_ERR_UNSUPPORTED, "listwise scores: more than 524288 queries");
  if (group > 0 && n_p != n_q * group)
    return set_error(DHR_ERR_INVALID, "pairwise scores: " + std::to_string(n_p) + " passage rows for " + std::to_string(n_q) + " queries x " +
                                          std::to_string(group) + " passages");
  x = Sides{qv, qi, pv, pi, ld_qv, ld_qi, ld_pv, ld_pi, n_q, n_p, dims, value_dtype, index_dtype, group};
  return DHR_OK;
}

// stages the four input arrays of a host call; x then points at the device copies
hipError_t stage_sides(Sides& x, DevMem m[4], hipStream_t s) {
  const int ves = val_esize(x.val_dt), xes = idx_esize(x.idx_dt);
  hipError_t e;
  if ((e = stage_in(m[0], x.qv, x.ld_qv, x.n_q, x.dims, ves, s)) != hipSuccess || (e = stage_in(m[1], x.qi, x.ld_qi, x.n_q, x.dims, xes, s)) != hipSuccess ||
      (e = stage_in(m[2], x.pv, x.ld_pv, x.n_p, x.dims, ves, s)) != hipSuccess || (e = stage_in(m[3], x.pi, x.ld_pi, x.n_p, x.dims, xes, s)) != hipSuccess)
    return e;
  x.qv = m[0].p; x.qi = m[1].p; x.pv = m[2].p; x.pi = m[3].p;
  x.ld_qv = x.ld_qi = x.ld_pv = x.ld_pi = x.dims;
  return hipSuccess;
}

}  // namespace

extern "C" int64_t dhr_gip_scores_workspace(int64_t n_q, int64_t n_p, int32_t dims, int32_t group) try {
  if (n_q <= 0 || n_p <= 0 || n_q > MAX_ROWS || n_p > MAX_ROWS || dims <= 0 || group != 0) return 0;
  const FwdPlan pl = plan_fwd(n_q, n_p, dims, true);
  return pl.slices > 1 ? (int64_t)pl.slices * n_q * n_p * 4 : 0;
} DHR_CATCH_VALUE(0)

extern "C" int dhr_gip_scores(int32_t device, int32_t mem_kind, const void* q_value, int64_t ld_q_value, const void* q_index, int64_t ld_q_index,
                              int64_t n_q, const void* p_value, int64_t ld_p_value, const void* p_index, int64_t ld_p_index, int64_t n_p, int32_t dims,
                              int32_t value_dtype, int32_t index_dtype, int32_t group, float* out, int64_t ld_out, void* workspace,
                              int64_t workspace_bytes, void* stream) try {
  dhr::alloc_checkpoint();
  Sides x;
  if (!out) return set_error(DHR_ERR_INVALID, "null pointer");
  int rc = check_sides(q_value, ld_q_value, q_index, ld_q_index, n_q, p_value, ld_p_value, p_index, ld_p_index, n_p, dims, value_dtype, index_dtype,
                       group, mem_kind, x);
  if (rc) return rc;
  const int64_t out_cols = group > 0 ? group : n_p;
  if (ld_out < out_cols || workspace_bytes < 0) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (n_q == 0 || n_p == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_scores(x, out, ld_out, workspace, workspace ? workspace_bytes : 0, s));
    return DHR_OK;
  }
  DevMem m[4], m_out, m_ws;
  HIP_TRY(stage_sides(x, m, s));
  HIP_TRY(dev_alloc(m_out, n_q * out_cols * 4));
  const int64_t ws_bytes = dhr_gip_scores_workspace(n_q, n_p, dims, group);
  if (ws_bytes) HIP_TRY(dev_alloc(m_ws, ws_bytes));
  HIP_TRY(launch_scores(x, (float*)m_out.p, out_cols, m_ws.p, ws_bytes, s));
  HIP_TRY(stage_out(out, ld_out, m_out.p, n_q, out_cols, 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_gip_scores_backward(int32_t device, int32_t mem_kind, const void* q_value, int64_t ld_q_value, const void* q_index,
                                       int64_t ld_q_index, int64_t n_q, const void* p_value, int64_t ld_p_value, const void* p_index,
                                       int64_t ld_p_index, int64_t n_p, int32_t dims, int32_t value_dtype, int32_t index_dtype, int32_t group,
                                       const float* grad_out, int64_t ld_grad, float* grad_q, int64_t ld_grad_q, float* grad_p, int64_t ld_grad_p,
                                       void* stream) try {
  dhr::alloc_checkpoint();
  Sides x;
  if (!grad_out) return set_error(DHR_ERR_INVALID, "null pointer");
  int rc = check_sides(q_value, ld_q_value, q_index, ld_q_index, n_q, p_value, ld_p_value, p_index, ld_p_index, n_p, dims, value_dtype, index_dtype,
                       group, mem_kind, x);
  if (rc) return rc;
  const int64_t g_cols = group > 0 ? group : n_p;
  if (ld_grad < g_cols || (grad_q && ld_grad_q < dims) || (grad_p && ld_grad_p < dims)) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if ((!grad_q && !grad_p) || (n_q == 0 && n_p == 0)) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_scores_bwd(x, grad_out, ld_grad, n_q ? grad_q : nullptr, ld_grad_q, n_p ? grad_p : nullptr, ld_grad_p, s));
    return DHR_OK;
  }
  DevMem m[4], m_g, m_dq, m_dp;
  HIP_TRY(stage_sides(x, m, s));
  HIP_TRY(stage_in(m_g, grad_out, ld_grad, n_q, g_cols, 4, s));
  if (grad_q && n_q) HIP_TRY(dev_alloc(m_dq, n_q * dims * 4));
  if (grad_p && n_p) HIP_TRY(dev_alloc(m_dp, n_p * dims * 4));
  HIP_TRY(launch_scores_bwd(x, (const float*)m_g.p, g_cols, (float*)m_dq.p, dims, (float*)m_dp.p, dims, s));
  if (m_dq.p) HIP_TRY(stage_out(grad_q, ld_grad_q, m_dq.p, n_q, dims, 4, s));
  if (m_dp.p) HIP_TRY(stage_out(grad_p, ld_grad_p, m_dp.p, n_p, dims, 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_densify_backward(int32_t device, int32_t mem_kind, const float* grad_value, int64_t ld_grad_value, const void* index,
                                    int32_t index_dtype, int64_t ld_index, int64_t batch, int32_t vocab, int32_t remove_dims, int32_t dims,
                                    void* grad_lexical, int32_t grad_dtype, int64_t ld_grad, void* stream) try {
  dhr::alloc_checkpoint();
  if (!grad_value || !index || !grad_lexical) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!val_ok(grad_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (!idx_ok(index_dtype)) return set_error(DHR_ERR_INVALID, "index dtype must be uint8, int8 or int16");
  if (batch < 0 || vocab <= 0 || dims <= 0 || remove_dims < 0 || remove_dims >= vocab || ld_grad < vocab || ld_grad_value < dims || ld_index < dims)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if ((vocab - remove_dims) % dims != 0)
    return set_error(DHR_ERR_INVALID, "Input lexical representation cannot be densified, please fix dims or remove_dims");
  const int n_groups = (vocab - remove_dims) / dims;
  if (batch == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_densify_bwd(grad_value, ld_grad_value, index, index_dtype, ld_index, batch, remove_dims, dims, n_groups, grad_lexical,
                               grad_dtype, ld_grad, s));
    return DHR_OK;
  }
  // host arrays: stage blocks of rows through the device
  const int oes = val_esize(grad_dtype), xes = idx_esize(index_dtype);
  const int64_t block = std::max<int64_t>(1, std::min<int64_t>(batch, ((int64_t)256 << 20) / ((int64_t)vocab * oes)));
  DevMem m_out;
  HIP_TRY(dev_alloc(m_out, block * vocab * oes));
  for (int64_t lo = 0; lo < batch; lo += block) {
    const int64_t rows = std::min(block, batch - lo);
    DevMem m_dv, m_idx;
    HIP_TRY(stage_in(m_dv, grad_value + lo * ld_grad_value, ld_grad_value, rows, dims, 4, s));
    HIP_TRY(stage_in(m_idx, (const char*)index + lo * ld_index * xes, ld_index, rows, dims, xes, s));
    HIP_TRY(launch_densify_bwd((const float*)m_dv.p, dims, m_idx.p, index_dtype, dims, rows, remove_dims, dims, n_groups, m_out.p,
                               grad_dtype, vocab, s));
    HIP_TRY(stage_out((char*)grad_lexical + lo * ld_grad * oes, ld_grad, m_out.p, rows, vocab, oes, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DHR_OK;
} DHR_CATCH_STATUS

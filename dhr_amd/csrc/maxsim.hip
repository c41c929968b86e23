// Late-interaction (MaxSim) scores of a ColBERT training step and of the TCT teacher of a DHR step, with their gradient
// (tevatron/ColBERT/modeling.py:188-190, 204-219).  The reference builds scores[a][b][i][j] = <q[a][i], p[b][j]> as one [n_q, n_p, Lq, Lp]
// tensor, takes the max over j and the sum over i; autograd keeps that tensor and scatters into a zero-filled copy of it.  Here:
//   maxsim_fwd_kernel     a workgroup owns one passage b and a block of 4 * NQ queries (a wave: NQ of them).  The passage's tokens go through
//                         LDS 32 tokens x 256 bytes at a time (rows padded to 272 bytes: the 16-byte fragment reads of 16 consecutive rows fall
//                         on 16 different slots of a bank row), the wave's query block is the B operand of v_mfma_f32_32x32x16_f16 (fp32
//                         inputs: v_mfma_f32_32x32x2_f32, exact), so a lane holds one query token against 16 passage tokens: the max over
//                         passage tokens is a register reduction with a running (value, token), the sum over query tokens one 32-lane
//                         butterfly.  D <= one chunk (128 fp16 / 64 fp32 columns): the query fragments stay in registers; wider: a K loop with
//                         the accumulators kept across it and the query fragments re-read per chunk.
//   maxsim_bwd_q_kernel   owner-computes: a workgroup owns (a, i), a thread 4 columns of D; the rows of threads walk b interleaved, several
//                         gathers of p[b][arg[a][b][i]] in flight, and their partial sums are added in row order.
//   maxsim_bwd_p_kernel   a wave owns (b, a block of passage tokens, 128 columns) with fp32 accumulators in LDS; it walks (a, i) in
//                         increasing order, 64 at a time (arg and dL/dS loaded once per lane, the tokens of its block picked by a ballot),
//                         adds G * q[a][i] into row arg - first token, and writes the whole block once.
// Every sum has a fixed order that depends on the shape alone (no atomics): two runs are bit-identical, and a pair's score does not depend on
// which other pairs are scored.  Products and sums are fp32.
#include "host_stage.h"
#include "op_dispatch.h"

namespace {

constexpr int ROW_BYTES = 256;             // bytes of one token staged per K chunk: 128 fp16 / 64 fp32 columns
constexpr int ROW_PITCH = ROW_BYTES + 16;  // LDS pitch of a token
constexpr int TILE = 32;                   // tokens per MFMA tile, both sides
constexpr int MAX_D = 1024, MAX_LP = 32767;
constexpr int64_t MAX_BATCH = 1 << 17, MAX_LQ = 1 << 16;
constexpr int BWD_P_ROWS = 16;             // passage tokens a wave of the dp kernel owns (16 x 128 fp32 = 8 KB of LDS)
constexpr int BWD_P_COLS = 128;
constexpr int FWD_FILL = 512;              // workgroups the forward wants before it gives a wave two queries

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

struct Side {
  const void* x;
  int64_t ld_tok, ld_batch;
  int64_t n;      // batch
  int len;        // tokens
  int vec;        // 16-byte loads are aligned (base and both strides)
};

struct FwdArgs {
  Side q, p;
  int D, group, n_chunks;
  float* out;
  int64_t ld_out;
  int16_t* arg;   // [A][cols][Lq] or NULL
  int64_t cols;
};

// 16 bytes of a row starting at element col0: one aligned load, or element by element with zeros beyond D
template <typename T>
__device__ __forceinline__ uint4 load16(const T* row, int col0, int D, bool vec) {
  constexpr int E = 16 / (int)sizeof(T);
  if (vec && col0 + E <= D) return *reinterpret_cast<const uint4*>(row + col0);
  union { uint4 u; T t[E]; } r;
  r.u = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (col0 + e < D) r.t[e] = row[col0 + e];
  return r.u;
}

// acc += P-tile fragment x Q-block fragment over one 256-byte chunk: slot 2v + h of a row is the k range of lane half h in step v
template <typename T>
__device__ __forceinline__ void mma_chunk(const uint4 (&pf)[8], const uint4 (&qf)[8], float16v& acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      union { uint4 u; half8 h; } a, b;
      a.u = pf[v]; b.u = qf[v];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.h, b.h, acc, 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(pf[v].x), __uint_as_float(qf[v].x), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(pf[v].y), __uint_as_float(qf[v].y), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(pf[v].z), __uint_as_float(qf[v].z), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(pf[v].w), __uint_as_float(qf[v].w), acc, 0, 0, 0);
    }
  }
#endif
}

// grid: (passage b, block of 4 * NQ queries; group > 0: one block, the passage's own query).  MULTI: D spans more than one chunk.
template <typename T, int NQ, bool MULTI>
__global__ void __launch_bounds__(256) maxsim_fwd_kernel(FwdArgs g) {
  constexpr int E = 16 / (int)sizeof(T);         // elements per 16-byte slot
  constexpr int KC = ROW_BYTES / (int)sizeof(T); // columns per chunk
  __shared__ __attribute__((aligned(16))) unsigned char tile[TILE * ROW_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t b = blockIdx.x;
  const int Lq = g.q.len, Lp = g.p.len, D = g.D;
  const T* pb = (const T*)g.p.x + b * g.p.ld_batch;
  // the queries of this wave
  int64_t qa[NQ];
  bool q_on[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    if (g.group > 0) { qa[u] = b / g.group; q_on[u] = wave == 0 && u == 0; }
    else { qa[u] = (int64_t)blockIdx.y * (4 * NQ) + wave + 4 * u; q_on[u] = qa[u] < g.q.n; }
  }
  const int64_t col = g.group > 0 ? b % g.group : b;
  // staging: thread t moves slots t and t + 256 of the 32 x 16 slots of a chunk
  const int st_row = threadIdx.x >> 4, st_slot = threadIdx.x & 15;
  uint4 stage[2];
  auto fetch = [&](int tile_j0, int chunk) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = tile_j0 + st_row + 16 * u;
      stage[u] = j < Lp ? load16<T>(pb + (int64_t)j * g.p.ld_tok, chunk * KC + st_slot * E, D, g.p.vec) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto load_q = [&](uint4 (&qf)[8], int64_t a, int i0, int chunk) {
    const int i = i0 + r;
    const T* row = (const T*)g.q.x + a * g.q.ld_batch + (int64_t)i * g.q.ld_tok;
#pragma unroll
    for (int v = 0; v < 8; ++v) qf[v] = i < Lq ? load16<T>(row, chunk * KC + (2 * v + h) * E, D, g.q.vec) : make_uint4(0u, 0u, 0u, 0u);
  };

  float score[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) score[u] = 0.f;
  const int n_steps = ((Lp + TILE - 1) / TILE) * g.n_chunks;

  for (int i0 = 0; i0 < Lq; i0 += TILE) {
    float best_v[NQ];
    int best_j[NQ];
    float16v acc[NQ];
    uint4 qreg[MULTI ? 1 : NQ][8];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      best_v[u] = -INFINITY;
      best_j[u] = 0;
      if constexpr (!MULTI)
        if (q_on[u]) load_q(qreg[u], qa[u], i0, 0);
    }
    fetch(0, 0);
    for (int step = 0; step < n_steps; ++step) {
      const int j0 = (step / g.n_chunks) * TILE, chunk = step % g.n_chunks;
#pragma unroll
      for (int u = 0; u < 2; ++u) *reinterpret_cast<uint4*>(tile + (st_row + 16 * u) * ROW_PITCH + st_slot * 16) = stage[u];
      __syncthreads();
      if (step + 1 < n_steps) fetch(((step + 1) / g.n_chunks) * TILE, (step + 1) % g.n_chunks);
      uint4 pf[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) pf[v] = *reinterpret_cast<const uint4*>(tile + r * ROW_PITCH + (2 * v + h) * 16);
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        if (!q_on[u]) continue;                          // (wave-uniform)
        if (chunk == 0)
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[u][k] = 0.f;
        if constexpr (MULTI) {
          load_q(qreg[0], qa[u], i0, chunk);
          mma_chunk<T>(pf, qreg[0], acc[u]);
        } else {
          mma_chunk<T>(pf, qreg[u], acc[u]);
        }
        if (chunk == g.n_chunks - 1) {
          // this lane: query token i0 + r against passage tokens j0 + 4h + (k & 3) + 8 (k >> 2), increasing in k: strict > keeps the first
          if (j0 + TILE <= Lp) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
              if (acc[u][k] > best_v[u]) { best_v[u] = acc[u][k]; best_j[u] = j0 + 4 * h + (k & 3) + 8 * (k >> 2); }
          } else {                                       // the passage's last tile: its padded rows never win
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              const int j = j0 + 4 * h + (k & 3) + 8 * (k >> 2);
              if (j < Lp && acc[u][k] > best_v[u]) { best_v[u] = acc[u][k]; best_j[u] = j; }
            }
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      if (!q_on[u]) continue;
      // the two lane halves hold interleaved passage tokens of the same query token
      const float ov = __shfl_xor(best_v[u], 32, 64);
      const int oj = __shfl_xor(best_j[u], 32, 64);
      if (ov > best_v[u] || (ov == best_v[u] && oj < best_j[u])) { best_v[u] = ov; best_j[u] = oj; }
      const bool real = i0 + r < Lq;
      if (g.arg && real && h == 0) g.arg[(qa[u] * g.cols + col) * Lq + i0 + r] = (int16_t)best_j[u];
      float s = real ? best_v[u] : 0.f;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      score[u] += s;
    }
  }
#pragma unroll
  for (int u = 0; u < NQ; ++u)
    if (q_on[u] && lane == 0) g.out[qa[u] * g.ld_out + col] = score[u];
}

struct BwdArgs {
  Side q, p;
  int D, group;
  const int16_t* arg;   // [A][cols][Lq]
  int64_t cols;
  const float* G;
  int64_t ld_g;
  void* dq;             // [A][Lq][D] packed, TO
  void* dp;             // [B][Lp][D] packed, TO
};

// 4 consecutive columns of a row starting at d0, as floats (zeros beyond D)
template <typename T>
__device__ __forceinline__ float4 load4(const T* row, int d0, int D, bool vec) {
  if (vec && d0 + 4 <= D) {
    if constexpr (sizeof(T) == 2) {
      union { uint2 u; T t[4]; } r;
      r.u = *reinterpret_cast<const uint2*>(row + d0);
      return make_float4((float)r.t[0], (float)r.t[1], (float)r.t[2], (float)r.t[3]);
    } else {
      return *reinterpret_cast<const float4*>(row + d0);
    }
  }
  float4 o;
  o.x = d0 < D ? (float)row[d0] : 0.f;
  o.y = d0 + 1 < D ? (float)row[d0 + 1] : 0.f;
  o.z = d0 + 2 < D ? (float)row[d0 + 2] : 0.f;
  o.w = d0 + 3 < D ? (float)row[d0 + 3] : 0.f;
  return o;
}

// grid: a * Lq + i.  tpr threads (a power of two, 4 columns each) cover D; the 256 / tpr rows of threads walk b interleaved.
template <typename T, typename TO>
__global__ void __launch_bounds__(256) maxsim_bwd_q_kernel(BwdArgs g, int tpr) {
  __shared__ float4 part[256];
  const int Lq = g.q.len, D = g.D;
  const int64_t a = blockIdx.x / Lq;
  const int i = (int)(blockIdx.x - a * Lq);
  const int rows = 256 / tpr, slot = threadIdx.x / tpr, d0 = (threadIdx.x % tpr) * 4;
  const int64_t b_lo = g.group > 0 ? a * g.group : 0, n_b = g.group > 0 ? g.group : g.p.n;
  const int16_t* arg = g.arg + a * g.cols * Lq + i;
  const float* G = g.G + a * g.ld_g;
  const T* p = (const T*)g.p.x;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (d0 < D) {
#pragma unroll 8
    for (int64_t c = slot; c < n_b; c += rows) {
      const int j = min(max((int)arg[c * Lq], 0), g.p.len - 1);      // (a winner the forward wrote is in range; a caller's own array may not be)
      const float w = G[c];
      const float4 v = load4<T>(p + (b_lo + c) * g.p.ld_batch + (int64_t)j * g.p.ld_tok, d0, D, g.p.vec);
      acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
    }
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (slot != 0 || d0 >= D) return;
  for (int s = 1; s < rows; ++s) {                      // in row order
    const float4 o = part[s * tpr + threadIdx.x];
    acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
  }
  TO* out = (TO*)g.dq + ((int64_t)blockIdx.x) * D + d0;
  out[0] = (TO)acc.x;
  if (d0 + 1 < D) out[1] = (TO)acc.y;
  if (d0 + 2 < D) out[2] = (TO)acc.z;
  if (d0 + 3 < D) out[3] = (TO)acc.w;
}

// grid: (b, block of BWD_P_ROWS passage tokens, block of BWD_P_COLS columns); one wave, a lane owns two columns
template <typename T, typename TO>
__global__ void __launch_bounds__(64) maxsim_bwd_p_kernel(BwdArgs g) {
  __shared__ float2 acc[BWD_P_ROWS][64];
  const int lane = threadIdx.x;
  const int Lq = g.q.len, Lp = g.p.len, D = g.D;
  const int64_t b = blockIdx.x;
  const int j_lo = blockIdx.y * BWD_P_ROWS, d0 = blockIdx.z * BWD_P_COLS + 2 * lane;
  const int64_t a_lo = g.group > 0 ? b / g.group : 0, n_a = g.group > 0 ? 1 : g.q.n;
  const int64_t col = g.group > 0 ? b % g.group : b;
  const bool pair = (g.q.vec & 2) && d0 + 2 <= D;       // one aligned load of both columns
#pragma unroll
  for (int k = 0; k < BWD_P_ROWS; ++k) acc[k][lane] = make_float2(0.f, 0.f);
  const T* q = (const T*)g.q.x;
  const int64_t total = n_a * Lq;
  for (int64_t f0 = 0; f0 < total; f0 += 64) {
    // lane: element f0 + lane of the (a, i) sequence
    const int64_t f = f0 + lane;
    int rel = -1;
    float w = 0.f;
    if (f < total) {
      const int64_t a = a_lo + f / Lq;
      rel = (int)g.arg[(a * g.cols + col) * Lq + f % Lq] - j_lo;
      w = g.G[a * g.ld_g + col];
    }
    unsigned long long todo = __ballot((unsigned)rel < (unsigned)BWD_P_ROWS);
    while (todo) {                                       // in increasing (a, i), eight gathers in flight
      int at[8];
      float2 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        at[k] = -1;
        if (todo) {
          at[k] = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int64_t fk = f0 + at[k];
          const T* row = q + (a_lo + fk / Lq) * g.q.ld_batch + (fk % Lq) * g.q.ld_tok;
          if (pair) {
            if constexpr (sizeof(T) == 2) {
              union { uint32_t u; T t[2]; } x;
              x.u = *reinterpret_cast<const uint32_t*>(row + d0);
              v[k] = make_float2((float)x.t[0], (float)x.t[1]);
            } else {
              v[k] = *reinterpret_cast<const float2*>(row + d0);
            }
          } else {
            v[k].x = d0 < D ? (float)row[d0] : 0.f;
            v[k].y = d0 + 1 < D ? (float)row[d0 + 1] : 0.f;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (at[k] < 0) break;
        const int row = __shfl(rel, at[k], 64);
        const float wk = __shfl(w, at[k], 64);
        float2 s = acc[row][lane];
        s.x = fmaf(wk, v[k].x, s.x);
        s.y = fmaf(wk, v[k].y, s.y);
        acc[row][lane] = s;
      }
    }
  }
  TO* out = (TO*)g.dp + (b * Lp + j_lo) * D + d0;
  for (int k = 0; k < BWD_P_ROWS && j_lo + k < Lp; ++k) {
    const float2 s = acc[k][lane];
    if (d0 < D) out[(int64_t)k * D] = (TO)s.x;
    if (d0 + 1 < D) out[(int64_t)k * D + 1] = (TO)s.y;
  }
}

bool aligned(const void* x, int64_t ld_tok, int64_t ld_batch, int es, int bytes) {
  return (uintptr_t)x % bytes == 0 && (ld_tok * es) % bytes == 0 && (ld_batch * es) % bytes == 0;
}

// vec bit 0: 16-byte loads (forward), 8 bytes of fp16 / 16 of fp32 for the dq gathers; bit 1: a pair of columns (dp)
Side make_side(const void* x, int64_t ld_tok, int64_t ld_batch, int64_t n, int len, int es) {
  Side s{x, ld_tok, ld_batch, n, len, 0};
  if (aligned(x, ld_tok, ld_batch, es, 16)) s.vec |= 1;
  if (aligned(x, ld_tok, ld_batch, es, 2 * es)) s.vec |= 2;
  return s;
}

struct Problem {
  Side q, p;
  int D, val_dt, group;
  int64_t cols;
};

hipError_t launch_fwd(const Problem& x, float* out, int64_t ld_out, int16_t* arg, hipStream_t s) {
  const int kc = ROW_BYTES / val_esize(x.val_dt);
  FwdArgs a{x.q, x.p, x.D, x.group, (x.D + kc - 1) / kc, out, ld_out, arg, x.cols};
  a.q.vec &= 1; a.p.vec &= 1;
  const bool multi = a.n_chunks > 1;
  // two queries per wave where that still fills the device: half the re-reads of a passage tile.  Four per wave need 256 registers, which
  // leaves one workgroup per CU, and measured slower (profiles/maxsim_scores.txt).
  const int nq = x.group == 0 && ((x.q.n + 7) / 8) * x.p.n >= FWD_FILL ? 2 : 1;
  const int per_wg = 4 * nq;
  const dim3 grid((unsigned)x.p.n, x.group > 0 ? 1u : (unsigned)((x.q.n + per_wg - 1) / per_wg));
  with_value_type(x.val_dt, [&](auto t) { with_int<2, 1>(nq, [&](auto n) { with_flag(multi, [&](auto m) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((maxsim_fwd_kernel<T, decltype(n)::value, decltype(m)::value>), grid, dim3(256), 0, s, a);
  }); }); });
  return hipGetLastError();
}

hipError_t launch_bwd(const Problem& x, const int16_t* arg, const float* G, int64_t ld_g, void* dq, void* dp, int grad_dt, hipStream_t s) {
  BwdArgs a{x.q, x.p, x.D, x.group, arg, x.cols, G, ld_g, dq, dp};
  // the dq gathers read 4 columns at once: 8 bytes of fp16, 16 of fp32
  a.p.vec = aligned(x.p.x, x.p.ld_tok, x.p.ld_batch, val_esize(x.val_dt), 4 * val_esize(x.val_dt));
  // f(tag of the input type, tag of the gradient type)
  auto with_types = [&](auto&& f) { with_value_type(x.val_dt, [&](auto t) { with_value_type(grad_dt, [&](auto o) { f(t, o); }); }); };
  if (dq) {
    int tpr = 1;
    while (tpr * 4 < x.D) tpr *= 2;                      // D <= 1024: at most 256
    const dim3 grid((unsigned)(x.q.n * x.q.len));
    with_types([&](auto t, auto o) {
      hipLaunchKernelGGL((maxsim_bwd_q_kernel<typename decltype(t)::type, typename decltype(o)::type>), grid, dim3(256), 0, s, a, tpr);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (dp) {
    const dim3 grid((unsigned)x.p.n, (unsigned)((x.p.len + BWD_P_ROWS - 1) / BWD_P_ROWS), (unsigned)((x.D + BWD_P_COLS - 1) / BWD_P_COLS));
    with_types([&](auto t, auto o) {
      hipLaunchKernelGGL((maxsim_bwd_p_kernel<typename decltype(t)::type, typename decltype(o)::type>), grid, dim3(64), 0, s, a);
    });
  }
  return hipGetLastError();
}

// the checks the two entry points share; fills x
int check_problem(int32_t mem_kind, const void* q, int64_t ld_q_tok, int64_t ld_q_batch, int64_t A, int64_t Lq, const void* p, int64_t ld_p_tok,
                  int64_t ld_p_batch, int64_t B, int64_t Lp, int32_t D, int32_t value_dtype, int32_t group, Problem& x) {
  if (!q || !p) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!val_ok(value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (A < 0 || B < 0 || Lq <= 0 || Lp <= 0 || D <= 0 || group < 0) return set_error(DHR_ERR_INVALID, "bad sizes");
  if (ld_q_tok < D || ld_p_tok < D || ld_q_batch < D || ld_p_batch < D) return set_error(DHR_ERR_INVALID, "a stride is shorter than a row of D values");
  if (group > 0 && B != A * group)
    return set_error(DHR_ERR_INVALID, "maxsim scores: " + std::to_string(B) + " passage rows for " + std::to_string(A) + " queries x " +
                                          std::to_string(group) + " passages");
  if (D > MAX_D) return set_error(DHR_ERR_UNSUPPORTED, "maxsim scores: more than 1024 dims");
  if (Lp > MAX_LP) return set_error(DHR_ERR_UNSUPPORTED, "maxsim scores: more than 32767 passage tokens (the winning token is an int16)");
  if (A > MAX_BATCH || B > MAX_BATCH || Lq > MAX_LQ || A * Lq >= ((int64_t)1 << 31))
    return set_error(DHR_ERR_UNSUPPORTED, "maxsim scores: more than 131072 rows on a side, 65536 query tokens or 2^31 query tokens in all");
  const int es = val_esize(value_dtype);
  x.q = make_side(q, ld_q_tok, ld_q_batch, A, (int)Lq, es);
  x.p = make_side(p, ld_p_tok, ld_p_batch, B, (int)Lp, es);
  x.D = D; x.val_dt = value_dtype; x.group = group;
  x.cols = group > 0 ? group : B;
  return DHR_OK;
}

// a host [n][len][D] array with two strides -> a packed device copy
hipError_t stage_side(DevMem& m, Side& sd, int D, int es, hipStream_t s) {
  hipError_t e = dev_alloc(m, sd.n * sd.len * D * es);
  for (int64_t k = 0; k < sd.n && e == hipSuccess; ++k)
    e = copy_in((char*)m.p + k * sd.len * D * es, (const char*)sd.x + k * sd.ld_batch * es, sd.ld_tok, sd.len, D, es, s);
  sd = make_side(m.p, D, (int64_t)sd.len * D, sd.n, sd.len, es);
  return e;
}

}  // namespace

extern "C" int dhr_maxsim_scores(int32_t device, int32_t mem_kind, const void* q, int64_t ld_q_tok, int64_t ld_q_batch, int64_t A, int64_t Lq,
                                 const void* p, int64_t ld_p_tok, int64_t ld_p_batch, int64_t B, int64_t Lp, int32_t D, int32_t value_dtype,
                                 int32_t group, float* out, int64_t ld_out, int16_t* arg, void* stream) try {
  dhr::alloc_checkpoint();
  Problem x;
  if (!out) return set_error(DHR_ERR_INVALID, "null pointer");
  int rc = check_problem(mem_kind, q, ld_q_tok, ld_q_batch, A, Lq, p, ld_p_tok, ld_p_batch, B, Lp, D, value_dtype, group, x);
  if (rc) return rc;
  if (ld_out < x.cols) return set_error(DHR_ERR_INVALID, "ld_out is shorter than a row of scores");
  if (A == 0 || B == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_fwd(x, out, ld_out, arg, s));
    return DHR_OK;
  }
  const int es = val_esize(x.val_dt);
  DevMem m_q, m_p, m_out, m_arg;
  HIP_TRY(stage_side(m_q, x.q, D, es, s));
  HIP_TRY(stage_side(m_p, x.p, D, es, s));
  HIP_TRY(dev_alloc(m_out, A * x.cols * 4));
  if (arg) HIP_TRY(dev_alloc(m_arg, A * x.cols * Lq * 2));
  HIP_TRY(launch_fwd(x, (float*)m_out.p, x.cols, (int16_t*)m_arg.p, s));
  HIP_TRY(stage_out(out, ld_out, m_out.p, A, x.cols, 4, s));
  if (arg) HIP_TRY(hipMemcpyAsync(arg, m_arg.p, (size_t)(A * x.cols * Lq * 2), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_maxsim_scores_backward(int32_t device, int32_t mem_kind, const void* q, int64_t ld_q_tok, int64_t ld_q_batch, int64_t A,
                                          int64_t Lq, const void* p, int64_t ld_p_tok, int64_t ld_p_batch, int64_t B, int64_t Lp, int32_t D,
                                          int32_t value_dtype, int32_t group, const int16_t* arg, const float* grad_out, int64_t ld_grad,
                                          void* dq, void* dp, int32_t grad_dtype, void* stream) try {
  dhr::alloc_checkpoint();
  Problem x;
  if (!arg || !grad_out) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!val_ok(grad_dtype)) return set_error(DHR_ERR_INVALID, "bad gradient dtype");
  int rc = check_problem(mem_kind, q, ld_q_tok, ld_q_batch, A, Lq, p, ld_p_tok, ld_p_batch, B, Lp, D, value_dtype, group, x);
  if (rc) return rc;
  if (ld_grad < x.cols) return set_error(DHR_ERR_INVALID, "ld_grad is shorter than a row of scores");
  if (A == 0) dq = nullptr;
  if (B == 0) dp = nullptr;
  if (!dq && !dp) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int ges = val_esize(grad_dtype);
  const size_t dq_bytes = (size_t)(A * Lq * D * ges), dp_bytes = (size_t)(B * Lp * D * ges);
  if (A == 0 || B == 0) {                               // no scored pair: the side that has rows gets zeros
    void* dst = dq ? dq : dp;
    const size_t bytes = dq ? dq_bytes : dp_bytes;
    if (mem_kind == DHR_MEM_DEVICE) HIP_TRY(hipMemsetAsync(dst, 0, bytes, s));
    else memset(dst, 0, bytes);
    return DHR_OK;
  }
  if (mem_kind == DHR_MEM_DEVICE) {
    HIP_TRY(launch_bwd(x, arg, grad_out, ld_grad, dq, dp, grad_dtype, s));
    return DHR_OK;
  }
  const int es = val_esize(x.val_dt);
  DevMem m_q, m_p, m_arg, m_g, m_dq, m_dp;
  HIP_TRY(stage_side(m_q, x.q, D, es, s));
  HIP_TRY(stage_side(m_p, x.p, D, es, s));
  HIP_TRY(stage_in(m_arg, arg, x.cols * Lq, A, x.cols * Lq, 2, s));
  HIP_TRY(stage_in(m_g, grad_out, ld_grad, A, x.cols, 4, s));
  if (dq) HIP_TRY(dev_alloc(m_dq, (int64_t)dq_bytes));
  if (dp) HIP_TRY(dev_alloc(m_dp, (int64_t)dp_bytes));
  HIP_TRY(launch_bwd(x, (const int16_t*)m_arg.p, (const float*)m_g.p, x.cols, m_dq.p, m_dp.p, grad_dtype, s));
  if (dq) HIP_TRY(hipMemcpyAsync(dq, m_dq.p, dq_bytes, hipMemcpyDeviceToHost, s));
  if (dp) HIP_TRY(hipMemcpyAsync(dp, m_dp.p, dp_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

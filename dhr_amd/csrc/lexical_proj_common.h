// What lexical_proj.hip (encoding) and lexical_proj_train.hip (training) share: the arguments, the compaction of the unmasked token rows, the
// staged MFMA tile product, the softmax statistics pass with its combine, and the fold; on the host the operand rules, the workspace rule and
// the one place that fills ProjArgs (the workspace layout itself: lexical_proj_layout.h).  One definition each, so the training forward is
// bit-identical to the encoding one.  The kernels that touch hidden / weight are templates on their 16-bit element type E (_Float16 or __bf16):
// the staging moves bytes, the fragment layouts of v_mfma_f32_32x32x16_f16 and _bf16 are the same, so tiling, walk and reduction order are common.
#pragma once
#include "lexical_common.h"
#include "lexical_proj_layout.h"
#include "op_dispatch.h"

// Internal linkage on purpose: each translation unit that includes this header compiles its own copy of the kernels below, the non-template
// ones (count, scan, fill, statistics, combine) included.  The duplication costs code size only and keeps the launches free of cross-unit symbols.
namespace {

// (TM, TN and the split constants: lexical_proj_layout.h)
constexpr int BK = 64;                 // columns of H staged per step (128 bytes of a row)
constexpr int PITCH = 2 * BK + 16;     // LDS pitch of a staged row: the 16-byte reads of 16 consecutive rows fall on 16 different slots
constexpr int GROUP_ROWS = 1024;       // token rows (before masking) a fold workgroup owns at least
constexpr int MAX_TOKENS = 32767;      // training: tok is int16
constexpr int MAX_H = 1024;            // training: the widest hidden size whose gradient kernels are built

typedef float float16v __attribute__((ext_vector_type(16)));

struct ProjArgs {
  const _Float16* hid;                 // of the kernel's element type E (read as const E*: a 16-bit type either way), strides in elements
  int64_t ld_hb, ld_ht;
  const _Float16* wgt;
  int64_t ld_w;
  const void* bias;                    // NULL: none; fp32, or E like hid and wgt, or ...
  int bias_f32;
  int bias_f16;                        // ... fp16 next to bf16 operands (E = __bf16 alone; the fp16 kernels read fp32 or fp16, as they always did)
  const float* tw;
  int64_t ld_tw;
  const float* mask;
  int64_t ld_mask;
  int64_t B;
  int T, H, V;
  int vec_h, vec_w;                    // 16-byte loads are aligned
  int n_split, n_ntiles, group;        // shares / vocabulary tiles of the statistics pass; passages per fold workgroup
  int* hdr;                            // [0]: unmasked token rows M
  int* cnt;                            // [B] unmasked tokens
  int* start;                          // [B + 1] first row of a passage in the list
  int* tmask;                          // [B] first masked token, -1: none
  int* rows;                           // [M] b * T + t
  float4* stats;                       // [M] (max, sum, w, mask)
  float2* part;                        // [n_split][B * T] (max, sum)
  float* reps;
  int64_t ld_reps;
  int16_t* tok;                        // training only: [B, V] the first maximising token and its p
  int64_t ld_tok;
  float* pwin;
  int64_t ld_pwin;
};

// the dtype of the bias, or of an output of the training backward, as the flag pair the kernels read: fp32, fp16, neither (then it is E)
inline void dtype_flags(int val_dtype, int& f32, int& f16) { f32 = val_dtype == DHR_VAL_F32; f16 = val_dtype == DHR_VAL_F16; }

__global__ void __launch_bounds__(64) proj_count_kernel(ProjArgs a) {
  const int64_t b = blockIdx.x;
  const float* m = a.mask + b * a.ld_mask;
  int n = 0, first = a.T;
  for (int t = threadIdx.x; t < a.T; t += 64) {
    if (m[t] != 0.f) ++n;
    else first = min(first, t);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    first = min(first, __shfl_xor(first, o, 64));
  }
  if (threadIdx.x == 0) {
    a.cnt[b] = n;
    a.tmask[b] = first < a.T ? first : -1;
  }
}

// one workgroup: start[b] = the unmasked tokens of the passages before b, start[B] = hdr[0] = all of them
__global__ void __launch_bounds__(256) proj_scan_kernel(ProjArgs a) {
  __shared__ int sums[256];
  const int64_t per = (a.B + 255) / 256;
  const int64_t lo = min(a.B, (int64_t)threadIdx.x * per), hi = min(a.B, lo + per);
  int s = 0;
  for (int64_t b = lo; b < hi; ++b) s += a.cnt[b];
  sums[threadIdx.x] = s;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) base += sums[k];
  for (int64_t b = lo; b < hi; ++b) {
    a.start[b] = base;
    base += a.cnt[b];
  }
  if (threadIdx.x == 255) {
    a.start[a.B] = base;
    a.hdr[0] = base;
  }
}

__global__ void __launch_bounds__(64) proj_fill_kernel(ProjArgs a) {
  const int64_t b = blockIdx.x;
  const float* m = a.mask + b * a.ld_mask;
  int* out = a.rows + a.start[b];
  int base = 0;
  for (int t0 = 0; t0 < a.T; t0 += 64) {
    const int t = t0 + threadIdx.x;
    const bool on = t < a.T && m[t] != 0.f;
    const unsigned long long live = __ballot(on);
    if (on) out[base + __popcll(live & ((1ull << threadIdx.x) - 1))] = (int)(b * a.T + t);
    base += __popcll(live);
  }
}

template <typename E>
__device__ __forceinline__ uint4 load16h(const E* p, bool vec) {
  if (vec) return *reinterpret_cast<const uint4*>(p);
  union { uint4 u; E t[8]; } r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r.t[e] = p[e];
  return r.u;
}

template <typename E>
__device__ __forceinline__ float bias_at(const ProjArgs& a, int v) {
  if (!a.bias) return 0.f;
  if constexpr (__is_same(E, __bf16))
    if (a.bias_f16) return (float)((const _Float16*)a.bias)[v];
  return a.bias_f32 ? ((const float*)a.bias)[v] : (float)((const E*)a.bias)[v];
}


// The product of 64 staged rows `hrow` (thread t stages 16-byte slot t & 7 of rows (t >> 3) + 32 u; LDS rows [0, TM)) and 256 staged rows
// `wrow` (LDS rows [TM, TM + TN)) over all of H.  The caller clamps rows beyond the problem to a valid one (their results are never used);
// columns beyond H are zeros.  W_REG: acc[i][j][k] holds w-row wave * 64 + 32 i + (8 (k >> 2) + 4 h + (k & 3)) against h-row 32 j + r;
// otherwise h-row 32 i + (...) against w-row wave * 64 + 32 j + r (r = lane & 31, h = lane >> 5, k the accumulator register).
template <typename E, bool W_REG>
__device__ __forceinline__ void tile_product_rows(unsigned char* lds, int H, const E* const (&hrow)[2], int vec_h, const E* const (&wrow)[TN / 32],
                                                  int vec_w, float16v (&acc)[2][2]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int slot = tid & 7, rb = tid >> 3;
  uint4 sh[2], sw[TN / 32];
  auto fetch = [&](int chunk) {
    const int col = chunk * BK + slot * 8;
    const bool in = col < H;                              // H is a multiple of 8: a slot is inside or outside as a whole
    const int c = in ? col : 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sh[u] = load16h(hrow[u] + c, vec_h);
      if (!in) sh[u] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < TN / 32; ++u) {
      sw[u] = load16h(wrow[u] + c, vec_w);
      if (!in) sw[u] = make_uint4(0u, 0u, 0u, 0u);
    }
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;
  const int n_chunks = (H + BK - 1) / BK;
  fetch(0);
  for (int chunk = 0; chunk < n_chunks; ++chunk) {
#pragma unroll
    for (int u = 0; u < 2; ++u) *reinterpret_cast<uint4*>(lds + (rb + 32 * u) * PITCH + slot * 16) = sh[u];
#pragma unroll
    for (int u = 0; u < TN / 32; ++u) *reinterpret_cast<uint4*>(lds + (TM + rb + 32 * u) * PITCH + slot * 16) = sw[u];
    __syncthreads();
    if (chunk + 1 < n_chunks) fetch(chunk + 1);
    const int k_steps = min(BK / 16, (H - chunk * BK + 15) / 16);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      if (s < k_steps) {                                   // (uniform)
        typedef typename Vec<E>::type frag;
        frag hf[2], wf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          hf[i] = *reinterpret_cast<const frag*>(lds + (32 * i + r) * PITCH + s * 32 + h * 16);
          wf[i] = *reinterpret_cast<const frag*>(lds + (TM + wave * 64 + 32 * i + r) * PITCH + s * 32 + h * 16);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            // the builtin is named here, not behind an overloaded helper: with one, the fp16 fold kernel took another register assignment
            if constexpr (__is_same(E, __bf16))
              acc[i][j] = W_REG ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], hf[j], acc[i][j], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_32x32x16_bf16(hf[i], wf[j], acc[i][j], 0, 0, 0);
            else
              acc[i][j] = W_REG ? __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i], hf[j], acc[i][j], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_32x32x16_f16(hf[i], wf[j], acc[i][j], 0, 0, 0);
          }
      }
    }
    __syncthreads();
  }
#endif
}

// tile_product_rows of the token rows hrow and the weight rows [n0, n0 + TN): TOK_LANE puts the token on the lane (weight rows in the
// registers), otherwise the token rows are in the registers and the weight row is on the lane
template <typename E, bool TOK_LANE>
__device__ __forceinline__ void tile_product(unsigned char* lds, const ProjArgs& a, const E* const (&hrow)[2], int n0, float16v (&acc)[2][2]) {
  const int rb = threadIdx.x >> 3;
  const E* wrow[TN / 32];
#pragma unroll
  for (int u = 0; u < TN / 32; ++u) wrow[u] = (const E*)a.wgt + (int64_t)min(n0 + rb + 32 * u, a.V - 1) * a.ld_w;
  tile_product_rows<E, TOK_LANE>(lds, a.H, hrow, a.vec_h, wrow, a.vec_w, acc);
}

// (max, sum exp(x - max)) of two disjoint parts of a row -> of their union; a part without a column is (-inf, 0)
__device__ __forceinline__ void softmax_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  const float a = m == -INFINITY ? 0.f : s * expf(m - mm);
  const float b = m2 == -INFINITY ? 0.f : s2 * expf(m2 - mm);
  m = mm;
  s = a + b;
}

// the pointers of the two token rows a thread stages: rows row0 + (t >> 3) + 32 u of the list, clamped to [.., row_end)
template <typename E>
__device__ __forceinline__ void token_rows(const ProjArgs& a, int row0, int row_end, const E* (&hrow)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int id = a.rows[min(row0 + (int)(threadIdx.x >> 3) + 32 * u, row_end - 1)];
    const int b = id / a.T, t = id - b * a.T;
    hrow[u] = (const E*)a.hid + (int64_t)b * a.ld_hb + (int64_t)t * a.ld_ht;
  }
}

// grid: (tiles of TM rows of the worst-case list, shares of the vocabulary)
template <typename E>
__global__ void __launch_bounds__(256) proj_stats_kernel(ProjArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[(TM + TN) * PITCH];
  __shared__ float sh_bias[TN];
  __shared__ float2 sh_red[4][TM];
  const int M = a.hdr[0];
  const int m0 = blockIdx.x * TM;
  if (m0 >= M) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const E* hrow[2];
  token_rows(a, m0, M, hrow);
  const int nt_lo = (int)((int64_t)blockIdx.y * a.n_ntiles / a.n_split), nt_hi = (int)((int64_t)(blockIdx.y + 1) * a.n_ntiles / a.n_split);
  float m_run[2] = {-INFINITY, -INFINITY}, s_run[2] = {0.f, 0.f};
  for (int nt = nt_lo; nt < nt_hi; ++nt) {
    const int n0 = nt * TN;
    sh_bias[tid] = n0 + tid < a.V ? bias_at<E>(a, n0 + tid) : -INFINITY;      // a column beyond the vocabulary: x = -inf, exp = 0
    float16v acc[2][2];
    tile_product<E, true>(tile, a, hrow, n0, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float t_max = -INFINITY;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          acc[i][j][k] += sh_bias[wave * 64 + 32 * i + 8 * (k >> 2) + 4 * h + (k & 3)];
          t_max = fmaxf(t_max, acc[i][j][k]);
        }
      if (t_max > -INFINITY) {
        const float m_new = fmaxf(m_run[j], t_max);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int k = 0; k < 16; ++k) sum += expf(acc[i][j][k] - m_new);
        s_run[j] = s_run[j] * expf(m_run[j] - m_new) + sum;
        m_run[j] = m_new;
      }
    }
    __syncthreads();                                                       // sh_bias is rewritten by the next tile
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {                                            // the lane halves: h = 0 first
    const float om = __shfl_xor(m_run[j], 32, 64), os = __shfl_xor(s_run[j], 32, 64);
    float m = h ? om : m_run[j], s = h ? os : s_run[j];
    softmax_merge(m, s, h ? m_run[j] : om, h ? s_run[j] : os);
    if (h == 0) sh_red[wave][32 * j + r] = make_float2(m, s);
  }
  __syncthreads();
  if (tid < TM && m0 + tid < M) {
    float m = sh_red[0][tid].x, s = sh_red[0][tid].y;
    for (int w = 1; w < 4; ++w) softmax_merge(m, s, sh_red[w][tid].x, sh_red[w][tid].y);   // in wave order
    a.part[(int64_t)blockIdx.y * (a.B * a.T) + m0 + tid] = make_float2(m, s);
  }
}

__global__ void __launch_bounds__(256) proj_combine_kernel(ProjArgs a) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= a.hdr[0]) return;
  const int id = a.rows[row];
  const int64_t b = id / a.T;
  const int t = id - (int)b * a.T;
  const int64_t ld = a.B * a.T;
  float m = -INFINITY;
  for (int k = 0; k < a.n_split; ++k) m = fmaxf(m, a.part[k * ld + row].x);
  double s = 0.0;                                        // in share order, fp64: rounded to fp32 once
  for (int k = 0; k < a.n_split; ++k) {
    const float2 p = a.part[k * ld + row];
    if (p.x > -INFINITY) s += (double)p.y * exp((double)p.x - (double)m);
  }
  a.stats[row] = make_float4(m, (float)s, a.tw[b * a.ld_tw + t], a.mask[b * a.ld_mask + t]);
}

enum { ROW_LIVE = 1, ROW_FIRST = 2, ROW_LAST = 4, ROW_Z_BEFORE = 8, ROW_Z_AFTER = 16 };

// grid: (blocks of TN vocabulary columns, groups of a.group passages).  TRAIN: also the first maximising token of every (passage, column),
// counted like the mask's columns, and its p (a masked token that wins is named like any other, with p = 0: it is never multiplied)
template <typename E, bool TRAIN>
__global__ void __launch_bounds__(256) proj_fold_kernel(ProjArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) unsigned char tile[(TM + TN) * PITCH];
  __shared__ float4 sh_st[TM];
  __shared__ int sh_flag[TM];
  __shared__ float sh_z[TM];
  __shared__ int sh_b[TM];
  __shared__ int sh_t[TM], sh_tm[TM];                    // TRAIN: the row's token and its passage's first masked token
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int n0 = blockIdx.x * TN, col = n0 + tid;        // after the swap a lane owns column wave * 64 + lane of the block
  const bool col_on = col < a.V;
  const float bias = col_on ? bias_at<E>(a, col) : 0.f;
  const int64_t b_lo = (int64_t)blockIdx.y * a.group, b_hi = min(a.B, b_lo + a.group);
  const int row_lo = a.start[b_lo], row_hi = a.start[b_hi];
  if (col_on)
    for (int64_t b = b_lo; b < b_hi; ++b)                // a fully masked passage: its first token's zero
      if (a.cnt[b] == 0) {
        a.reps[b * a.ld_reps + col] = (1.f * a.tw[b * a.ld_tw]) * 0.f;
        if (TRAIN) {
          a.tok[b * a.ld_tok + col] = 0;
          a.pwin[b * a.ld_pwin + col] = 0.f;
        }
      }
  float best = 0.f, best_p = 0.f;
  int best_t = 0;
  for (int m0 = row_lo; m0 < row_hi; m0 += TM) {
    if (tid < TM) {
      const int row = m0 + tid;
      int flag = 0, bb = 0, tt = 0, tmm = 0;
      float z = 0.f;
      float4 st = make_float4(0.f, 1.f, 0.f, 0.f);
      if (row < row_hi) {
        const int id = a.rows[row];
        bb = id / a.T;
        const int t = id - bb * a.T;
        const int first = row == a.start[bb], last = row == a.start[bb + 1] - 1;
        const int tm = a.tmask[bb];
        tt = t; tmm = tm;
        const int t_prev = first ? -1 : a.rows[row - 1] - bb * a.T;
        st = a.stats[row];
        flag = ROW_LIVE | (first ? ROW_FIRST : 0) | (last ? ROW_LAST : 0);
        if (tm >= 0) {
          z = (1.f * a.tw[(int64_t)bb * a.ld_tw + tm]) * 0.f;                 // (p * w) * 0 with p finite and positive
          if (t_prev < tm && tm < t) flag |= ROW_Z_BEFORE;
          if (last && tm > t) flag |= ROW_Z_AFTER;
        }
      }
      sh_st[tid] = st; sh_flag[tid] = flag; sh_z[tid] = z; sh_b[tid] = bb;
      if (TRAIN) { sh_t[tid] = tt; sh_tm[tid] = tmm; }
    }
    const E* hrow[2];
    token_rows(a, m0, row_hi, hrow);
    float16v acc[2][2];
    tile_product<E, false>(tile, a, hrow, n0, acc);         // (its first barrier publishes the row table)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // rows 32 i + 8 q + 4 hh + e: lane half hh computed them for both column tiles; half h keeps tile h and takes the other half's
        float lo[4], hi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float own = h ? acc[i][1][4 * q + e] : acc[i][0][4 * q + e];
          const float send = h ? acc[i][0][4 * q + e] : acc[i][1][4 * q + e];
          const float recv = __shfl_xor(send, 32, 64);
          lo[e] = h ? recv : own;
          hi[e] = h ? own : recv;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int row = 32 * i + 8 * q + u;
          const int flag = __builtin_amdgcn_readfirstlane(sh_flag[row]);
          if (!(flag & ROW_LIVE)) continue;
          const float4 s = sh_st[row];
          const float x = (u < 4 ? lo[u & 3] : hi[u & 3]) + bias;
          const float p = expf(x - s.x) / s.y;
          const float c = (p * s.z) * s.w;
          if (flag & ROW_FIRST) best = -INFINITY;
          if (flag & ROW_Z_BEFORE) {
            const float z = sh_z[row];
            if (z > best) {
              best = z;
              if (TRAIN) { best_t = sh_tm[row]; best_p = 0.f; }
            }
          }
          if (c > best) {                                 // strict: the first token keeps a tie (the sign of a zero maximum)
            best = c;
            if (TRAIN) { best_t = sh_t[row]; best_p = p; }
          }
          if (flag & ROW_LAST) {
            if (flag & ROW_Z_AFTER) {
              const float z = sh_z[row];
              if (z > best) {
                best = z;
                if (TRAIN) { best_t = sh_tm[row]; best_p = 0.f; }
              }
            }
            if (col_on) {
              a.reps[(int64_t)sh_b[row] * a.ld_reps + col] = best;
              if (TRAIN) {
                a.tok[(int64_t)sh_b[row] * a.ld_tok + col] = (int16_t)best_t;
                a.pwin[(int64_t)sh_b[row] * a.ld_pwin + col] = best_p;
              }
            }
          }
        }
      }
    }
    __syncthreads();                                      // the row table is rewritten by the next tile
  }
}

// The operands of a projection head as its entry point received them (n_tokens counts the tokens after the skipped ones; encoding skips none).
struct ProjOperands {
  int32_t mem_kind; const void* hidden; int32_t value_dtype; int64_t batch; int32_t n_tokens, skip_tokens, hidden_dim; int64_t ld_batch, ld_token;
  const void* weight; int32_t vocab; int64_t ld_weight; const void* bias; int32_t bias_dtype;
  const float* term_weights; int64_t ld_weights; const float* mask; int64_t ld_mask;
  void* workspace; int64_t workspace_bytes;
};

// The operand rules of the three entry points, before anything is dereferenced.  `what` prefixes the messages.  The training calls
// (train = true) add the limits of their kernels and answer the operand types and host memory last; the encoding call refuses everything but
// device memory at once and answers the operand types before the sizes.  more_dtypes_ok / more_sizes_ok: the caller's own arguments that
// answer with the same two messages (the record's value dtype and cls_dim of the encoding call).
inline int check_operands(const char* what, bool train, const ProjOperands& o, bool more_dtypes_ok = true, bool more_sizes_ok = true) {
  auto operand_types = [&]() -> int {
    if (o.value_dtype == DHR_VAL_F32) return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": hidden states and weight must be fp16 or bf16");
    if (o.bias && o.bias_dtype == DHR_VAL_BF16 && o.value_dtype == DHR_VAL_F16)
      return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": a bf16 bias needs bf16 hidden states and weight (the fp16 kernels read fp32 or fp16)");
    return DHR_OK;
  };
  if (!o.hidden || !o.weight || !o.term_weights || !o.mask) return set_error(DHR_ERR_INVALID, "null pointer");
  if (train && !DHR_MEM_KIND_OK(o.mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (!train && o.mem_kind != DHR_MEM_DEVICE) return set_error(DHR_ERR_INVALID, std::string(what) + ": device memory only");
  if (!val_ok_bf16(o.value_dtype) || (o.bias && !val_ok_bf16(o.bias_dtype)) || !more_dtypes_ok) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (!train)
    if (int rc = operand_types()) return rc;
  const int64_t L = (int64_t)o.n_tokens + o.skip_tokens;
  if (o.batch < 0 || o.n_tokens <= 0 || o.vocab <= 0 || o.hidden_dim <= 0 || o.skip_tokens < 0 || o.skip_tokens > MAX_TOKENS ||
      o.ld_token < o.hidden_dim || o.ld_batch < (L - 1) * o.ld_token + o.hidden_dim || o.ld_weight < o.hidden_dim || o.ld_weights < o.n_tokens ||
      o.ld_mask < o.n_tokens || !more_sizes_ok || o.workspace_bytes < 0 || o.batch * L > ((int64_t)1 << 31) - 1)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (o.hidden_dim % 8) return set_error(DHR_ERR_INVALID, "the hidden size must be a multiple of 8");
  if (!train) return DHR_OK;
  if (o.n_tokens > MAX_TOKENS) return set_error(DHR_ERR_UNSUPPORTED, "more than 32767 tokens (the token index is int16)");
  if (o.hidden_dim > MAX_H) return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": hidden sizes above 1024 are not built");
  if (int rc = operand_types()) return rc;
  if (o.mem_kind != DHR_MEM_DEVICE)
    return set_error(DHR_ERR_UNSUPPORTED, std::string(what) + ": host arrays are not staged, training tensors live on the device (DHR_MEM_DEVICE)");
  return DHR_OK;
}

// the workspace rule of the three entry points; size_fn names the function that returns `total`
inline int check_workspace(const char* size_fn, int64_t total, const ProjOperands& o) {
  if (!o.workspace || o.workspace_bytes < total)
    return set_error(DHR_ERR_INVALID, std::string("workspace is smaller than ") + size_fn + " (" + std::to_string(total) + " bytes)");
  if ((uintptr_t)o.workspace % 16) return set_error(DHR_ERR_INVALID, "workspace must be aligned to 16 bytes");
  return DHR_OK;
}

// ProjArgs of the operands and the shared sections of the workspace; the caller adds its outputs (reps, and tok / pwin when training)
inline ProjArgs proj_args(const ProjLayout& l, const ProjOperands& o) {
  char* ws = (char*)o.workspace;
  ProjArgs a{};
  a.hid = (const _Float16*)o.hidden + (int64_t)o.skip_tokens * o.ld_token; a.ld_hb = o.ld_batch; a.ld_ht = o.ld_token;
  a.wgt = (const _Float16*)o.weight; a.ld_w = o.ld_weight;
  a.bias = o.bias; dtype_flags(o.bias_dtype, a.bias_f32, a.bias_f16);
  a.tw = o.term_weights; a.ld_tw = o.ld_weights; a.mask = o.mask; a.ld_mask = o.ld_mask;
  a.B = o.batch; a.T = o.n_tokens; a.H = o.hidden_dim; a.V = o.vocab;
  a.vec_h = (uintptr_t)a.hid % 16 == 0 && o.ld_batch % 8 == 0 && o.ld_token % 8 == 0;
  a.vec_w = (uintptr_t)o.weight % 16 == 0 && o.ld_weight % 8 == 0;
  a.n_split = l.n_split; a.n_ntiles = l.n_ntiles;
  a.group = (int)std::max<int64_t>((GROUP_ROWS + o.n_tokens - 1) / o.n_tokens, (o.batch + 65534) / 65535);
  a.hdr = (int*)(ws + l.hdr); a.cnt = (int*)(ws + l.cnt); a.start = (int*)(ws + l.start); a.tmask = (int*)(ws + l.tmask);
  a.rows = (int*)(ws + l.rows); a.stats = (float4*)(ws + l.stats); a.part = (float2*)(ws + l.part);
  return a;
}

// the forward of both heads on a filled ProjArgs: compaction of the unmasked rows, statistics, combine, fold (TRAIN: with tok and pwin).
// value_dtype is DHR_VAL_F16 or DHR_VAL_BF16; the caller asks hipGetLastError()
template <bool TRAIN>
void launch_forward(int value_dtype, const ProjArgs& a, hipStream_t s) {
  const int64_t BT = a.B * a.T;
  hipLaunchKernelGGL(proj_count_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
  hipLaunchKernelGGL(proj_scan_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(proj_fill_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
  const dim3 g_stats((unsigned)((BT + TM - 1) / TM), (unsigned)a.n_split), g_fold((unsigned)a.n_ntiles, (unsigned)((a.B + a.group - 1) / a.group));
  with_half_type(value_dtype, [&](auto t) { hipLaunchKernelGGL(proj_stats_kernel<typename decltype(t)::type>, g_stats, dim3(256), 0, s, a); });
  hipLaunchKernelGGL(proj_combine_kernel, dim3((unsigned)((BT + 255) / 256)), dim3(256), 0, s, a);
  with_half_type(value_dtype, [&](auto t) { hipLaunchKernelGGL((proj_fold_kernel<typename decltype(t)::type, TRAIN>), g_fold, dim3(256), 0, s, a); });
}

}  // namespace

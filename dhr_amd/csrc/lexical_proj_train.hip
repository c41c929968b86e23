// The lexical head of a TRAINING step with the vocabulary projection fused in, forward and backward.  lexical_train.hip starts from the MLM
// logits [B, L, V] and writes their gradient; here the op starts from the projector's input (hidden [B, L, H], weight [V, H], bias [V]) and
// returns the gradients of those: nothing of size B * T * V exists, forward or backward.  With r the unmasked token rows (b, t) of the list
// that lexical_proj_common.h compacts,
//   x[r][v] = hidden[r] . W[v] + bias[v],  p = softmax_v(x),  c = (p * w) * m,  reps[b][v] = max_t c at the first maximising token tok[b][v]
//   A[r] = sum over {v : tok[b][v] == t} of g[b][v] * p[r][v],   dL/dw[b][t] = m * A,   D[r] = w * m * A
//   dx[r][v] = p[r][v] * ([tok[b][v] == t] * g[b][v] * w * m - D[r])                                  (registers and LDS only)
//   dhidden[r][k] = sum_v dx[r][v] W[v][k],   dW[v][k] = sum_r dx[r][v] hidden[r][k],   dbias[v] = sum_r dx[r][v]
// Forward: the passes of the encoding op (count / scan / fill, statistics, combine, fold); the fold also writes tok and pwin, the p of the
// winning token.  The row list, the per-passage starts and the per-row statistics stay in the workspace for the backward.
// Backward:
//   proj_route_sum_kernel   pass 1: A as a segmented sum of g * pwin over the columns routed to each token (no GEMM): the scan of
//                           lexical_route_sum_kernel, fp64 slots added in a fixed order, rounded once.  Writes dL/dw and D.
//   proj_grad_kernel<2>     pass 2, dhidden: a workgroup owns 64 token rows and walks the vocabulary 256 columns at a time (a share of it when
//                           there are few token rows; proj_grad_combine_kernel then adds the shares in order).
//   proj_grad_kernel<3>     pass 3, dW and dbias: a workgroup owns 64 vocabulary columns and walks all token rows of the list, 256 at a time.
// Both GEMM passes are one kernel with the roles of the two operands exchanged.  Every kernel that reads hidden / weight is a
// template on their element type E (_Float16 or __bf16), with the staging, the tiling and every order of summation in common.
// Per walked tile: (1) x on v_mfma_f32_32x32x16_f16 (_bf16 where E is __bf16) with the
// owned ("resident") row on the lane and the walked rows in the accumulator registers -- the token on the lane in pass 2, the vocabulary
// column on the lane in pass 3; (2) dx in fp32 in those registers, rounded to E once and passed through LDS once, as [resident][walked];
// (3) a second MFMA chain out[resident][H] += dx . (walked operand), for which the walked operand's LDS image is staged again chunk by chunk
// and read by columns; the four waves split each 64 x 64 block of the output, whose accumulators stay in registers for the whole walk
// (16 per 64 columns of H: 192 at H = 768; a wider H is cut into two slabs, each of which computes x again).  One workgroup owns its rows of the output: no atomics, no float atomics
// anywhere, every sum in a fixed order -- two runs are bit-identical.  dbias is the fp32 sum of the unrounded dx.
// Everything is enqueued on the caller's stream; nothing is allocated.  NaN / inf inputs are out of scope.
#include "op_dispatch.h"
#include "lexical_proj_common.h"

namespace {

constexpr int RT_BIG = 16;             // tokens per workgroup of the route sums ...
constexpr int RT_SMALL = 4;            // ... and where 16 would leave most of the chip without a workgroup
constexpr int DXP = 2 * TN + 16;       // LDS pitch of a row of the dx image [resident 64][walked 256] of E
constexpr int MAX_CHUNKS = 12;         // 64-column chunks of H whose output accumulators fit the registers: 16 registers per chunk

struct GradArgs {
  const float* g;                      // dL/dreps [B, V]
  int64_t ld_g;
  const int16_t* tok;
  int64_t ld_tok;
  const float* D;                      // [B * T] w * m * A
  void* out;                           // pass 2: dhidden at the first unskipped token; pass 3: dW (NULL: dbias only)
  int out_f32, out_f16;                // the dtype of out: fp32, fp16 next to bf16 operands (E = __bf16 alone), else E
  int64_t ld_ob, ld_ot;                // pass 2: batch / token strides; pass 3: ld_ob is the row stride
  void* dbias;                         // pass 3, NULL: not wanted
  int dbias_f32, dbias_f16;
  float* partial;                      // pass 2 with shares: [n_split][B * T][H] fp32
  int n_split;
  int c_lo, c_n;                       // the slab of H this launch owns: 64-column chunks [c_lo, c_lo + c_n)
};

// A[b][t] of RT tokens of one passage -> dL/dw = m * A and D = (w * m) * A.  grid: (tiles of RT tokens, passages)
template <int RT>
__global__ void __launch_bounds__(256) proj_route_sum_kernel(const float* __restrict__ g, int64_t ld_g, const int16_t* __restrict__ tok, int64_t ld_tok,
                                                             const float* __restrict__ pwin, int64_t ld_pwin, const float* __restrict__ tw,
                                                             int64_t ld_tw, const float* __restrict__ mask, int64_t ld_mask, int T, int V,
                                                             float* __restrict__ D, float* __restrict__ dw, int64_t ld_dw) {
  constexpr int U = 8;                                   // columns a thread has in flight
  __shared__ double acc[RT][256];
  const int64_t b = blockIdx.y;
  const int t0 = blockIdx.x * RT;
  const int nt = min(RT, T - t0);
#pragma unroll
  for (int k = 0; k < RT; ++k) acc[k][threadIdx.x] = 0.0;
  const float* gb = g + b * ld_g;
  const float* pb = pwin + b * ld_pwin;
  const int16_t* tb = tok + b * ld_tok;
  for (int base = threadIdx.x; base < V; base += 256 * U) {
    int k[U];
    float pv[U], gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) k[u] = (int)tb[min(base + 256 * u, V - 1)] - t0;
#pragma unroll
    for (int u = 0; u < U; ++u) {                          // unconditional loads at clamped addresses: a thread's U columns are in flight together
      const int v = base + 256 * u;
      if (v >= V || k[u] < 0 || k[u] >= nt) k[u] = -1;
      pv[u] = pb[min(v, V - 1)];
      gv[u] = gb[min(v, V - 1)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)                            // a thread's columns in increasing order
      if (k[u] >= 0) acc[k[u]][threadIdx.x] += (double)gv[u] * (double)pv[u];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < nt; k += 4) {
    double s = ((acc[k][lane] + acc[k][lane + 64]) + acc[k][lane + 128]) + acc[k][lane + 192];
    s = wave_sum(s);
    if (lane == 0) {
      const float a = (float)s;
      const float w = tw[b * ld_tw + t0 + k], m = mask[b * ld_mask + t0 + k];
      D[b * T + t0 + k] = (w * m) * a;
      if (dw) dw[b * ld_dw + t0 + k] = m * a;
    }
  }
}

// the rows of dhidden that no workgroup of pass 2 owns, skipped and masked tokens: exact zeros.  grid: B * (skip + T) rows
__global__ void __launch_bounds__(256) proj_zero_rows_kernel(ProjArgs a, void* out, int out_f32, int64_t ld_ob, int64_t ld_ot, int skip) {
  const int L = skip + a.T;
  const int64_t b = blockIdx.x / L;
  const int l = (int)(blockIdx.x - b * L);
  if (l >= skip && a.mask[b * a.ld_mask + l - skip] != 0.f) return;
  const int64_t at = b * ld_ob + (int64_t)l * ld_ot;
  for (int k = threadIdx.x; k < a.H; k += 256) {
    if (out_f32) ((float*)out)[at + k] = 0.f;
    else ((unsigned short*)out)[at + k] = 0;             // +0 of fp16 and of bf16
  }
}

typedef short short4t __attribute__((__vector_size__(4 * sizeof(short))));

// ds_read_b64_tr_b16: every lane of the wave must be active
__device__ __forceinline__ short4t lds_read_tr16(const unsigned char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4t*)p);
#else
  return short4t{};
#endif
}

// a gradient, rounded once (to nearest even): fp32, or of the operands' type E, or (f16: E = __bf16 alone) fp16 next to bf16 operands.  The
// fp16 kernels keep the two-way store they always had; the bf16 kernels convert both ways and select, which keeps the stores two-way as well
// (a branch per store on a third case costs the widest gradient kernel its registers: it spills).
template <typename E>
__device__ __forceinline__ void store_out(void* out, int f32, int f16, int64_t at, float v) {
  if (f32) {
    ((float*)out)[at] = v;
  } else if constexpr (__is_same(E, __bf16)) {
    union { _Float16 f; unsigned short u; } h;
    union { __bf16 f; unsigned short u; } b;
    h.f = (_Float16)v;
    b.f = (__bf16)v;
    ((unsigned short*)out)[at] = f16 ? h.u : b.u;
  } else {
    ((E*)out)[at] = (E)v;
  }
}

// PASS 2: resident = 64 rows of the token list (grid x), walked = a share (grid y) of the vocabulary; out = dhidden.
// PASS 3: resident = 64 vocabulary columns (grid x), walked = the token list; out = dW, and dbias.
// NC: 64-column chunks of H the output registers hold (>= q.c_n, the chunks of the launch's slab of H).
template <typename E, int PASS, int NC>
__global__ void __launch_bounds__(256) proj_grad_kernel(ProjArgs a, GradArgs q) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) unsigned char tile[(TM + TN) * PITCH];
  __shared__ __attribute__((aligned(16))) unsigned char dxs[TM * DXP];
  __shared__ float4 sh_st[TN];                           // per token slot: (max, sum, w * m, D)
  __shared__ int2 sh_bt[TN];                             // (passage, token); token -1: no such row
  __shared__ int64_t sh_off[TN];                         // pass 3: where the slot's row of hidden starts (a row past the list: the last one's)
  __shared__ float sh_bias[TN];                          // pass 2: the bias of the walked columns
  __shared__ float sh_red[8][TM];                        // pass 3: dbias of (wave, lane half)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int slot = tid & 7, rbs = tid >> 3;
  const int M = a.hdr[0];
  const int res0 = blockIdx.x * TM;
  int tile_lo, tile_hi;
  if (PASS == 2) {
    if (res0 >= M) return;
    tile_lo = (int)((int64_t)blockIdx.y * a.n_ntiles / q.n_split);
    tile_hi = (int)((int64_t)(blockIdx.y + 1) * a.n_ntiles / q.n_split);
  } else {
    tile_lo = 0;
    tile_hi = (M + TN - 1) / TN;
  }
  auto token_slot = [&](int row) {                       // the table entry of row `row` of the list, for slot tid
    float4 st = make_float4(0.f, 1.f, 0.f, 0.f);
    int2 bt = make_int2(0, -1);
    if (row < M) {
      const int id = a.rows[row];
      const float4 s = a.stats[row];
      bt.x = id / a.T;
      bt.y = id - bt.x * a.T;
      st = make_float4(s.x, s.y, s.z * s.w, q.D[id]);
    }
    sh_st[tid] = st;
    sh_bt[tid] = bt;
    if (PASS == 3) {
      const int id = a.rows[min(row, M - 1)];
      const int b = id / a.T, t = id - b * a.T;
      sh_off[tid] = (int64_t)b * a.ld_hb + (int64_t)t * a.ld_ht;
    }
  };
  const E* hrow[2];
  float bias_res[2] = {0.f, 0.f};
  if (PASS == 2) {
    token_rows(a, res0, M, hrow);
    if (tid < TM) token_slot(res0 + tid);
  } else {
#pragma unroll
    for (int u = 0; u < 2; ++u) hrow[u] = (const E*)a.wgt + (int64_t)min(res0 + rbs + 32 * u, a.V - 1) * a.ld_w;
#pragma unroll
    for (int j = 0; j < 2; ++j) bias_res[j] = res0 + 32 * j + r < a.V ? bias_at<E>(a, res0 + 32 * j + r) : 0.f;
  }
  typedef typename Vec<E>::type frag;
  const int vec_res = PASS == 2 ? a.vec_h : a.vec_w, vec_walk = PASS == 2 ? a.vec_w : a.vec_h;
  const int rb2 = wave & 1, kb = wave >> 1;              // the wave's 32 x 32 block of a 64 x 64 block of the output
  float16v out[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < 16; ++k) out[c][k] = 0.f;
  float db[2] = {0.f, 0.f};
  for (int t_i = tile_lo; t_i < tile_hi; ++t_i) {
    const int w0 = t_i * TN;
    // walked row rbs + 32 u of the tile, clamped to a valid one (its dx is zero)
    auto walk_row = [&](int u) -> const E* {
      if (PASS == 2) return (const E*)a.wgt + (int64_t)min(w0 + rbs + 32 * u, a.V - 1) * a.ld_w;
      return (const E*)a.hid + sh_off[rbs + 32 * u];
    };
    if (PASS == 2) {
      sh_bias[tid] = w0 + tid < a.V ? bias_at<E>(a, w0 + tid) : 0.f;
    } else {
      token_slot(w0 + tid);
      __syncthreads();                                     // the rows' addresses are read below
    }
    float16v acc[2][2];
    {
      const E* wrow[TN / 32];
#pragma unroll
      for (int u = 0; u < TN / 32; ++u) wrow[u] = walk_row(u);
      tile_product_rows<E, true>(tile, a.H, hrow, vec_res, wrow, vec_walk, acc);   // (its first barrier publishes the tables, it ends with one)
    }
    // dx of walked row wave * 64 + 32 i + 8 qd + 4 h + e against resident row 32 j + r, four adjacent walked rows as one 8-byte store
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int ws0 = wave * 64 + 32 * i + 8 * qd + 4 * h;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int rslot = 32 * j + r;
          union { uint2 u; E t[4]; } d4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int tslot = PASS == 2 ? rslot : ws0 + e;
            const int v = PASS == 2 ? w0 + ws0 + e : res0 + rslot;
            const float4 st = sh_st[tslot];
            const int2 bt = sh_bt[tslot];
            const float x = acc[i][j][4 * qd + e] + (PASS == 2 ? sh_bias[ws0 + e] : bias_res[j]);
            float dx = 0.f;
            if (bt.y >= 0 && v < a.V) {
              const float p = expf(x - st.x) / st.y;
              float routed = 0.f;
              if ((int)q.tok[(int64_t)bt.x * q.ld_tok + v] == bt.y) routed = q.g[(int64_t)bt.x * q.ld_g + v] * st.z;
              dx = p * (routed - st.w);
            }
            if (PASS == 3) db[j] += dx;
            d4.t[e] = (E)dx;                               // the one rounding of dx, to nearest even
          }
          *reinterpret_cast<uint2*>(dxs + rslot * DXP + 2 * ws0) = d4.u;
        }
      }
    }
    __syncthreads();
    if (PASS == 3 && !q.out) continue;                     // (uniform) dbias alone
    // out[resident][64 c + ..] += dx[resident][walked] . (walked operand)[walked][64 c + ..]
    uint4 sw[TN / 32];
    auto fetch = [&](int c) {
      const int col = (q.c_lo + c) * BK + slot * 8;
      const bool in = col < a.H;
#pragma unroll
      for (int u = 0; u < TN / 32; ++u) {
        sw[u] = load16h(walk_row(u) + (in ? col : 0), vec_walk);
        if (!in) sw[u] = make_uint4(0u, 0u, 0u, 0u);
      }
    };
    fetch(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < q.c_n) {                                     // (uniform)
#pragma unroll
        for (int u = 0; u < TN / 32; ++u) *reinterpret_cast<uint4*>(tile + (TM + rbs + 32 * u) * PITCH + slot * 16) = sw[u];
        __syncthreads();
        if (c + 1 < q.c_n) fetch(c + 1);
#pragma unroll 4
        for (int s = 0; s < TN / 16; ++s) {
          const frag df = *reinterpret_cast<const frag*>(dxs + (32 * rb2 + r) * DXP + 2 * (16 * s + 8 * h));
          // the staged image read by columns, walked rows 16 s + 8 h + (0 .. 7) of column 32 kb + r: two transposed reads of 4 rows x 16
          // columns per 16 lanes (lane 4 q + p of the group gives the address of row q, columns 4 p .. 4 p + 3, and receives its own column)
          const unsigned char* tr = tile + (TM + 16 * s + 8 * h + ((lane >> 2) & 3)) * PITCH + 2 * (32 * kb + (lane & 16) + 4 * (lane & 3));
          union { struct { short4t lo, hi; } p; frag v; } wf;
          wf.p.lo = lds_read_tr16(tr);
          wf.p.hi = lds_read_tr16(tr + 4 * PITCH);
          if constexpr (__is_same(E, __bf16)) out[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, wf.v, out[c], 0, 0, 0);
          else out[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(df, wf.v, out[c], 0, 0, 0);
        }
        __syncthreads();
      }
    }
  }
  // out[c][k]: resident row 32 rb2 + 8 (k >> 2) + 4 h + (k & 3), column 64 (c_lo + c) + 32 kb + r of H
  if (q.out) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = (q.c_lo + c) * BK + 32 * kb + r;
      if (c < q.c_n && col < a.H) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int rs = 32 * rb2 + 8 * (k >> 2) + 4 * h + (k & 3);
          if (PASS == 2) {
            const int2 bt = sh_bt[rs];
            if (bt.y < 0) continue;
            if (q.n_split > 1) q.partial[((int64_t)blockIdx.y * (a.B * a.T) + res0 + rs) * a.H + col] = out[c][k];
            else store_out<E>(q.out, q.out_f32, q.out_f16, (int64_t)bt.x * q.ld_ob + (int64_t)bt.y * q.ld_ot + col, out[c][k]);
          } else if (res0 + rs < a.V) {
            store_out<E>(q.out, q.out_f32, q.out_f16, (int64_t)(res0 + rs) * q.ld_ob + col, out[c][k]);
          }
        }
      }
    }
  }
  if (PASS == 3 && q.dbias) {                              // lane (r, h) of every wave holds a part of columns r and 32 + r: added in a fixed order
    sh_red[2 * wave + h][r] = db[0];
    sh_red[2 * wave + h][32 + r] = db[1];
    __syncthreads();
    if (tid < TM && res0 + tid < a.V) {
      float s = sh_red[0][tid];
      for (int k = 1; k < 8; ++k) s += sh_red[k][tid];
      store_out<E>(q.dbias, q.dbias_f32, q.dbias_f16, res0 + tid, s);
    }
  }
#endif
}

// the shares of pass 2 in share order (fp64, rounded once) -> dhidden.  grid: (rows of the worst-case list, blocks of 256 columns of H)
template <typename E>
__global__ void __launch_bounds__(256) proj_grad_combine_kernel(ProjArgs a, GradArgs q) {
  const int row = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
  if (row >= a.hdr[0] || col >= a.H) return;
  const int id = a.rows[row];
  const int b = id / a.T, t = id - b * a.T;
  double s = 0.0;
  for (int k = 0; k < q.n_split; ++k) s += (double)q.partial[((int64_t)k * (a.B * a.T) + row) * a.H + col];
  store_out<E>(q.out, q.out_f32, q.out_f16, (int64_t)b * q.ld_ob + (int64_t)t * q.ld_ot + col, (float)s);
}

// One launch per slab of H: up to MAX_CHUNKS 64-column chunks fit the registers; a wider H (above 768) is cut into equal slabs, each of
// which computes x again.  dbias belongs to the first slab; where it is all that is wanted (no out), the later slabs have nothing to write.
template <int PASS>
void launch_grad(int value_dtype, int hidden_dim, dim3 grid, hipStream_t s, const ProjArgs& a, GradArgs q) {
  const int n_chunks = (hidden_dim + BK - 1) / BK;
  const int n_slabs = (n_chunks + MAX_CHUNKS - 1) / MAX_CHUNKS, per = (n_chunks + n_slabs - 1) / n_slabs;
  for (int c = 0; c < n_chunks; c += per) {
    q.c_lo = c; q.c_n = std::min(per, n_chunks - c);
    with_half_type(value_dtype, [&](auto t) { with_int<2, 6, MAX_CHUNKS>(per <= 2 ? 2 : per <= 6 ? 6 : MAX_CHUNKS, [&](auto n) {
      hipLaunchKernelGGL((proj_grad_kernel<typename decltype(t)::type, PASS, decltype(n)::value>), grid, dim3(256), 0, s, a, q);
    }); });
    if (!q.out) break;
    q.dbias = nullptr;
  }
}

}  // namespace

extern "C" int64_t dhr_lexical_proj_train_workspace(int64_t batch, int32_t n_tokens, int32_t vocab, int32_t hidden_dim) try {
  if (batch < 0 || n_tokens <= 0 || n_tokens > MAX_TOKENS || vocab <= 0 || hidden_dim <= 0 || hidden_dim > MAX_H || hidden_dim % 8 ||
      batch * n_tokens > ((int64_t)1 << 31) - 1)
    return 0;
  return proj_train_layout(batch, n_tokens, vocab, hidden_dim).total;
} DHR_CATCH_VALUE(0)

extern "C" int dhr_lexical_proj_train(int32_t device, int32_t mem_kind, const void* hidden, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                                      int32_t skip_tokens, int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight, int32_t vocab,
                                      int64_t ld_weight, const void* bias, int32_t bias_dtype, const float* term_weights, int64_t ld_weights,
                                      const float* mask, int64_t ld_mask, float* out_reps, int64_t ld_reps, int16_t* out_tokens, int64_t ld_tokens,
                                      float* out_pwin, int64_t ld_pwin, void* workspace, int64_t workspace_bytes, void* stream) try {
  dhr::alloc_checkpoint();
  if (!out_reps || !out_tokens || !out_pwin) return set_error(DHR_ERR_INVALID, "null pointer");
  const ProjOperands o{mem_kind, hidden, value_dtype, batch, n_tokens, skip_tokens, hidden_dim, ld_batch, ld_token, weight, vocab, ld_weight, bias,
                       bias_dtype, term_weights, ld_weights, mask, ld_mask, workspace, workspace_bytes};
  int rc = check_operands("dhr_lexical_proj_train", true, o);
  if (rc) return rc;
  if (ld_reps < vocab || ld_tokens < vocab || ld_pwin < vocab) return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (batch == 0) return DHR_OK;
  const ProjTrainLayout l = proj_train_layout(batch, n_tokens, vocab, hidden_dim);
  rc = check_workspace("dhr_lexical_proj_train_workspace", l.total, o);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  ProjArgs a = proj_args(l, o);
  a.reps = out_reps; a.ld_reps = ld_reps;
  a.tok = out_tokens; a.ld_tok = ld_tokens;
  a.pwin = out_pwin; a.ld_pwin = ld_pwin;
  launch_forward<true>(value_dtype, a, s);
  HIP_TRY(hipGetLastError());
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_lexical_proj_backward(int32_t device, int32_t mem_kind, const void* hidden, int32_t value_dtype, int64_t batch, int32_t n_tokens,
                                         int32_t skip_tokens, int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight,
                                         int32_t vocab, int64_t ld_weight, const void* bias, int32_t bias_dtype, const float* term_weights,
                                         int64_t ld_weights, const float* mask, int64_t ld_mask, const float* grad_reps, int64_t ld_grad_reps,
                                         const int16_t* tokens, int64_t ld_tokens, const float* pwin, int64_t ld_pwin, void* workspace,
                                         int64_t workspace_bytes, void* grad_hidden, int32_t grad_hidden_dtype, int64_t ld_grad_batch,
                                         int64_t ld_grad_token, void* grad_weight, int32_t grad_weight_dtype, int64_t ld_grad_weight, void* grad_bias,
                                         int32_t grad_bias_dtype, float* grad_term_weights, int64_t ld_grad_term_weights, void* stream) try {
  dhr::alloc_checkpoint();
  if (!grad_reps || !tokens || !pwin) return set_error(DHR_ERR_INVALID, "null pointer");
  const ProjOperands o{mem_kind, hidden, value_dtype, batch, n_tokens, skip_tokens, hidden_dim, ld_batch, ld_token, weight, vocab, ld_weight, bias,
                       bias_dtype, term_weights, ld_weights, mask, ld_mask, workspace, workspace_bytes};
  int rc = check_operands("dhr_lexical_proj_backward", true, o);
  if (rc) return rc;
  if ((grad_hidden && !val_ok_bf16(grad_hidden_dtype)) || (grad_weight && !val_ok_bf16(grad_weight_dtype)) ||
      (grad_bias && !val_ok_bf16(grad_bias_dtype)))
    return set_error(DHR_ERR_INVALID, "bad value dtype");
  auto bf16_of_fp16 = [&](const void* p, int32_t dt) { return p && dt == DHR_VAL_BF16 && value_dtype == DHR_VAL_F16; };
  if (bf16_of_fp16(grad_hidden, grad_hidden_dtype) || bf16_of_fp16(grad_weight, grad_weight_dtype) || bf16_of_fp16(grad_bias, grad_bias_dtype))
    return set_error(DHR_ERR_UNSUPPORTED, "dhr_lexical_proj_backward: a bf16 gradient needs bf16 hidden states and weight (the fp16 kernels write fp32 or fp16)");
  if (ld_grad_reps < vocab || ld_tokens < vocab || ld_pwin < vocab || (grad_term_weights && ld_grad_term_weights < n_tokens) ||
      (grad_weight && ld_grad_weight < hidden_dim) ||
      (grad_hidden && (ld_grad_token < hidden_dim || ld_grad_batch < (int64_t)(n_tokens + skip_tokens - 1) * ld_grad_token + hidden_dim)))
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (batch == 0 || (!grad_hidden && !grad_weight && !grad_bias && !grad_term_weights)) return DHR_OK;
  const ProjTrainLayout l = proj_train_layout(batch, n_tokens, vocab, hidden_dim);
  rc = check_workspace("dhr_lexical_proj_train_workspace", l.total, o);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const ProjArgs a = proj_args(l, o);
  const int T = n_tokens;
  const int64_t BT = batch * T;
  float* D = (float*)((char*)workspace + l.D);
  // pass 1: every later pass reads D
  const bool small = (int64_t)((T + RT_BIG - 1) / RT_BIG) * batch < 512;
  for (int64_t lo = 0; lo < batch; lo += 65535) {           // (grid y limit)
    const unsigned rows = (unsigned)std::min<int64_t>(65535, batch - lo);
    float* dw = grad_term_weights ? grad_term_weights + lo * ld_grad_term_weights : nullptr;
    with_int<RT_SMALL, RT_BIG>(small ? RT_SMALL : RT_BIG, [&](auto r) {
      constexpr int RT = decltype(r)::value;
      hipLaunchKernelGGL(proj_route_sum_kernel<RT>, dim3((unsigned)((T + RT - 1) / RT), rows), dim3(256), 0, s, grad_reps + lo * ld_grad_reps,
                         ld_grad_reps, tokens + lo * ld_tokens, ld_tokens, pwin + lo * ld_pwin, ld_pwin, term_weights + lo * ld_weights, ld_weights,
                         mask + lo * ld_mask, ld_mask, T, vocab, D + lo * T, dw, ld_grad_term_weights);
    });
  }
  HIP_TRY(hipGetLastError());
  GradArgs q{};
  q.g = grad_reps; q.ld_g = ld_grad_reps; q.tok = tokens; q.ld_tok = ld_tokens; q.D = D;
  if (grad_hidden) {                                       // pass 2
    const int es = grad_hidden_dtype == DHR_VAL_F32 ? 4 : 2;
    hipLaunchKernelGGL(proj_zero_rows_kernel, dim3((unsigned)(batch * (skip_tokens + T))), dim3(256), 0, s, a, grad_hidden,
                       (int)(grad_hidden_dtype == DHR_VAL_F32), ld_grad_batch, ld_grad_token, (int)skip_tokens);
    q.out = (char*)grad_hidden + (int64_t)skip_tokens * ld_grad_token * es;
    dtype_flags(grad_hidden_dtype, q.out_f32, q.out_f16); q.ld_ob = ld_grad_batch; q.ld_ot = ld_grad_token;
    q.partial = (float*)((char*)workspace + l.partial); q.n_split = l.grad_split;
    launch_grad<2>(value_dtype, hidden_dim, dim3((unsigned)((BT + TM - 1) / TM), (unsigned)l.grad_split), s, a, q);
    if (l.grad_split > 1) {
      const dim3 g_comb((unsigned)BT, (unsigned)((hidden_dim + 255) / 256));
      with_half_type(value_dtype, [&](auto t) {
        hipLaunchKernelGGL(proj_grad_combine_kernel<typename decltype(t)::type>, g_comb, dim3(256), 0, s, a, q);
      });
    }
    HIP_TRY(hipGetLastError());
  }
  if (grad_weight || grad_bias) {                          // pass 3
    q.out = grad_weight; dtype_flags(grad_weight_dtype, q.out_f32, q.out_f16); q.ld_ob = ld_grad_weight; q.ld_ot = 0;
    q.dbias = grad_bias; dtype_flags(grad_bias_dtype, q.dbias_f32, q.dbias_f16);
    q.partial = nullptr; q.n_split = 1;
    launch_grad<3>(value_dtype, hidden_dim, dim3((unsigned)((vocab + TM - 1) / TM)), s, a, q);
    HIP_TRY(hipGetLastError());
  }
  return DHR_OK;
} DHR_CATCH_STATUS

// Streamed exact inner-product search over fp32 vectors of any width (dhr_stream_search_*): the retrieval route of the reference that searches
// the un-densified vectors, [lexical reps over the whole vocabulary | semantic reps] per text, chunk by chunk with a running top-k
// (tevatron/datasets/beir/encode_and_retrieval.py).  DESIGN.md section 4o.
//   score(q, r) = sum_c qa[q][c] pa[r][c] + sum_c qb[q][c] pb[r][c], a function of the two rows alone, bit for bit:
//   every row x gets a power-of-two scale 2^e that brings its largest magnitude into [2^14, 2^15) and is split as in kmeans.hip into two fp16
//   images, hi = fp16(x 2^e) (0 where that would be subnormal) and lo = fp16((x 2^e - hi) 2^11).  Per 128 columns the products hi.hi (one fp32
//   MFMA accumulator) and hi.lo + lo.hi (a second one) are summed by v_mfma_f32_32x32x16_f16, then folded into a float64 sum per output; the
//   total is unscaled exactly and rounded to fp32 once.  lo.lo is dropped.
//   stream_split_kernel    the two images of a set of rows, [rows padded to 128][D_pad], each segment padded to 128 columns with zeros, and the rows'
//                          exponents: the queries once at create, the passages block by block (4 bytes per element, as much as the block's
//                          fp32 rows, written once and read by every query tile; splitting on the way into LDS instead was built first and
//                          spent as many VALU cycles per chunk as the MFMAs take, once per query tile).
//   stream_score_kernel    a workgroup of 8 waves owns 128 queries x 128 rows, a wave 32 queries x 64 rows: 32 float64 sums per lane.  Both operands
//                          go through LDS in chunks of 128 columns (rows padded to 272 bytes, as in kmeans.hip / maxsim.hip; 139 KB), the next
//                          chunk is in registers while this one is multiplied.  Epilogue: (score, row) against the query's k-th entry as of launch;
//                          survivors go to the query's slice of a [Q][block_rows] candidate buffer, one atomic per wave and query.
//   stream_select_kernel   per query with survivors: bitonic sort of M of them at a time in LDS, bitonic merge with the running list.
// The [Q, n_rows] score matrix never reaches memory; a slice holds block_rows entries and a row is appended at most once, so it cannot overflow.
#include <memory>

#include "host_stage.h"

namespace {

constexpr int KC = 128;                    // columns per chunk: 256 bytes of fp16
constexpr int ROW_PITCH = 256 + 16;        // LDS pitch of a row of one chunk
constexpr int TQ = 128, TR = 128;          // queries and passage rows of a workgroup
constexpr int SCORE_THREADS = 512;
constexpr int IMG = TQ * ROW_PITCH;        // one image of one operand of one chunk
constexpr int SCORE_LDS = 4 * IMG + TR * 4;
constexpr int SELECT_THREADS = 256;
constexpr int MAX_D = 131072, MAX_Q = 65536, MAX_K = 4096, MAX_BLOCK = 65536;
constexpr float LO_SCALE = 2048.f;
constexpr double LO_UNSCALE = 1.0 / 2048.0;
constexpr float F16_MIN_NORMAL = 6.103515625e-05f;
constexpr int64_t ROW_PAD = INT64_MAX;     // the row of a padding entry of the select: behind every real (-inf, row)

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));

// the exponent e of a row whose largest magnitude is m: m 2^e in [2^14, 2^15); 0 for a row of zeros or one that holds an infinity
__device__ __forceinline__ int row_exponent(float m) {
  if (!(m > 0.f) || m == INFINITY) return 0;
  int x;
  (void)frexpf(m, &x);
  return 15 - x;
}

// (v - hi is exact in fp32: hi is v rounded to 11 bits, or 0)
__device__ __forceinline__ void split(float x, int e, _Float16& hi, _Float16& lo) {
  const float v = ldexpf(x, e);
  hi = (_Float16)v;
  if (fabsf((float)hi) < F16_MIN_NORMAL) hi = (_Float16)0.f;
  lo = (_Float16)((v - (float)hi) * LO_SCALE);
}

// largest |x| of a row over both segments (fmaxf drops a NaN: the row's other values keep their scale), reduced over the workgroup
__device__ __forceinline__ float row_max(const float* a, int d_a, const float* b, int d_b, float* part) {
  const int tid = threadIdx.x;
  float m = 0.f;
  for (int c = tid; c < d_a; c += 256) m = fmaxf(m, fabsf(a[c]));
  for (int c = tid; c < d_b; c += 256) m = fmaxf(m, fabsf(b[c]));
  part[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] = fmaxf(part[tid], part[tid + o]);
    __syncthreads();
  }
  return part[0];
}

// grid: the rows padded to 128 (queries, or the passages of a block); rows beyond Q and columns beyond a segment are zeros
__global__ void __launch_bounds__(256) stream_split_kernel(const float* __restrict__ qa, int64_t ld_qa, const float* __restrict__ qb, int64_t ld_qb, int Q,
                                                           int d_a, int d_b, int pa, int d_pad, _Float16* __restrict__ qhi, _Float16* __restrict__ qlo,
                                                           int32_t* __restrict__ q_exp) {
  __shared__ float part[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  const bool real = q < Q;
  const float* a = qa + (real ? q : 0) * ld_qa;
  const float* b = d_b ? qb + (real ? q : 0) * ld_qb : nullptr;
  const int e = real ? row_exponent(row_max(a, d_a, b, d_b, part)) : 0;
  if (tid == 0) q_exp[q] = e;
  for (int col = tid; col < d_pad; col += 256) {
    float x = 0.f;
    if (real && col < pa) { if (col < d_a) x = a[col]; }
    else if (real && col - pa < d_b) x = b[col - pa];
    _Float16 hi, lo;
    split(x, e, hi, lo);
    qhi[(int64_t)q * d_pad + col] = hi;
    qlo[(int64_t)q * d_pad + col] = lo;
  }
}

__global__ void __launch_bounds__(256) stream_init_kernel(float* __restrict__ list_s, int64_t* __restrict__ list_r, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { list_s[i] = -INFINITY; list_r[i] = -1; }
}

struct ScoreArgs {
  const _Float16 *qhi, *qlo;   // [Q_pad][d_pad]
  const _Float16 *phi, *plo;   // [rows of the block padded to 128][d_pad]
  const int32_t *q_exp, *p_exp;
  int n_chunks, d_pad;
  int n_queries, n_rows;       // rows of the block
  int64_t row_base;            // the caller's number of the block's first row
  const float* list_s;         // [Q][k], sorted
  const int64_t* list_r;
  int k;
  uint2* cand;                 // [Q][cap] (score bits, row in the block)
  uint32_t* cnt;               // [Q]
  uint32_t cap;
};

// grid: score_grid() workgroups.  Workgroup i runs on XCD i % 8, so the 32 that an XCD holds at a time are given one
// block of 8 query tiles x 4 row tiles: every chunk of an operand tile that reaches the XCD's L2 is used 4 or 8 times.
__global__ void __launch_bounds__(SCORE_THREADS) stream_score_kernel(ScoreArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char *QH = lds, *QL = lds + IMG, *PH = lds + 2 * IMG, *PL = lds + 3 * IMG;
  int32_t* pexp = reinterpret_cast<int32_t*>(lds + 4 * IMG);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5, wq = wave & 3, wr = wave >> 2;
  const int n_qt = (g.n_queries + TQ - 1) / TQ, n_rt = (g.n_rows + TR - 1) / TR, n_qb = (n_qt + 7) / 8;
  const int block = (blockIdx.x >> 8) * 8 + (blockIdx.x & 7), within = (blockIdx.x >> 3) & 31;
  const int qt = (block % n_qb) * 8 + (within & 7), rt = (block / n_qb) * 4 + (within >> 3);
  if (qt >= n_qt || rt >= n_rt) return;
  const int q0 = qt * TQ, row0 = rt * TR;
  if (t < TR) pexp[t] = g.p_exp[row0 + t];
  // staging: thread t moves slot t & 15 of rows t >> 4, 32 + (t >> 4), ... of the four images of a chunk (padded: every load is whole and aligned)
  const int64_t d_pad = g.d_pad;
  const int64_t st_at = (int64_t)(t >> 4) * d_pad + (t & 15) * 8;
  const _Float16 *qhi = g.qhi + q0 * d_pad + st_at, *qlo = g.qlo + q0 * d_pad + st_at;
  const _Float16 *phi = g.phi + row0 * d_pad + st_at, *plo = g.plo + row0 * d_pad + st_at;
  const int st_off = (t >> 4) * ROW_PITCH + (t & 15) * 16;
  uint4v qh[4], ql[4], ph[4], pl[4];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t at = (int64_t)chunk * KC + i * 32 * d_pad;
      qh[i] = *reinterpret_cast<const uint4v*>(qhi + at);
      ql[i] = *reinterpret_cast<const uint4v*>(qlo + at);
      ph[i] = *reinterpret_cast<const uint4v*>(phi + at);
      pl[i] = *reinterpret_cast<const uint4v*>(plo + at);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = st_off + i * 32 * ROW_PITCH;
      *reinterpret_cast<uint4v*>(QH + off) = qh[i];
      *reinterpret_cast<uint4v*>(QL + off) = ql[i];
      *reinterpret_cast<uint4v*>(PH + off) = ph[i];
      *reinterpret_cast<uint4v*>(PL + off) = pl[i];
    }
  };
  double sum[2][16];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int k = 0; k < 16; ++k) sum[rb][k] = 0.0;
  fetch(0);
  for (int chunk = 0; chunk < g.n_chunks; ++chunk) {
    store();
    __syncthreads();
    if (chunk + 1 < g.n_chunks) fetch(chunk + 1);
    float16v hh[2], hl[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int k = 0; k < 16; ++k) { hh[rb][k] = 0.f; hl[rb][k] = 0.f; }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int q_at = (wq * 32 + r) * ROW_PITCH + (2 * v + h) * 16;
      const half8 b_hi = *reinterpret_cast<const half8*>(QH + q_at);
      const half8 b_lo = *reinterpret_cast<const half8*>(QL + q_at);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const int p_at = (wr * 64 + rb * 32 + r) * ROW_PITCH + (2 * v + h) * 16;
        const half8 a_hi = *reinterpret_cast<const half8*>(PH + p_at);
        const half8 a_lo = *reinterpret_cast<const half8*>(PL + p_at);
        hh[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, hh[rb], 0, 0, 0);
        hl[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, hl[rb], 0, 0, 0);
        hl[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, hl[rb], 0, 0, 0);
      }
    }
#endif
    // the fold: 128 columns of fp32 sums into the float64 sum of the output
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int k = 0; k < 16; ++k) sum[rb][k] += (double)hh[rb][k] + (double)hl[rb][k] * LO_UNSCALE;
    __syncthreads();
  }
  // this lane: query q against rows row0 + 64 wr + 32 rb + 4h + (k & 3) + 8 (k >> 2) of the block
  const int q = q0 + wq * 32 + r;
  const bool q_real = q < g.n_queries;
  const int qe = q_real ? g.q_exp[q] : 0;
  const float thr_s = q_real ? g.list_s[(int64_t)q * g.k + g.k - 1] : INFINITY;
  const int64_t thr_r = q_real ? g.list_r[(int64_t)q * g.k + g.k - 1] : -1;
  float score[2][16];
  uint32_t pass = 0;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int local = wr * 64 + rb * 32 + 4 * h + (k & 3) + 8 * (k >> 2);
      const int row = row0 + local;
      const float s = (float)ldexp(sum[rb][k], -(qe + pexp[local])) + 0.f;            // (+ 0: no negative zero in a list)
      score[rb][k] = s;
      const bool in = q_real && row < g.n_rows && (s > thr_s || (s == thr_s && g.row_base + row < thr_r));       // a NaN passes neither test
      pass |= (uint32_t)in << (rb * 16 + k);
    }
  const uint32_t mine = __popc(pass), other = __shfl_xor(mine, 32, 64);
  uint32_t at = 0;
  if (h == 0 && mine + other > 0) at = atomicAdd(g.cnt + q, mine + other);       // lanes r and r + 32 hold the same query
  at = __shfl(at, r, 64) + (h ? other : 0);
  uint2* slice = g.cand + (int64_t)(q_real ? q : 0) * g.cap;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (pass >> (rb * 16 + k) & 1) {
        const int row = row0 + wr * 64 + rb * 32 + 4 * h + (k & 3) + 8 * (k >> 2);
        if (at < g.cap) slice[at] = make_uint2(__float_as_uint(score[rb][k]), (uint32_t)row);
        ++at;
      }
}

struct SelectArgs2 {
  const uint2* cand;
  uint32_t* cnt;
  uint32_t cap;
  int64_t row_base;
  float* list_s;
  int64_t* list_r;
  int k, M;
};

__device__ __forceinline__ bool better(const float* ss, const int64_t* rr, int a, int b) {
  return ss[a] > ss[b] || (ss[a] == ss[b] && rr[a] < rr[b]);
}

// The n entries from `off` (n a power of two): a bitonic sort (first = 2), or the merge of a bitonic sequence (first = n); best first where
// desc, else worst first.
__device__ void bitonic(float* ss, int64_t* rr, int off, int n, bool desc, int first) {
  for (int k2 = first; k2 <= n; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n / 2; i += SELECT_THREADS) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), a = off + lo, b = a + j;
        const bool best_first = ((lo & k2) == 0 || k2 == n) == desc;
        if (better(ss, rr, b, a) == best_first) {
          const float s = ss[a]; ss[a] = ss[b]; ss[b] = s;
          const int64_t w = rr[a]; rr[a] = rr[b]; rr[b] = w;
        }
      }
      __syncthreads();
    }
}

// grid: queries.  LDS: 2 M rows (int64), then 2 M scores: the list in [0, M), a batch of survivors in [M, 2 M).
__global__ void __launch_bounds__(SELECT_THREADS) stream_select_kernel(SelectArgs2 g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int q = blockIdx.x, tid = threadIdx.x, M = g.M, k = g.k;
  int64_t* rr = reinterpret_cast<int64_t*>(lds);
  float* ss = reinterpret_cast<float*>(lds + (size_t)2 * M * 8);
  const uint32_t n = min(g.cnt[q], g.cap);
  if (n == 0) return;
  for (int i = tid; i < M; i += SELECT_THREADS) {
    ss[i] = i < k ? g.list_s[(int64_t)q * k + i] : -INFINITY;
    rr[i] = i < k ? g.list_r[(int64_t)q * k + i] : ROW_PAD;
  }
  const uint2* slice = g.cand + (int64_t)q * g.cap;
  for (uint32_t base = 0; base < n; base += M) {
    for (int i = tid; i < M; i += SELECT_THREADS) {
      const bool real = base + i < n;
      const uint2 c = real ? slice[base + i] : make_uint2(0u, 0u);
      ss[M + i] = real ? __uint_as_float(c.x) : -INFINITY;
      rr[M + i] = real ? g.row_base + (int64_t)c.y : ROW_PAD;
    }
    __syncthreads();
    bitonic(ss, rr, M, M, false, 2);
    bitonic(ss, rr, 0, 2 * M, true, 2 * M);
  }
  for (int i = tid; i < k; i += SELECT_THREADS) {
    g.list_s[(int64_t)q * k + i] = ss[i];
    g.list_r[(int64_t)q * k + i] = rr[i] == ROW_PAD ? -1 : rr[i];
  }
  if (tid == 0) g.cnt[q] = 0;
}

int64_t up(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
int pad_cols(int d) { return (d + KC - 1) / KC * KC; }

template <class K>
hipError_t allow_lds(K kernel, int bytes) {      // beyond the 64 KiB a kernel gets unasked
  return bytes > 65536 ? hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) : hipSuccess;
}

}  // namespace

struct dhr_stream_search {
  int device = 0;
  int Q = 0, Q_pad = 0, d_a = 0, d_b = 0, pa = 0, d_pad = 0, k = 0, block_rows = 0, M = 0;
  DevMem mem;                  // one allocation; the arrays below are parts of it
  _Float16 *qhi = nullptr, *qlo = nullptr, *phi = nullptr, *plo = nullptr;      // the images of the queries and of a block of passages
  int32_t *q_exp = nullptr, *p_exp = nullptr;
  float* list_s = nullptr;
  int64_t* list_r = nullptr;
  uint32_t* cnt = nullptr;
  uint2* cand = nullptr;
  int64_t bytes = 0;
};

namespace {

int check_segment(const char* what, const void* a, int64_t ld_a, int d_a, const void* b, int64_t ld_b, int d_b) {
  if (!a) return set_error(DHR_ERR_INVALID, "null pointer");
  if ((b != nullptr) != (d_b > 0)) return set_error(DHR_ERR_INVALID, std::string("stream search: ") + what + "_b must be NULL exactly when d_b is 0");
  if (ld_a < d_a || (d_b > 0 && ld_b < d_b)) return set_error(DHR_ERR_INVALID, std::string("stream search: a row stride of ") + what + " is shorter than its segment");
  return DHR_OK;
}

int check_dtype(int32_t value_dtype) {
  if (!val_ok(value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (value_dtype != DHR_VAL_F32) return set_error(DHR_ERR_UNSUPPORTED, "stream search: values must be fp32 (DHR_VAL_F32)");
  return DHR_OK;
}

// one block of at most block_rows rows, all on the device: its images, scores against the lists as they are, select
hipError_t launch_block(const dhr_stream_search& h, const float* pa, int64_t ld_pa, const float* pb, int64_t ld_pb, int n, int64_t row_base, hipStream_t s) {
  const int n_pad = (n + TR - 1) / TR * TR;
  hipLaunchKernelGGL(stream_split_kernel, dim3((unsigned)n_pad), dim3(256), 0, s, pa, ld_pa, pb, ld_pb, n, h.d_a, h.d_b, h.pa, h.d_pad, h.phi, h.plo, h.p_exp);
  ScoreArgs a{h.qhi, h.qlo, h.phi, h.plo, h.q_exp, h.p_exp, h.d_pad / KC, h.d_pad, h.Q, n, row_base, h.list_s, h.list_r, h.k, h.cand, h.cnt, (uint32_t)h.block_rows};
  hipError_t e = allow_lds(stream_score_kernel, SCORE_LDS);
  if (e != hipSuccess) return e;
  const int blocks = ((h.Q_pad / TQ + 7) / 8) * ((n_pad / TR + 3) / 4);      // of 8 x 4 tiles, dealt over the 8 XCDs
  hipLaunchKernelGGL(stream_score_kernel, dim3((unsigned)((blocks + 7) / 8 * 256)), dim3(SCORE_THREADS), SCORE_LDS, s, a);
  SelectArgs2 sel{h.cand, h.cnt, (uint32_t)h.block_rows, row_base, h.list_s, h.list_r, h.k, h.M};
  const int lds = 2 * h.M * 12;
  if ((e = allow_lds(stream_select_kernel, lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(stream_select_kernel, dim3((unsigned)h.Q), dim3(SELECT_THREADS), (size_t)lds, s, sel);
  return hipGetLastError();
}

}  // namespace

extern "C" int dhr_stream_search_create(int32_t device, int32_t mem_kind, const void* q_a, int64_t ld_qa, const void* q_b, int64_t ld_qb, int32_t value_dtype,
                                        int32_t n_queries, int32_t d_a, int32_t d_b, int32_t k, int32_t block_rows, dhr_stream_search** out,
                                        void* stream) try {
  dhr::alloc_checkpoint();
  if (!out) return set_error(DHR_ERR_INVALID, "null pointer");
  *out = nullptr;
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (int rc = check_dtype(value_dtype)) return rc;
  if (d_a < 1 || d_b < 0 || (int64_t)d_a + d_b > MAX_D)
    return set_error(DHR_ERR_INVALID, "stream search: d_a must be >= 1, d_b >= 0 and d_a + d_b <= 131072, got " + std::to_string(d_a) + " and " + std::to_string(d_b));
  if (n_queries < 1 || n_queries > MAX_Q) return set_error(DHR_ERR_INVALID, "stream search: n_queries must be in [1, 65536], got " + std::to_string(n_queries));
  if (k < 1) return set_error(DHR_ERR_INVALID, "stream search: k must be >= 1, got " + std::to_string(k));
  if (k > MAX_K) return set_error(DHR_ERR_UNSUPPORTED, "stream search: k above 4096 is not built, got " + std::to_string(k));
  if (block_rows != 0 && (block_rows < TR || block_rows > MAX_BLOCK || block_rows % TR))
    return set_error(DHR_ERR_INVALID, "stream search: block_rows must be 0 or a multiple of 128 in [128, 65536], got " + std::to_string(block_rows));
  if (int rc = check_segment("q", q_a, ld_qa, d_a, q_b, ld_qb, d_b)) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  std::unique_ptr<dhr_stream_search> h(new dhr_stream_search);
  h->device = device;
  h->Q = n_queries; h->Q_pad = (n_queries + TQ - 1) / TQ * TQ;
  h->d_a = d_a; h->d_b = d_b; h->pa = pad_cols(d_a); h->d_pad = h->pa + pad_cols(d_b);
  h->k = k;
  // the default block: candidate slices of 256 MB in all, at most 16 384 rows
  h->block_rows = block_rows ? block_rows : (int)std::min<int64_t>(16384, std::max<int64_t>(TR, ((int64_t)1 << 25) / h->Q_pad / TR * TR));
  h->M = 1024;
  while (h->M < k) h->M *= 2;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t o = at; at += up(bytes); return o; };
  const int64_t o_qhi = take((int64_t)h->Q_pad * h->d_pad * 2), o_qlo = take((int64_t)h->Q_pad * h->d_pad * 2), o_qe = take((int64_t)h->Q_pad * 4);
  const int64_t o_phi = take((int64_t)h->block_rows * h->d_pad * 2), o_plo = take((int64_t)h->block_rows * h->d_pad * 2);
  const int64_t o_pe = take((int64_t)h->block_rows * 4), o_ls = take((int64_t)n_queries * k * 4), o_lr = take((int64_t)n_queries * k * 8);
  const int64_t o_cnt = take((int64_t)h->Q_pad * 4), o_cand = take((int64_t)n_queries * h->block_rows * 8);
  h->bytes = at;
  HIP_TRY(dev_alloc(h->mem, at));
  char* base = (char*)h->mem.p;
  h->qhi = (_Float16*)(base + o_qhi); h->qlo = (_Float16*)(base + o_qlo); h->q_exp = (int32_t*)(base + o_qe); h->p_exp = (int32_t*)(base + o_pe);
  h->phi = (_Float16*)(base + o_phi); h->plo = (_Float16*)(base + o_plo);
  h->list_s = (float*)(base + o_ls); h->list_r = (int64_t*)(base + o_lr); h->cnt = (uint32_t*)(base + o_cnt); h->cand = (uint2*)(base + o_cand);
  const bool host = mem_kind == DHR_MEM_HOST;
  DevMem m_a, m_b;
  const float *qa = (const float*)q_a, *qb = (const float*)q_b;
  if (host) {
    HIP_TRY(stage_in(m_a, q_a, ld_qa, n_queries, d_a, 4, s));
    qa = (const float*)m_a.p; ld_qa = d_a;
    if (d_b) { HIP_TRY(stage_in(m_b, q_b, ld_qb, n_queries, d_b, 4, s)); qb = (const float*)m_b.p; ld_qb = d_b; }
  }
  HIP_TRY(hipMemsetAsync(h->cnt, 0, (size_t)h->Q_pad * 4, s));
  const int64_t n_list = (int64_t)n_queries * k;
  hipLaunchKernelGGL(stream_init_kernel, dim3((unsigned)std::min<int64_t>((n_list + 255) / 256, 4096)), dim3(256), 0, s, h->list_s, h->list_r, n_list);
  hipLaunchKernelGGL(stream_split_kernel, dim3((unsigned)h->Q_pad), dim3(256), 0, s, qa, ld_qa, qb, ld_qb, n_queries, d_a, d_b, h->pa, h->d_pad, h->qhi, h->qlo,
                     h->q_exp);
  HIP_TRY(hipGetLastError());
  if (host) HIP_TRY(hipStreamSynchronize(s));
  *out = h.release();
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_stream_search_add(dhr_stream_search* h, int32_t mem_kind, const void* p_a, int64_t ld_pa, const void* p_b, int64_t ld_pb, int32_t value_dtype,
                                     int64_t n_rows, int64_t row_base, void* stream) try {
  dhr::alloc_checkpoint();
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (int rc = check_dtype(value_dtype)) return rc;
  if (n_rows < 0 || n_rows > ((int64_t)1 << 40)) return set_error(DHR_ERR_INVALID, "stream search: n_rows must be in [0, 2^40], got " + std::to_string(n_rows));
  if (row_base < 0 || row_base > ((int64_t)1 << 62)) return set_error(DHR_ERR_INVALID, "stream search: row_base must be in [0, 2^62], got " + std::to_string(row_base));
  if (!h) return set_error(DHR_ERR_INVALID, "null pointer");
  if (n_rows == 0) return DHR_OK;          // (an empty array may have no address)
  if (int rc = check_segment("p", p_a, ld_pa, h->d_a, p_b, ld_pb, h->d_b)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const bool host = mem_kind == DHR_MEM_HOST;
  const int64_t per = std::min<int64_t>(n_rows, h->block_rows);
  DevMem m_a, m_b;                         // host arrays: one block at a time goes through these
  if (host) {
    HIP_TRY(dev_alloc(m_a, per * h->d_a * 4));
    if (h->d_b) HIP_TRY(dev_alloc(m_b, per * h->d_b * 4));
  }
  for (int64_t r0 = 0; r0 < n_rows; r0 += per) {
    const int n = (int)std::min<int64_t>(per, n_rows - r0);
    const float* pa = (const float*)p_a + r0 * ld_pa;
    const float* pb = h->d_b ? (const float*)p_b + r0 * ld_pb : nullptr;
    int64_t la = ld_pa, lb = ld_pb;
    if (host) {
      HIP_TRY(copy_in(m_a.p, pa, ld_pa, n, h->d_a, 4, s));
      pa = (const float*)m_a.p; la = h->d_a;
      if (h->d_b) { HIP_TRY(copy_in(m_b.p, pb, ld_pb, n, h->d_b, 4, s)); pb = (const float*)m_b.p; lb = h->d_b; }
    }
    HIP_TRY(launch_block(*h, pa, la, pb, lb, n, row_base + r0, s));
  }
  if (host) HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int dhr_stream_search_result(dhr_stream_search* h, float* out_scores, int64_t* out_rows, int32_t out_mem_kind, void* stream) try {
  dhr::alloc_checkpoint();
  if (!h || !out_scores || !out_rows) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(out_mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)h->Q * h->k;
  const hipMemcpyKind kind = out_mem_kind == DHR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIP_TRY(hipMemcpyAsync(out_scores, h->list_s, n * 4, kind, s));
  HIP_TRY(hipMemcpyAsync(out_rows, h->list_r, n * 8, kind, s));
  if (out_mem_kind == DHR_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

extern "C" int64_t dhr_stream_search_device_bytes(const dhr_stream_search* h) try { return h ? h->bytes : 0; } DHR_CATCH_VALUE(0)

extern "C" void dhr_stream_search_destroy(dhr_stream_search* h) try {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;                                // (hipFree waits for the work that still reads the arrays)
} DHR_CATCH_VOID

// Per-query row exclusion behind a ranked list (dhr_exclude_rows; dhr_search_excluding in api.hip runs it behind a deeper dhr_search): drops from
// each query's list the rows of its exclusion list and keeps the first k_out of the rest, in their input order.
//
// One workgroup of 256 lanes per query.  The query's exclusion list is staged into LDS in chunks of DHR_EXCLUDE_CHUNK rows (16 KiB), so a list
// of any length costs further passes and never a larger allocation: the passes over all chunks but the last only mark the entries they hit in a
// per-entry bit mask (LDS, n_in bits, present only where some list of the batch is longer than one chunk); the pass over the last chunk tests
// mask and chunk together and compacts.  A chunk of at most EXCL_LINEAR rows is compared row by row (every lane reads the same LDS word: a
// broadcast, no bank conflict) -- the case of the callers this was written for, one to a few dozen positives per query; a longer chunk is sorted
// in place (bitonic, padded to a power of two with INT64_MAX) and binary-searched over its real rows.  The compaction is the refine level's
// (kernels.hip): ballot + mbcnt prefix inside a wave, four wave counts through LDS, the running base in a register of every lane -- no global
// atomics, every output position follows from the input order alone, so two calls on the same arguments are bit-identical.
#include <mutex>

#include "host_stage.h"

namespace dhr {
namespace {
constexpr int EXCL_THREADS = 256;
constexpr int EXCL_WAVES = EXCL_THREADS / 64;
constexpr int EXCL_CHUNK = DHR_EXCLUDE_CHUNK;
constexpr int EXCL_LINEAR = 64;               // rows of a chunk that are compared one by one instead of sorted and searched
constexpr int64_t EXCL_PAD = INT64_MAX;
static_assert((EXCL_CHUNK & (EXCL_CHUNK - 1)) == 0 && EXCL_CHUNK >= 2 * EXCL_THREADS, "the bitonic sort wants a power of two of at least 512 rows");

// ex[0, m): the staged chunk; sorted ascending when m > EXCL_LINEAR
__device__ __forceinline__ bool excl_member(const int64_t* ex, int m, int64_t r) {
  if (m <= EXCL_LINEAR) {
    bool hit = false;
    for (int j = 0; j < m; ++j) hit |= ex[j] == r;
    return hit;
  }
  int lo = 0, hi = m;                          // first position with ex[pos] >= r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ex[mid] < r) lo = mid + 1; else hi = mid;
  }
  return lo < m && ex[lo] == r;
}

__global__ void __launch_bounds__(EXCL_THREADS) exclude_rows_kernel(int n_in, const float* __restrict__ in_scores, const int64_t* __restrict__ in_rows,
                                                                     const int64_t* __restrict__ excl_ptr, const int64_t* __restrict__ excl_rows, int k_out,
                                                                     float* __restrict__ out_scores, int64_t* __restrict__ out_rows,
                                                                     int32_t* __restrict__ out_valid, int flag_words) {
  __shared__ int64_t ex[EXCL_CHUNK];
  __shared__ uint32_t wave_n[2][EXCL_WAVES];
  extern __shared__ uint32_t flags[];          // [flag_words] bit i: entry i is in one of the chunks before the last (0 words: every list fits one chunk)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const int64_t e_lo = excl_ptr[q], e_len = excl_ptr[q + 1] - e_lo;
  const int n_chunks = e_len > EXCL_CHUNK ? (int)((e_len + EXCL_CHUNK - 1) / EXCL_CHUNK) : 1;
  const bool flagged = n_chunks > 1;           // (uniform over the workgroup; flag_words > 0 then: the launcher sizes the mask by the longest list)
  const float* qs = in_scores + q * n_in;
  const int64_t* qr = in_rows + q * n_in;
  if (flagged) {
    for (int i = tid; i < flag_words; i += EXCL_THREADS) flags[i] = 0u;
  }
  int m = 0;
  for (int c = 0; c < n_chunks; ++c) {
    __syncthreads();                           // the previous pass is done with ex; the mask is zeroed
    const int64_t c_lo = e_lo + (int64_t)c * EXCL_CHUNK;
    m = (int)(e_len - (int64_t)c * EXCL_CHUNK < EXCL_CHUNK ? e_len - (int64_t)c * EXCL_CHUNK : EXCL_CHUNK);
    for (int i = tid; i < m; i += EXCL_THREADS) ex[i] = excl_rows[c_lo + i];
    if (m > EXCL_LINEAR) {
      int P = 2 * EXCL_LINEAR;
      while (P < m) P <<= 1;
      for (int i = m + tid; i < P; i += EXCL_THREADS) ex[i] = EXCL_PAD;
      for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          __syncthreads();
          for (int t = tid; t < P / 2; t += EXCL_THREADS) {
            const int a = 2 * t - (t & (j - 1)), b = a + j;
            const int64_t va = ex[a], vb = ex[b];
            if ((va > vb) == ((a & k) == 0)) { ex[a] = vb; ex[b] = va; }
          }
        }
      }
    }
    __syncthreads();
    if (c == n_chunks - 1) break;
    for (int i = tid; i < n_in; i += EXCL_THREADS) {
      const int64_t r = qr[i];
      if (r >= 0 && excl_member(ex, m, r)) atomicOr(&flags[i >> 5], 1u << (i & 31));      // (an LDS atomic; OR commutes, the mask does not depend on the order)
    }
  }
  // ---- the last chunk: test and compact, 256 entries per round, in input order
  int base = 0;
  for (int t0 = 0, par = 0; t0 < n_in && base < k_out; t0 += EXCL_THREADS, par ^= 1) {
    const int i = t0 + tid;
    bool keep = false;
    int64_t r = -1;
    if (i < n_in) {
      r = qr[i];
      if (r >= 0) keep = !(flagged && ((flags[i >> 5] >> (i & 31)) & 1u)) && !excl_member(ex, m, r);
    }
    const unsigned long long bal = __ballot(keep);
    const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (lane == 0) wave_n[par][wave] = (uint32_t)__popcll(bal);
    __syncthreads();                           // (one barrier per round: the next round writes the other half of wave_n)
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < EXCL_WAVES; ++w) {
      const int n = (int)wave_n[par][w];
      off += w < wave ? n : 0;
      tot += n;
    }
    const int pos = base + off + before;
    if (keep && pos < k_out) {
      out_scores[q * k_out + pos] = qs[i];
      out_rows[q * k_out + pos] = r;
    }
    base += tot;
  }
  const int valid = base < k_out ? base : k_out;
  for (int j = valid + tid; j < k_out; j += EXCL_THREADS) {
    out_scores[q * k_out + j] = -INFINITY;
    out_rows[q * k_out + j] = -1;
  }
  if (out_valid && tid == 0) out_valid[q] = valid;
}
}  // namespace

// excl_ptr: DEVICE copy of the CSR offsets [n_queries + 1]; max_list: the longest list of the batch (sizes the per-entry mask)
hipError_t launch_exclude_rows(int n_queries, int n_in, const float* in_scores, const int64_t* in_rows, const int64_t* excl_ptr, const int64_t* excl_rows,
                               int64_t max_list, int k_out, float* out_scores, int64_t* out_rows, int32_t* out_valid, hipStream_t s) {
  if (n_queries <= 0) return hipSuccess;
  const int flag_words = max_list > EXCL_CHUNK ? (n_in + 31) / 32 : 0;
  const int lds = flag_words * 4;
  if (lds > 0) {                                // beyond the 64 KiB a kernel gets unasked: per device and under a lock, as in kernels.hip
    static std::mutex mu;
    static int have[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    if (lds > have[dev & 63]) {
      const hipError_t e = hipFuncSetAttribute((const void*)exclude_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return e;
      have[dev & 63] = lds;
    }
  }
  hipLaunchKernelGGL(exclude_rows_kernel, dim3((unsigned)n_queries), dim3(EXCL_THREADS), (size_t)lds, s, n_in, in_scores, in_rows, excl_ptr, excl_rows,
                     k_out, out_scores, out_rows, out_valid, flag_words);
  return hipGetLastError();
}
}  // namespace dhr

// The CSR of a batch's exclusion lists, checked on the host before anything touches the device: offsets from 0, never decreasing; rows present
// where there are any.  Leaves the longest list in *max_list and the number of rows in *total.
int check_exclusions(int n_queries, const int64_t* excl_ptr_host, const int64_t* excl_rows, int64_t* max_list, int64_t* total) {
  if (!excl_ptr_host) return set_error(DHR_ERR_INVALID, "null excl_ptr_host");
  if (excl_ptr_host[0] != 0) return set_error(DHR_ERR_INVALID, "excl_ptr_host[0] must be 0, is " + std::to_string(excl_ptr_host[0]));
  int64_t longest = 0;
  for (int q = 0; q < n_queries; ++q) {
    const int64_t len = excl_ptr_host[q + 1] - excl_ptr_host[q];
    if (len < 0) return set_error(DHR_ERR_INVALID, "excl_ptr_host decreases at query " + std::to_string(q));
    longest = std::max(longest, len);
  }
  if (excl_ptr_host[n_queries] > 0 && !excl_rows) return set_error(DHR_ERR_INVALID, "null excl_rows");
  *max_list = longest;
  *total = excl_ptr_host[n_queries];
  return DHR_OK;
}

extern "C" int32_t dhr_debug_exclude_chunk(void) try {
  return EXCL_CHUNK;
} DHR_CATCH_VALUE(0)

extern "C" int dhr_exclude_rows(int32_t device, int32_t mem_kind, int32_t n_queries, int32_t n_in, const float* in_scores, const int64_t* in_rows,
                                const int64_t* excl_ptr_host, const int64_t* excl_rows, int32_t k_out, float* out_scores, int64_t* out_rows,
                                int32_t* out_valid, void* stream) try {
  dhr::alloc_checkpoint();
  if (!in_scores || !in_rows || !out_scores || !out_rows) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (n_queries < 0) return set_error(DHR_ERR_INVALID, "n_queries must be >= 0");
  if (n_in <= 0) return set_error(DHR_ERR_INVALID, "n_in must be > 0");
  if (k_out <= 0 || k_out > n_in) return set_error(DHR_ERR_INVALID, "need 0 < k_out <= n_in");
  int64_t max_list = 0, total = 0;
  const int rc = check_exclusions(n_queries, excl_ptr_host, excl_rows, &max_list, &total);
  if (rc != DHR_OK) return rc;
  if (max_list > EXCL_CHUNK && n_in > (1 << 20))
    return set_error(DHR_ERR_UNSUPPORTED, "lists of more than 1048576 entries together with an exclusion list longer than " + std::to_string(EXCL_CHUNK) +
                                              " rows (" + std::to_string(max_list) + ") are not supported");
  if (n_queries == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const size_t ptr_bytes = (size_t)(n_queries + 1) * 8, n = (size_t)n_queries * n_in, no = (size_t)n_queries * k_out;
  if (mem_kind == DHR_MEM_DEVICE) {             // enqueued: the offsets travel in stream-ordered scratch, the caller's stream stays asynchronous
    void* d_ptr = nullptr;
    HIP_TRY(hipMallocAsync(&d_ptr, ptr_bytes, s));
    hipError_t e = copy_in(d_ptr, excl_ptr_host, ptr_bytes, s);
    if (e == hipSuccess)
      e = launch_exclude_rows(n_queries, n_in, in_scores, in_rows, (const int64_t*)d_ptr, excl_rows, max_list, k_out, out_scores, out_rows, out_valid, s);
    (void)hipFreeAsync(d_ptr, s);
    HIP_TRY(e);
    return DHR_OK;
  }
  // host arrays: staged through the device, complete on return
  DevMem m_ptr, m_ex, m_is, m_ir, m_os, m_or, m_ov;
  HIP_TRY(stage_in(m_ptr, excl_ptr_host, ptr_bytes, s));
  HIP_TRY(stage_in(m_ex, excl_rows, (size_t)total * 8, s));
  HIP_TRY(stage_in(m_is, in_scores, n * 4, s));
  HIP_TRY(stage_in(m_ir, in_rows, n * 8, s));
  HIP_TRY(dev_alloc(m_os, (int64_t)no * 4));
  HIP_TRY(dev_alloc(m_or, (int64_t)no * 8));
  if (out_valid) HIP_TRY(dev_alloc(m_ov, (int64_t)n_queries * 4));
  HIP_TRY(launch_exclude_rows(n_queries, n_in, (const float*)m_is.p, (const int64_t*)m_ir.p, (const int64_t*)m_ptr.p, (const int64_t*)m_ex.p, max_list, k_out,
                              (float*)m_os.p, (int64_t*)m_or.p, (int32_t*)m_ov.p, s));
  HIP_TRY(stage_out(out_scores, m_os.p, no * 4, s));
  HIP_TRY(stage_out(out_rows, m_or.p, no * 8, s));
  if (out_valid) HIP_TRY(stage_out(out_valid, m_ov.p, (size_t)n_queries * 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

// Sparse term-weight vectors -> DLR index records (densify/densify_corpus.py:29-52, densify/densify_query.py:96 of the reference: the producer of
// the BM25, DeepImpact, uniCOIL and SPLADE indexes).  The reference folds the {term: weight} entries of one vector in the order they are given,
// in Python, one token at a time; the dense op dhr_densify is no substitute, since for whole-word matching the vocabulary is a Lucene term list
// of millions of terms and a [batch, vocab] array cannot exist.  Here the input is CSR and one wave folds one vector:
//   densify_sparse_kernel   the row lives in LDS as one word per slice (group << 16 | fp16 bits), up to four vectors per workgroup.  Entries are
//                           read 64 at a time, coalesced; a lane's RANK is the number of lower lanes of its batch that hit the same slice (13
//                           wave votes, no LDS); round k applies the lanes of rank k, so every slice sees its entries in entry order and the
//                           fold of the reference holds for any weights (zeros, -0.0, negatives), not only for positive ones.  The LDS row is
//                           then written out whole, zeros included: no memset, no global atomics, nothing allocated, the same bits every run.
// A term id is never an address: ids outside [omission, vocab) are skipped before anything is derived from them; row ranges are clamped to
// [0, nnz].  The waves of a workgroup share nothing, so the kernel has no workgroup barrier.
#include "host_stage.h"
#include "op_dispatch.h"

namespace {

constexpr int MAX_DIMS = 8192;            // the index's column limit
constexpr int SLICE_BITS = 13;            // a slice number is below MAX_DIMS
constexpr int LDS_WORDS = 16384;          // 64 KiB of row words per workgroup

// the LDS accesses of one wave run in program order; this keeps the compiler from moving them across a round
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int64_t wave_uniform(int64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// fp16(w), rounded once to nearest even (an fp32 above 65 504 gives inf, as NumPy does)
__device__ __forceinline__ uint32_t half_bits(float w) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)w); }
__device__ __forceinline__ uint32_t half_bits(_Float16 w) { return (uint32_t)__builtin_bit_cast(uint16_t, w); }
__device__ __forceinline__ _Float16 as_half(uint32_t bits) { return __builtin_bit_cast(_Float16, (uint16_t)bits); }

template <typename TID, typename TW, typename TV, typename TI>
__global__ void __launch_bounds__(256) densify_sparse_kernel(const int64_t* __restrict__ row_ptr, const TID* __restrict__ ids,
                                                             const TW* __restrict__ weights, int64_t nnz, int64_t batch, int64_t vocab, int om,
                                                             int dims, TV* __restrict__ out_value, int64_t ld_value, TI* __restrict__ out_index,
                                                             int64_t ld_index, int32_t* __restrict__ collisions) {
  extern __shared__ uint32_t lds_rows[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  uint32_t* row = lds_rows + (size_t)wave * dims;
  for (int64_t b = (int64_t)blockIdx.x * waves + wave; b < batch; b += (int64_t)gridDim.x * waves) {
    for (int j = lane; j < dims; j += 64) row[j] = 0u;
    wave_sync();
    const int64_t lo = wave_uniform(min(max(row_ptr[b], (int64_t)0), nnz)), hi = wave_uniform(min(max(row_ptr[b + 1], (int64_t)0), nnz));
    int coll = 0;
    for (int64_t e0 = lo; e0 < hi; e0 += 64) {               // (a row whose end lies before its start is empty)
      const int64_t e = e0 + lane;
      bool in = false;
      int s = -1;
      uint32_t word = 0u;
      if (e < hi) {
        const int64_t t = (int64_t)ids[e];
        if (t >= om && t < vocab) {
          const int u = (int)(t - om), g = u / dims;
          in = true;
          s = u - g * dims;
          word = ((uint32_t)g << 16) | half_bits(weights[e]);
        }
      }
      // the lanes in scope whose slice has the same SLICE_BITS bits as this lane's, one vote per bit; those below this lane are its rank
      unsigned long long same = __ballot(in);
#pragma unroll
      for (int k = 0; k < SLICE_BITS; ++k) {
        const bool bit = (s >> k) & 1;
        const unsigned long long set = __ballot(bit);
        same &= bit ? set : ~set;
      }
      const int rank = __popcll(same & ((1ull << lane) - 1ull));
      for (int k = 0; __any(in && rank >= k); ++k) {
        if (in && rank == k) {
          const uint32_t cur = row[s];
          if ((cur & 0x7fffu) == 0u) {                       // value[s] == 0: +0.0 or -0.0
            row[s] = word;
          } else {
            ++coll;
            if (as_half(cur) < as_half(word)) row[s] = word;
          }
        }
        wave_sync();
      }
    }
    TV* ov = out_value + b * ld_value;
    TI* oi = out_index + b * ld_index;
    for (int j = lane; j < dims; j += 64) {
      const uint32_t q = row[j];
      ov[j] = (TV)as_half(q);
      oi[j] = (TI)(q >> 16);
    }
    if (collisions) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) coll += __shfl_xor(coll, d);
      if (lane == 0) collisions[b] = coll;
    }
    wave_sync();                                             // the row is read before the next vector zeroes it
  }
}

int launch(const int64_t* row_ptr, const void* ids, int id_bytes, const void* weights, int weight_dtype, int64_t nnz, int64_t batch, int64_t vocab,
           int om, int dims, void* out_value, int out_value_dtype, int64_t ld_value, void* out_index, int index_dtype, int64_t ld_index,
           int32_t* collisions, hipStream_t s) {
  const int waves = std::max(1, std::min(4, LDS_WORDS / dims));
  const dim3 grid((unsigned)std::min<int64_t>((batch + waves - 1) / waves, 1 << 16));
  const size_t lds = (size_t)waves * dims * 4;
  with_id_type(id_bytes, [&](auto i) { with_value_type(weight_dtype, [&](auto w) { with_value_type(out_value_dtype, [&](auto v) {
    with_index_type(index_dtype, [&](auto x) {
      using I = typename decltype(i)::type;
      using W = typename decltype(w)::type;
      using V = typename decltype(v)::type;
      using X = typename decltype(x)::type;
      hipLaunchKernelGGL((densify_sparse_kernel<I, W, V, X>), grid, dim3(waves * 64), lds, s, row_ptr, (const I*)ids, (const W*)weights, nnz, batch,
                         vocab, om, dims, (V*)out_value, ld_value, (X*)out_index, ld_index, collisions);
    });
  }); }); });
  HIP_TRY(hipGetLastError());
  return DHR_OK;
}

}  // namespace

extern "C" int dhr_densify_sparse(int32_t device, int32_t mem_kind, const int64_t* row_ptr, const void* term_ids, int32_t id_bytes,
                                  const void* weights, int32_t weight_dtype, int64_t nnz, int64_t batch, int64_t vocab, int32_t omission,
                                  int32_t dims, void* out_value, int32_t out_value_dtype, int64_t ld_value, void* out_index, int32_t index_dtype,
                                  int64_t ld_index, int32_t* collisions, void* stream) try {
  dhr::alloc_checkpoint();
  if (!row_ptr || !out_value || !out_index || (nnz > 0 && (!term_ids || !weights))) return set_error(DHR_ERR_INVALID, "null pointer");
  if (!DHR_MEM_KIND_OK(mem_kind)) return set_error(DHR_ERR_INVALID, "bad mem_kind");
  if (id_bytes != 4 && id_bytes != 8) return set_error(DHR_ERR_INVALID, "term ids must be int32 or int64 (id_bytes 4 or 8)");
  if (!val_ok(weight_dtype) || !val_ok(out_value_dtype)) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (!idx_ok(index_dtype)) return set_error(DHR_ERR_INVALID, "index dtype must be uint8, int8 or int16");
  if (nnz < 0 || batch < 0 || vocab <= 0 || dims <= 0 || omission < 0 || omission >= vocab || ld_value < dims || ld_index < dims)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  const int64_t max_group = (vocab - 1 - omission) / dims, limit = index_dtype == DHR_IDX_I16 ? 32767 : index_dtype == DHR_IDX_U8 ? 255 : 127;
  if (max_group > limit)
    return set_error(DHR_ERR_INVALID, "the largest group " + std::to_string(max_group) + " does not fit the index dtype (at most " +
                                          std::to_string(limit) + ")");
  if (dims > MAX_DIMS) return set_error(DHR_ERR_UNSUPPORTED, "more than 8192 dims");
  if (batch == 0) return DHR_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (mem_kind == DHR_MEM_DEVICE)                             // enqueued: the caller's stream stays asynchronous
    return launch(row_ptr, term_ids, id_bytes, weights, weight_dtype, nnz, batch, vocab, omission, dims, out_value, out_value_dtype, ld_value,
                  out_index, index_dtype, ld_index, collisions, s);
  // host arrays: staged through the device, complete on return
  const int wes = val_esize(weight_dtype), oes = val_esize(out_value_dtype), xes = idx_esize(index_dtype);
  DevMem m_ptr, m_ids, m_w, m_val, m_idx, m_coll;
  HIP_TRY(stage_in(m_ptr, row_ptr, (size_t)(batch + 1) * 8, s));
  HIP_TRY(stage_in(m_ids, term_ids, (size_t)nnz * id_bytes, s));
  HIP_TRY(stage_in(m_w, weights, (size_t)nnz * wes, s));
  HIP_TRY(dev_alloc(m_val, batch * dims * oes));
  HIP_TRY(dev_alloc(m_idx, batch * dims * xes));
  if (collisions) HIP_TRY(dev_alloc(m_coll, batch * 4));
  const int rc = launch((const int64_t*)m_ptr.p, m_ids.p, id_bytes, m_w.p, weight_dtype, nnz, batch, vocab, omission, dims, m_val.p, out_value_dtype,
                        dims, m_idx.p, index_dtype, dims, (int32_t*)m_coll.p, s);
  if (rc != DHR_OK) return rc;
  HIP_TRY(stage_out(out_value, ld_value, m_val.p, batch, dims, oes, s));
  HIP_TRY(stage_out(out_index, ld_index, m_idx.p, batch, dims, xes, s));
  if (collisions) HIP_TRY(stage_out(collisions, m_coll.p, (size_t)batch * 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DHR_OK;
} DHR_CATCH_STATUS

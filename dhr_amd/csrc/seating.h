// Seating of a query batch for the main pass (search_core.hip): which SLOT of the bound GEMM's query tiles a query
// computes in.  The filter epilogue of gemm_filter_g8_kernel enters a block of four accumulators wave-wide as soon as ONE of the wave's 32
// queries has a hit in it, and a few per cent of a batch pass 10-100 x the average through the filter: seated by descending hit count, the hot
// queries share a few wave columns instead of slowing dozens.  Nothing a query computes depends on its slot.
// Plain C++17, no HIP: the order and the padded-slot rule live here, seat_rank_kernel (kernels.hip) and tests/seating_check.cpp use them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DHR_SEAT_HD __host__ __device__
#else
#define DHR_SEAT_HD
#endif

namespace dhr {
namespace seat {

constexpr int MAX_QUERIES = 8192;      // padded queries of a seated batch (the keys of seat_rank_kernel live in one workgroup's LDS); beyond: identity

// Sort key of query q: the length of its bound lists over the sampled run; a padded query (q >= n_queries) sorts behind every real one
DHR_SEAT_HD inline int64_t key_of(uint32_t len, int q, int n_queries) { return q < n_queries ? (int64_t)len : (int64_t)-1; }
// Query a (key ka) sits in front of query b (key kb): longer lists first, ties by query number
DHR_SEAT_HD inline bool before(int64_t ka, int a, int64_t kb, int b) { return ka > kb || (ka == kb && a < b); }
// Slot of query q among the q_pad queries of the batch: the number of queries in front of it (rank sort; len[j] for j < n_queries only)
DHR_SEAT_HD inline int slot_of(const uint32_t* len, int q, int n_queries, int q_pad) {
  const int64_t kq = key_of(q < n_queries ? len[q] : 0u, q, n_queries);
  int slot = 0;
  for (int j = 0; j < q_pad; ++j) slot += before(key_of(j < n_queries ? len[j] : 0u, j, n_queries), j, kq, q) ? 1 : 0;
  return slot;
}

}  // namespace seat
}  // namespace dhr

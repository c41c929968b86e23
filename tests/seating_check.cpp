// Stand-alone check of dhr_amd/csrc/seating.h (plain C++17, built with AddressSanitizer and UBSan by tests/test_seating_order.py): the slot of
// every query under the order "longer bound lists first, ties by query number, padded queries behind the real ones" is a permutation of
// [0, q_pad), equals a stable sort by descending length, and keeps the padded slots in place.
#include "seating.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d): n_queries %d q_pad %d case %d\n", #c, __LINE__, nq, q_pad, kind); return 1; } } while (0)

int main() {
  std::mt19937 rng(12345);
  long cases = 0;
  const int sizes[] = {1, 2, 88, 255, 256, 257, 600, 700, 1023, 1024};
  for (int nq : sizes)
    for (int kind = 0; kind < 5; ++kind) {
      const int q_pad = (nq + 255) / 256 * 256;
      std::vector<uint32_t> len(nq);
      for (int q = 0; q < nq; ++q)
        len[q] = kind == 0 ? 0u                                        // all equal: the identity
               : kind == 1 ? (uint32_t)q                               // ascending: reversed
               : kind == 2 ? (uint32_t)(rng() % 4)                     // many ties
               : kind == 3 ? (q % 97 == 0 ? 0xffffffffu : rng() % 1000)   // a few huge ones (the largest value a counter holds)
                           : (uint32_t)rng();
      std::vector<int> slot(q_pad), seen(q_pad, 0);
      for (int q = 0; q < q_pad; ++q) {
        slot[q] = dhr::seat::slot_of(len.data(), q, nq, q_pad);
        CHECK(slot[q] >= 0 && slot[q] < q_pad);
        CHECK(seen[slot[q]]++ == 0);                                   // a permutation
        CHECK((q < nq) == (slot[q] < nq));                             // real queries in front of padded ones
        if (q >= nq) CHECK(slot[q] == q);                              // a padded query keeps its place
      }
      std::vector<int> order(nq);
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
      for (int s = 0; s < nq; ++s) CHECK(slot[order[s]] == s);
      if (kind == 0)
        for (int q = 0; q < nq; ++q) CHECK(slot[q] == q);
      ++cases;
    }
  std::printf("seating ok: %ld cases\n", cases);
  return 0;
}

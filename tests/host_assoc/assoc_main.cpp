// Test-only, a program of its own (never loaded into Python; `make asan` builds it under AddressSanitizer and UBSan): the host
// form of the permutation null (assoc_host.cpp) against the contract written out directly — the n1 smallest of N sorted keys,
// and a plain double loop over relabelings and features — on tables in which every feasible cell has a rank of its own, at
// the edges of the sample count, the slice and the block's relabelings.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_assoc_core.h"

using namespace dcrx_assoc;

extern "C" int assoc_host_permute(uint32_t N, uint64_t C, uint32_t F, const uint64_t *mask, const uint32_t *mult, const uint16_t *rank_in,
                                  uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, uint64_t seed, uint32_t *obs_rank, uint64_t *labels,
                                  uint32_t *perm_min, uint64_t *tail, uint64_t *flushes_out);

namespace {

// the contract's relabeling: sort the keys, take the n1 smallest
uint64_t plain_labels(uint64_t seed, uint32_t p, uint32_t N, uint32_t n1) {
  std::vector<std::pair<uint64_t, uint32_t>> keys;
  for (uint32_t s = 0; s < N; s++) keys.push_back({dcrx_rar::key(seed, p, s), s});
  std::sort(keys.begin(), keys.end());
  uint64_t L = 0;
  for (uint32_t i = 0; i < n1; i++) L |= 1ull << keys[i].second;
  return L;
}

int one(const char *what, uint32_t N, uint64_t C, uint32_t F, uint32_t P, uint32_t tail_share, uint64_t seed) {
  const uint32_t n1 = popcount(C);
  std::vector<uint16_t> rank(cells(N), 0xFFFF);      // cells no cohort produces: never read
  uint32_t n_ranks = 0;
  for (uint32_t m = 0; m <= N; m++)
    for (uint32_t k = m + 1; k-- > 0;)      // descending in k: not monotone the way a one-sided test is
      if (feasible(N, n1, m, k)) rank[m * (N + 1) + k] = (uint16_t)n_ranks++;
  const uint32_t tail_ranks = n_ranks / tail_share;
  std::vector<uint64_t> mask(F);
  std::vector<uint32_t> mult(F);
  for (uint32_t f = 0; f < F; f++) {
    const uint64_t a = dcrx_rar::fin(seed + f), b = dcrx_rar::fin(a);
    mask[f] = (f % 3 ? a & b : a) & sample_bits(N);      // sparse and dense patterns
    mult[f] = f % 7 == 0 ? 0 : (uint32_t)(b >> 40);
  }
  std::vector<uint32_t> obs(F + 1), least(P + 1);
  std::vector<uint64_t> labels(P + 1), tail(tail_ranks + 1);
  uint64_t flushes = 0;
  if (assoc_host_permute(N, C, F, mask.data(), mult.data(), rank.data(), n_ranks, tail_ranks, P, seed, obs.data(), labels.data(), least.data(),
                         tail.data(), &flushes)) {
    std::printf("%s: refused\n", what);
    return 1;
  }
  uint64_t differ = 0;
  std::vector<uint64_t> want_tail(tail_ranks, 0);
  for (uint32_t f = 0; f < F; f++) differ += obs[f] != rank[popcount(mask[f]) * (N + 1) + popcount(mask[f] & C)];
  for (uint32_t p = 0; p < P; p++) {
    const uint64_t L = plain_labels(seed, p, N, n1);
    differ += L != labels[p] || popcount(L) != n1;
    uint32_t lo = n_ranks;
    for (uint32_t f = 0; f < F; f++) {
      if (!mult[f]) continue;
      const uint32_t r = rank[popcount(mask[f]) * (N + 1) + popcount(mask[f] & L)];
      lo = std::min(lo, r);
      if (r < tail_ranks) want_tail[r] += mult[f];
    }
    differ += lo != least[p];
  }
  for (uint32_t r = 0; r < tail_ranks; r++) differ += want_tail[r] != tail[r];
  std::printf("%s: N %u, n1 %u, F %u, P %u, %u ranks, %u in the tail, %llu flushes: %llu differ\n", what, N, n1, F, P, n_ranks, tail_ranks,
              (unsigned long long)flushes, (unsigned long long)differ);
  return differ ? 1 : 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += one("two samples", 2, 1, 5, 3, 1, 0);
  bad += one("the seam of a mask's halves", 33, 0x1AAAAAAAAull, 300, 257, 1, 7);
  bad += one("a full-width mask, one case", 64, 1ull << 63, 257, 300, 2, ~0ull);
  bad += one("a full-width mask, one control", 64, ~0ull >> 1, 64, 65, 1, 3);
  bad += one("one past a slice and one past a block's relabelings", 16, 0xFF, SLICE + 1, BLOCK_PERMS + 1, 3, 11);
  bad += one("no features", 9, 0x3, 0, 10, 1, 5);
  bad += one("no permutations", 9, 0x3, 10, 0, 1, 5);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}

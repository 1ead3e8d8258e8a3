// Test-only, a program of its own (never loaded into Python; `make asan` builds it under AddressSanitizer and UBSan): the host
// form of the wide permutation null (assoc_wide_host.cpp) against the contract written out directly — the n1 smallest of N
// sorted keys, and a plain double loop over relabelings and features — on tables in which every feasible cell has a rank of its
// own, at the edges of the word count, the slice and the block's relabelings, in sorted and in shuffled order of popcount.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_assoc_wide_core.h"

using namespace dcrx_assoc_wide;

extern "C" int assoc_wide_host_permute(uint32_t N, const uint64_t *C_in, uint32_t F, const uint64_t *mask, const uint32_t *mult,
                                       const uint32_t *rank_in, uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, uint64_t seed,
                                       uint32_t *obs_rank, uint64_t *labels, uint32_t *perm_min, uint64_t *tail, uint64_t *counts_out);

namespace {

// the contract's relabeling: sort the keys, take the n1 smallest
std::vector<uint64_t> plain_labels(uint64_t seed, uint32_t p, uint32_t N, uint32_t n1) {
  std::vector<std::pair<uint64_t, uint32_t>> keys;
  for (uint32_t s = 0; s < N; s++) keys.push_back({dcrx_rar::key(seed, p, s), s});
  std::sort(keys.begin(), keys.end());
  std::vector<uint64_t> L(words_for(N), 0);
  for (uint32_t i = 0; i < n1; i++) L[keys[i].second >> 6] |= 1ull << (keys[i].second & 63);
  return L;
}

uint32_t count(const std::vector<uint64_t> &a, const uint64_t *b, uint32_t W) {
  uint32_t n = 0;
  for (uint32_t w = 0; w < W; w++) n += popcount(a[w] & b[w]);
  return n;
}

int one(const char *what, uint32_t N, uint32_t n1, uint32_t F, uint32_t P, uint32_t tail_share, uint64_t seed, bool sorted) {
  const uint32_t W = words_for(N);
  std::vector<uint64_t> C(W, 0);
  for (uint32_t i = 0; i < n1; i++) {      // cases spread over the words
    const uint32_t s = (uint32_t)(((uint64_t)i * N) / n1);
    C[s >> 6] |= 1ull << (s & 63);
  }
  std::vector<uint32_t> rank(cells(N), 0xFFFFFFFFu);      // cells no cohort produces: never read
  uint32_t n_ranks = 0;
  for (uint32_t m = 0; m <= N; m++)
    for (uint32_t k = m + 1; k-- > 0;)      // descending in k: not monotone the way a one-sided test is
      if (feasible(N, n1, m, k)) rank[m * (N + 1) + k] = n_ranks++;
  const uint32_t tail_ranks = n_ranks / tail_share;
  std::vector<std::pair<uint32_t, std::vector<uint64_t>>> feats(F);
  std::vector<uint32_t> mult(F);
  for (uint32_t f = 0; f < F; f++) {
    std::vector<uint64_t> M(W);
    uint32_t m = 0;
    for (uint32_t w = 0; w < W; w++) {
      const uint64_t a = dcrx_rar::fin(seed + f * 31 + w), b = dcrx_rar::fin(a), c = dcrx_rar::fin(b);
      M[w] = (f % 5 == 0 ? a : f % 5 == 1 ? a & b : (a & b & c & dcrx_rar::fin(c))) & word_bits(N, w);      // dense to sparse
      if (f % 5 >= 3 && w != f % W) M[w] = 0;                                                                // one word alone
      m += popcount(M[w]);
    }
    feats[f] = {m, M};
    mult[f] = f % 7 == 0 ? 0 : (uint32_t)(dcrx_rar::fin(seed ^ f) >> 40);
  }
  if (sorted) std::stable_sort(feats.begin(), feats.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
  std::vector<uint64_t> mask((size_t)F * W + 1);
  for (uint32_t f = 0; f < F; f++)
    for (uint32_t w = 0; w < W; w++) mask[(size_t)f * W + w] = feats[f].second[w];
  std::vector<uint32_t> obs(F + 1), least(P + 1);
  std::vector<uint64_t> labels((size_t)P * W + 1), tail(tail_ranks + 1);
  uint64_t counts[2] = {0, 0};
  if (assoc_wide_host_permute(N, C.data(), F, mask.data(), mult.data(), rank.data(), n_ranks, tail_ranks, P, seed, obs.data(), labels.data(),
                              least.data(), tail.data(), counts)) {
    std::printf("%s: refused\n", what);
    return 1;
  }
  uint64_t differ = 0;
  std::vector<uint64_t> want_tail(tail_ranks, 0);
  for (uint32_t f = 0; f < F; f++) differ += obs[f] != rank[feats[f].first * (N + 1) + count(C, &mask[(size_t)f * W], W)];
  for (uint32_t p = 0; p < P; p++) {
    const std::vector<uint64_t> L = plain_labels(seed, p, N, n1);
    differ += count(L, L.data(), W) != n1;
    for (uint32_t w = 0; w < W; w++) differ += L[w] != labels[(size_t)p * W + w];
    uint32_t lo = n_ranks;
    for (uint32_t f = 0; f < F; f++) {
      if (!mult[f]) continue;
      const uint32_t r = rank[feats[f].first * (N + 1) + count(L, &mask[(size_t)f * W], W)];
      lo = std::min(lo, r);
      if (r < tail_ranks) want_tail[r] += mult[f];
    }
    differ += lo != least[p];
  }
  for (uint32_t r = 0; r < tail_ranks; r++) differ += want_tail[r] != tail[r];
  std::printf("%s: N %u (%u words), n1 %u, F %u, P %u, %u ranks, %u in the tail, %llu runs, %llu flushes: %llu differ\n", what, N, W, n1, F, P,
              n_ranks, tail_ranks, (unsigned long long)counts[1], (unsigned long long)counts[0], (unsigned long long)differ);
  return differ ? 1 : 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += one("two samples", 2, 1, 5, 3, 1, 0, true);
  bad += one("a full word", 64, 31, 200, 70, 1, 7, false);
  bad += one("one sample into the second word, one case", 65, 1, 257, 130, 2, ~0ull, false);
  bad += one("three words, one control", 129, 128, 100, 65, 1, 3, true);
  bad += one("five words: two relabelings a lane", 300, 140, 90, 513, 3, 9, false);
  bad += one("ten words, sorted: one relabeling a lane", 640, 320, 120, 257, 2, 11, true);
  bad += one("sixteen words", 1024, 512, 60, 40, 1, 13, false);
  bad += one("one short of sixteen words", 1023, 300, 40, 30, 1, 17, true);
  bad += one("one past a slice and one past a block's relabelings", 70, 30, SLICE + 1, block_perms(2) + 1, 3, 11, true);
  bad += one("no features", 200, 3, 0, 10, 1, 5, true);
  bad += one("no permutations", 200, 3, 10, 0, 1, 5, true);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}

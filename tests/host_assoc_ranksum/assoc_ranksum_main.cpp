// Test-only, a program of its own (never loaded into Python; `make asan` builds it under AddressSanitizer and UBSan): the host
// form of the rank-sum null (assoc_ranksum_host.cpp) against the contract written out directly — the n1 smallest of N sorted
// keys, a rank sum as a plain sum of scores over the samples of a relabeling, the cell of a score by a linear scan of the edges —
// on seeded scores at the edges of the sample count, the slice, the group and the block's relabelings.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_assoc_ranksum_core.h"

using namespace dcrx_assoc_rs;

extern "C" int assoc_ranksum_host_run(uint32_t N, uint64_t C, uint32_t alternative, uint32_t F, const uint64_t *plane, const uint32_t *offset,
                                      const uint32_t *scale, const uint32_t *mult, uint32_t E, const uint32_t *edges, uint32_t P, uint64_t seed,
                                      uint32_t *obs_score, uint64_t *labels, uint32_t *perm_max, uint32_t *exceed, uint64_t *tail,
                                      uint64_t *counts_out);

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

uint64_t isqrt(unsigned __int128 x) {
  uint64_t r = 0;
  for (int b = 63; b >= 0; b--) {
    const uint64_t c = r | (1ull << b);
    if ((unsigned __int128)c * c <= x) r = c;
  }
  return r;
}

// the contract's score, from the scores themselves
uint32_t plain_score(const std::vector<uint32_t> &a, uint64_t L, uint32_t N, uint32_t offset, uint32_t scale, uint32_t alternative) {
  int64_t W = 0;
  for (uint32_t s = 0; s < N; s++)
    if (L >> s & 1) W += a[s];
  const int64_t D = (int64_t)N * W - (int64_t)offset;
  int64_t u = alternative == 0 ? D : alternative == 1 ? -D : (D < 0 ? -D : D);
  u = std::min<int64_t>(std::max<int64_t>(u, 0), (1 << 20) - 1);
  return (uint32_t)(((uint64_t)u * scale) >> 20);
}

int one(const char *what, uint32_t N, uint64_t C, uint32_t alternative, uint32_t F, uint32_t P, uint32_t E, uint64_t seed) {
  const uint32_t n1 = popcount(C);
  std::vector<std::vector<uint32_t>> a(F, std::vector<uint32_t>(N, 0));
  std::vector<uint64_t> plane((size_t)F * PLANES + 1, 0);
  std::vector<uint32_t> offset(F + 1), scale(F + 1), mult(F + 1);
  for (uint32_t f = 0; f < F; f++) {
    // values: sparse (most samples 0), dense, or constant; then doubled mid-ranks less their minimum
    std::vector<uint32_t> x(N);
    for (uint32_t s = 0; s < N; s++) {
      const uint64_t r = dcrx_rar::fin(seed * 1000003 + (uint64_t)f * 64 + s);
      x[s] = f % 5 == 4 ? 3 : f % 3 == 0 ? (uint32_t)(r % 1000) : (r % 16 == 0 ? (uint32_t)(r >> 8) % 4 + 1 : 0);
    }
    uint32_t least = 0xFFFFFFFFu;
    std::vector<uint32_t> d(N);
    for (uint32_t s = 0; s < N; s++) {
      uint32_t below = 0, same = 0;
      for (uint32_t q = 0; q < N; q++) { below += x[q] < x[s]; same += x[q] == x[s]; }
      d[s] = 2 * below + same + 1;
      least = std::min(least, d[s]);
    }
    uint64_t A = 0, B = 0;
    for (uint32_t s = 0; s < N; s++) {
      a[f][s] = d[s] - least;
      A += a[f][s];
      B += (uint64_t)a[f][s] * a[f][s];
      for (uint32_t b = 0; b < PLANES; b++) plane[(size_t)f * PLANES + b] |= (uint64_t)(a[f][s] >> b & 1) << s;
    }
    const uint64_t Q = N * B - A * A;
    offset[f] = (uint32_t)(n1 * A);
    scale[f] = Q ? (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, isqrt(((unsigned __int128)1 << 64) / Q)) : 0;
    mult[f] = f % 7 == 0 ? 0 : (uint32_t)(dcrx_rar::fin(seed + f) >> 40);
  }
  std::vector<uint32_t> obs(F + 1), most(P + 1), exceed(F + 1);
  std::vector<uint64_t> labels(P + 1), tail(E + 1), counts(4);
  // the edges: the largest distinct observed scores, ascending, as the stage picks them
  std::vector<uint32_t> seen;
  for (uint32_t f = 0; f < F; f++) seen.push_back(plain_score(a[f], C, N, offset[f], scale[f], alternative));
  std::sort(seen.begin(), seen.end());
  seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
  if (seen.size() > E) seen.erase(seen.begin(), seen.end() - E);
  E = (uint32_t)seen.size();
  seen.push_back(0);
  if (assoc_ranksum_host_run(N, C, alternative, F, plane.data(), offset.data(), scale.data(), mult.data(), E, seen.data(), P, seed, obs.data(),
                             labels.data(), most.data(), exceed.data(), tail.data(), counts.data())) {
    std::printf("%s: refused\n", what);
    return 1;
  }
  uint64_t differ = 0;
  std::vector<uint64_t> want_tail(E, 0);
  std::vector<uint32_t> want_exceed(F, 0);
  for (uint32_t f = 0; f < F; f++) differ += obs[f] != plain_score(a[f], C, N, offset[f], scale[f], alternative);
  for (uint32_t p = 0; p < P; p++) {
    const uint64_t L = plain_labels(seed, p, N, n1);
    differ += L != labels[p] || popcount(L) != n1;
    uint32_t hi = 0;
    for (uint32_t f = 0; f < F; f++) {
      const uint32_t t = plain_score(a[f], L, N, offset[f], scale[f], alternative);
      want_exceed[f] += t >= obs[f];
      if (!mult[f]) continue;
      hi = std::max(hi, t);
      for (uint32_t j = E; j-- > 0;)
        if (seen[j] <= t) { want_tail[j] += mult[f]; break; }
    }
    differ += hi != most[p];
  }
  for (uint32_t j = 0; j < E; j++) differ += want_tail[j] != tail[j];
  for (uint32_t f = 0; f < F; f++) differ += want_exceed[f] != exceed[f];
  std::printf("%s: N %u, n1 %u, alternative %u, F %u, P %u, %u edges, %llu wave adds, %llu + %llu flushes, %llu tail pairs: %llu differ\n", what, N,
              n1, alternative, F, P, E, (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2],
              (unsigned long long)counts[3], (unsigned long long)differ);
  return differ ? 1 : 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += one("two samples", 2, 1, 0, 5, 3, 4, 0);
  bad += one("the seam of a word's halves, less", 33, 0x1AAAAAAAAull, 1, 300, 257, 16, 7);
  bad += one("a full-width word, one case", 64, 1ull << 63, 2, 257, 300, 1024, ~0ull);
  bad += one("a full-width word, one control", 64, ~0ull >> 1, 0, 64, 65, 1, 3);
  bad += one("one past a slice and one past a block's relabelings", 16, 0xFF, 2, SLICE + 1, BLOCK_PERMS + 1, 40, 11);
  bad += one("no edges", 9, 0x3, 0, 50, 50, 0, 4);
  bad += one("no features", 9, 0x3, 0, 0, 10, 8, 5);
  bad += one("no permutations", 9, 0x3, 1, 10, 0, 8, 5);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}

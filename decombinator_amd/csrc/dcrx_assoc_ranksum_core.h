// dcrx_assoc_ranksum_core.h — what the rank-sum null of `associate --test rank-sum` (dcrx_assoc_ranksum.hip) shares with a plain
// host build (tests/host_assoc_ranksum): the bit planes of a feature's scores, the weighted popcount that is a rank sum, the
// fixed-point standardized score, the bounded search of the edges and the refusals both entries make.  The sizes of the walk,
// the selection of a relabeling (stage_keys, labels_from_keys), a block's slice and tile and perm_of are dcrx_assoc_core.h's:
// the relabelings are the presence null's, word for word.  include/dcrx.h "association, rank-sum" holds the contract.
#pragma once
#include <stdint.h>

#include "dcrx_assoc_core.h"

namespace dcrx_assoc_rs {

using namespace dcrx_assoc;

constexpr uint32_t PLANES = DCRX_ASSOC_RANKSUM_PLANES;      // a score a[f][s] is 0 .. 2 N - 2 <= 126: seven bits
constexpr uint32_t SHIFT = DCRX_ASSOC_RANKSUM_SHIFT;        // t = (u scale) >> SHIFT, u clamped to SHIFT bits
constexpr uint32_t MAX_EDGES = DCRX_ASSOC_RANKSUM_MAX_EDGES;
constexpr uint32_t RS_GROUP = 2;                            // features whose 11 words a wave asks for together
constexpr uint32_t U_MAX = (1u << SHIFT) - 1;
constexpr uint32_t NO_EDGE = 0xFFFFFFFFu;                   // edge_of: t is below every edge
constexpr uint32_t ALTERNATIVES = 3;                        // 0 greater, 1 less, 2 two-sided
constexpr uint64_t T_MAX = ((uint64_t)U_MAX * 0xFFFFFFFFull) >> SHIFT;
static_assert(2 * MAX_SAMPLES - 2 < (1u << PLANES), "a score fits the planes");
static_assert(SHIFT < 32 && (uint64_t)U_MAX * 0xFFFFFFFFull < (1ull << 63), "u scale fits 64 bits");
static_assert(T_MAX < NO_EDGE, "a score is a uint32 and never the value that stands for no edge");
static_assert((uint64_t)MAX_SAMPLES * MAX_SAMPLES * ((1u << PLANES) - 1) < (1ull << 31), "N W fits a signed 32-bit value, D a signed 64-bit one");
static_assert(SLICE % RS_GROUP == 0, "a slice is whole groups, but the last");
static_assert((uint64_t)SLICE * BLOCK_PERMS * (MAX_WEIGHT - 1) < (1ull << 63), "a block's tail cell cannot wrap");
static_assert(MAX_PERMUTATIONS < (1ull << 32), "exceed[f] is a uint32");

// W = the sum over the samples of L of a[s]: bit b of a[s] is bit s of planes[b]
DCRX_ASSOC_HD uint32_t weighted_sum(const uint64_t *planes, uint64_t L) {
  uint32_t W = 0;
  for (uint32_t b = 0; b < PLANES; b++) W += popcount(planes[b] & L) << b;
  return W;
}

// t of a rank sum W: D = N W - offset, u the alternative's side of D clamped to 0 .. 2^SHIFT - 1, t = (u scale) >> SHIFT
DCRX_ASSOC_HD uint32_t score_of(uint32_t W, uint32_t N, uint32_t offset, uint32_t scale, uint32_t alternative) {
  const int64_t D = (int64_t)((uint64_t)N * W) - (int64_t)offset;
  int64_t u = alternative == 0 ? D : alternative == 1 ? -D : (D < 0 ? -D : D);
  u = u < 0 ? 0 : u > (int64_t)U_MAX ? (int64_t)U_MAX : u;
  return (uint32_t)(((uint64_t)u * scale) >> SHIFT);
}

// the largest j with edges[j] <= t, NO_EDGE where there is none: at most 11 probes, every one inside 0 .. E - 1 whatever the
// array holds
DCRX_ASSOC_HD uint32_t edge_of(const uint32_t *edges, uint32_t E, uint32_t t) {
  uint32_t lo = 0, hi = E;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (edges[mid] <= t) lo = mid + 1; else hi = mid;
  }
  return lo ? lo - 1 : NO_EDGE;
}

// what both entries refuse of the scalars, in "association"'s order: 0, or 1 (DCRX_E_INVALID) .. 2 (DCRX_E_UNSUPPORTED)
DCRX_ASSOC_HD int refuse_scalars(uint32_t N, uint64_t C, uint32_t alternative, uint64_t F, uint32_t E, uint32_t P, const char **why) {
  if (N < 2 || N > MAX_SAMPLES) { *why = "2 .. DCRX_ASSOC_MAX_SAMPLES (64) samples"; return 1; }
  if (C & ~sample_bits(N)) { *why = "the case mask has a bit at or above the number of samples"; return 1; }
  if (C == 0 || C == sample_bits(N)) { *why = "the case mask holds no sample or every sample: 1 .. N - 1 cases"; return 1; }
  if (alternative >= ALTERNATIVES) { *why = "the alternative is 0 (greater), 1 (less) or 2 (two-sided)"; return 1; }
  if (E > MAX_EDGES) { *why = "more than DCRX_ASSOC_RANKSUM_MAX_EDGES (1024) edges"; return 1; }
  if (F >= MAX_FEATURES) { *why = "2^30 or more features"; return 2; }
  if (P > MAX_PERMUTATIONS) { *why = "more than DCRX_ASSOC_MAX_PERMUTATIONS (2^20) permutations"; return 2; }
  return 0;
}

}  // namespace dcrx_assoc_rs

// dcrx_assoc_core.h — what the permutation null of `associate` (dcrx_assoc.hip) shares with a plain host build
// (tests/host_assoc): the sizes of the walk, the two steps of the selection of a relabeling, the scoring of a (feature,
// relabeling) pair, a block's slice of the features and of the permutations, and the refusals both entries make.
// include/dcrx.h "association" holds the contract.
//
// The walk: a block of LANES lanes holds BLOCK_PERMS = LANES * PERMS_PER_LANE relabelings (lane t holds p0 + j LANES + t,
// j < PERMS_PER_LANE) and walks a slice of SLICE consecutive features against them.  The grid is (slices, permutation tiles).
// A block's tail cells are 64 bits wide: a block adds at most SLICE * BLOCK_PERMS multiplicities, each below 2^32, onto one
// cell: below 2^52, so nothing is flushed before the end.
#pragma once
#include <stdint.h>

#include "../../include/dcrx.h"
#include "dcrx_rarefy_core.h"

#if defined(__HIPCC__)
#define DCRX_ASSOC_HD __host__ __device__ __forceinline__
#else
#define DCRX_ASSOC_HD inline
#endif

namespace dcrx_assoc {

constexpr uint32_t LANES = 256;                            // a block of the walk
constexpr uint32_t LABEL_LANES = 64;                       // a block of the label selection: a lane a relabeling, its keys a column of LDS
constexpr uint32_t PERMS_PER_LANE = 4;                     // relabelings a lane keeps in registers, with their minima
constexpr uint32_t BLOCK_PERMS = LANES * PERMS_PER_LANE;   // relabelings of a block
constexpr uint32_t SLICE = 1024;                           // consecutive features of a block
constexpr uint32_t GROUP = 8;                              // features whose mask and multiplicity a wave asks for together
constexpr uint32_t MAX_SAMPLES = DCRX_ASSOC_MAX_SAMPLES;
constexpr uint32_t MAX_PERMUTATIONS = DCRX_ASSOC_MAX_PERMUTATIONS;
constexpr uint64_t MAX_FEATURES = 1ull << 30;
constexpr uint64_t MAX_WEIGHT = 1ull << 32;
constexpr uint32_t MAX_CELLS = (MAX_SAMPLES + 1) * (MAX_SAMPLES + 1);
static_assert(MAX_SAMPLES == 64, "a presence pattern and a relabeling are one uint64");
static_assert(MAX_CELLS <= 0xFFFF, "a rank fits the table's uint16");
static_assert(SLICE % GROUP == 0, "a slice is whole groups, but the last");
static_assert((uint64_t)SLICE * BLOCK_PERMS * (MAX_WEIGHT - 1) < (1ull << 63), "a block's tail cell cannot wrap");

DCRX_ASSOC_HD uint64_t sample_bits(uint32_t N) { return N >= 64 ? ~0ull : (1ull << N) - 1; }
DCRX_ASSOC_HD uint32_t cells(uint32_t N) { return (N + 1) * (N + 1); }
DCRX_ASSOC_HD uint32_t popcount(uint64_t x) { return dcrx_rar::popcount64(x); }

// L_p: the n1 samples of 0 .. N - 1 with the smallest key(seed, p, s) — dcrx_rarefy_core.h's key with p in the sample's place
// and s in the read's.  stage_keys writes the N keys of p once, `stride` entries apart (a lane's column of a block's LDS on the
// device, stride = the block's lanes, so that a wave's lanes read consecutive words; a plain array on the host);
// labels_from_keys reads them N^2 times: a sample is in when fewer than n1 samples have a smaller key (keys of one p are
// pairwise distinct).  Nothing indexed at run time lives in registers.
DCRX_ASSOC_HD void stage_keys(uint64_t *keys, uint32_t stride, uint64_t seed, uint32_t p, uint32_t N) {
  const uint64_t p_seed = dcrx_rar::sample_seed(seed, p);
  for (uint32_t s = 0; s < N; s++) keys[s * stride] = dcrx_rar::key_of(p_seed, s);
}
DCRX_ASSOC_HD uint64_t labels_from_keys(const uint64_t *keys, uint32_t stride, uint32_t N, uint32_t n1) {
  uint64_t L = 0;
  for (uint32_t s = 0; s < N; s++) {
    const uint64_t mine = keys[s * stride];
    uint32_t smaller = 0;
    for (uint32_t q = 0; q < N; q++) smaller += keys[q * stride] < mine ? 1u : 0u;
    if (smaller < n1) L |= 1ull << s;
  }
  return L;
}

// the score of feature mask M under labeling L: rank[m][k], m = popcount(M), k = popcount(M & L).  row_of gives m (N + 1), the
// same for every labeling; M has no bit at or above N, so the index is below (N + 1)^2 whatever L holds.
DCRX_ASSOC_HD uint32_t row_of(uint64_t M, uint32_t N) { return popcount(M) * (N + 1); }
DCRX_ASSOC_HD uint32_t score_at(const uint16_t *rank, uint32_t row, uint64_t M, uint64_t L) { return rank[row + popcount(M & L)]; }
DCRX_ASSOC_HD uint32_t score(const uint16_t *rank, uint32_t N, uint64_t M, uint64_t L) { return score_at(rank, row_of(M, N), M, L); }

// whether (m, k) is a cell the contract reads: max(0, m - (N - n1)) <= k <= min(m, n1)
DCRX_ASSOC_HD bool feasible(uint32_t N, uint32_t n1, uint32_t m, uint32_t k) {
  const uint32_t n0 = N - n1;
  return k <= m && k <= n1 && m - k <= n0;
}

// the grid of a walk over F features and P permutations, and block (bx, by)'s share of both: features [f0, f1), permutations
// from p0 on (lane t's j-th is p0 + j LANES + t, valid below P)
DCRX_ASSOC_HD uint32_t slices_for(uint64_t F) { return (uint32_t)((F + SLICE - 1) / SLICE); }
DCRX_ASSOC_HD uint32_t perm_tiles_for(uint32_t P) { return (P + BLOCK_PERMS - 1) / BLOCK_PERMS; }
DCRX_ASSOC_HD void slice_of(uint64_t F, uint32_t bx, uint32_t *f0, uint32_t *f1) {
  const uint64_t a = (uint64_t)bx * SLICE, b = a + SLICE;
  *f0 = (uint32_t)(a < F ? a : F);
  *f1 = (uint32_t)(b < F ? b : F);
}
DCRX_ASSOC_HD uint32_t perm_of(uint32_t by, uint32_t j, uint32_t t) { return by * BLOCK_PERMS + j * LANES + t; }

// what both entries refuse of the scalars: 0, or 1 (DCRX_E_INVALID) .. 2 (DCRX_E_UNSUPPORTED) with the reason
DCRX_ASSOC_HD int refuse_scalars(uint32_t N, uint64_t C, uint64_t F, uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, const char **why) {
  if (N < 2 || N > MAX_SAMPLES) { *why = "2 .. DCRX_ASSOC_MAX_SAMPLES (64) samples"; return 1; }
  if (C & ~sample_bits(N)) { *why = "the case mask has a bit at or above the number of samples"; return 1; }
  if (C == 0 || C == sample_bits(N)) { *why = "the case mask holds no sample or every sample: 1 .. N - 1 cases"; return 1; }
  if (n_ranks == 0 || n_ranks > cells(N)) { *why = "n_ranks is 1 .. (N + 1)^2"; return 1; }
  if (tail_ranks > n_ranks) { *why = "tail_ranks is above n_ranks"; return 1; }
  if (F >= MAX_FEATURES) { *why = "2^30 or more features"; return 2; }
  if (P > MAX_PERMUTATIONS) { *why = "more than DCRX_ASSOC_MAX_PERMUTATIONS (2^20) permutations"; return 2; }
  return 0;
}

}  // namespace dcrx_assoc

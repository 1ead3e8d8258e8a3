// dcrx_assoc_wide_core.h — what the wide permutation null of `associate` (dcrx_assoc_wide.hip: cohorts of up to 1024 samples)
// shares with a plain host build (tests/host_assoc_wide): the sizes of the walk, a sample's place in the words, the selection of
// a relabeling from an LDS-shaped array of keys, a run's row and cells with their flush, the scoring of a (feature, relabeling)
// pair, a block's share of the features and of the relabelings, and the refusals both entries make.
// include/dcrx.h "association, wide" holds the contract; the key, popcount and feasible() are the narrow layer's.
//
// The walk: a block of LANES lanes holds block_perms(W) = LANES * perms_per_lane(W) relabelings of W words each in registers
// (lane t holds p0 + j LANES + t, j < perms_per_lane(W)) and walks a slice of SLICE consecutive features against them in RUNS of
// equal popcount m.  Only the row of m is in LDS — N + 1 ranks of 32 bits — with one 64-bit tail cell per k beside it, whatever
// tail_ranks is; on a change of m the block flushes the non-zero cells onto tail[row[k]] (only where row[k] < tail_ranks) and
// stages the next row.  A block's cell takes at most SLICE * MAX_BLOCK_PERMS multiplicities below 2^32: below 2^52, so nothing
// is flushed for size.
#pragma once
#include <stdint.h>

#include "../../include/dcrx.h"
#include "dcrx_assoc_core.h"
#include "dcrx_rarefy_core.h"

#if defined(__HIPCC__)
#define DCRX_ASSOC_WIDE_UNROLL _Pragma("unroll")      // (a lane's few samples: static indices, registers)
#else
#define DCRX_ASSOC_WIDE_UNROLL
#endif

namespace dcrx_assoc_wide {

using dcrx_assoc::feasible;
using dcrx_assoc::popcount;

constexpr uint32_t LANES = 256;                            // a block of the walk, and of the label selection
constexpr uint32_t SLICE = 1024;                           // consecutive features of a block
constexpr uint32_t MAX_SAMPLES = DCRX_ASSOC_WIDE_MAX_SAMPLES;
constexpr uint32_t MAX_WORDS = MAX_SAMPLES / 64;
constexpr uint32_t LABEL_ITEMS = MAX_SAMPLES / LANES;      // samples a lane of the label selection answers for
constexpr uint32_t MAX_PERMUTATIONS = DCRX_ASSOC_MAX_PERMUTATIONS;
constexpr uint64_t MAX_FEATURES = dcrx_assoc::MAX_FEATURES;
constexpr uint64_t MAX_WEIGHT = dcrx_assoc::MAX_WEIGHT;
constexpr uint32_t MAX_CELLS = (MAX_SAMPLES + 1) * (MAX_SAMPLES + 1);
constexpr uint32_t NO_RUN = 0xFFFFFFFFu;                   // the popcount of the run before a block's first
// relabelings a lane keeps in registers: perms_per_lane(W) * W words of 64 bits are at most 32 VGPRs for the instances up to
// W = 16, so that no instance has scratch or spills (profiles/assoc_wide/resource_usage.md)
constexpr uint32_t perms_per_lane(uint32_t W) { return W <= 4 ? 4 : W <= 8 ? 2 : 1; }
constexpr uint32_t block_perms(uint32_t W) { return LANES * perms_per_lane(W); }
// features whose words and multiplicity a wave asks for together: 8 words of masks at most
constexpr uint32_t group(uint32_t W) { return W <= 8 ? 8 / W : 1; }
// (there is an instance of the walk per W = 1 .. 16, not per power of two: an instance of 16 words that served 9 .. 15 with the
// number of words as a run-time bound spilled 31 to 122 SGPRs in the three forms tried, a branch or a select and an address of
// its own per word; with W a constant a feature's words are loads at fixed offsets from one base and no instance spills.
// profiles/assoc_wide/resource_usage.md has the remarks of both)
constexpr uint32_t MAX_BLOCK_PERMS = block_perms(1);
static_assert(MAX_SAMPLES == 1024 && MAX_WORDS == 16, "sixteen words of 64 samples");
static_assert(MAX_SAMPLES % LANES == 0, "the label selection: whole samples a lane");
static_assert(LANES % 64 == 0, "a wave's ballot is one word of a relabeling");
static_assert((uint64_t)SLICE * MAX_BLOCK_PERMS * (MAX_WEIGHT - 1) < (1ull << 63), "a block's tail cell cannot wrap");
static_assert(block_perms(4) == MAX_BLOCK_PERMS && block_perms(5) < MAX_BLOCK_PERMS && block_perms(16) < MAX_BLOCK_PERMS,
              "MAX_BLOCK_PERMS bounds every instance");

DCRX_ASSOC_HD uint32_t words_for(uint32_t N) { return (N + 63) / 64; }
DCRX_ASSOC_HD uint32_t cells(uint32_t N) { return (N + 1) * (N + 1); }
// the samples of word w of N: all 64 but in the last, partial word
DCRX_ASSOC_HD uint64_t word_bits(uint32_t N, uint32_t w) {
  const uint32_t below = w * 64;
  return N <= below ? 0 : N - below >= 64 ? ~0ull : (1ull << (N - below)) - 1;
}

// L_p: the n1 samples with the smallest key(seed, p, s), the narrow layer's key.  stage_key writes sample s's key into the
// block's array; labels_in reads all N of them (every lane the same word at a time: a broadcast) and answers for lane t's
// LABEL_ITEMS samples: in when fewer than n1 samples have a smaller key (keys of one p are pairwise distinct).  Nothing indexed at run time lives in
// registers.
DCRX_ASSOC_HD uint64_t perm_seed(uint64_t seed, uint32_t p) { return dcrx_rar::sample_seed(seed, p); }
DCRX_ASSOC_HD void stage_key(uint64_t *keys, uint64_t p_seed, uint32_t s) { keys[s] = dcrx_rar::key_of(p_seed, s); }
DCRX_ASSOC_HD void labels_in(const uint64_t *keys, uint32_t N, uint32_t n1, uint32_t t, bool (&in)[LABEL_ITEMS]) {
  uint64_t mine[LABEL_ITEMS];
  uint32_t smaller[LABEL_ITEMS];
  DCRX_ASSOC_WIDE_UNROLL
  for (uint32_t i = 0; i < LABEL_ITEMS; i++) {      // lane t answers for the samples t + i LANES
    const uint32_t s = t + i * LANES;
    mine[i] = s < N ? keys[s] : 0;
    smaller[i] = 0;
  }
  for (uint32_t q = 0; q < N; q++) {
    const uint64_t key = keys[q];
  DCRX_ASSOC_WIDE_UNROLL
    for (uint32_t i = 0; i < LABEL_ITEMS; i++) smaller[i] += key < mine[i] ? 1u : 0u;
  }
  DCRX_ASSOC_WIDE_UNROLL
  for (uint32_t i = 0; i < LABEL_ITEMS; i++) in[i] = t + i * LANES < N && smaller[i] < n1;
}

// a run: the row of m, staged cell by cell (k <= m <= N: the index is below (N + 1)^2 whatever the table holds), and the flush
// of one cell onto the tail — the return value says whether the caller adds `c` to tail[*r]
DCRX_ASSOC_HD uint32_t row_cell(const uint32_t *rank, uint32_t N, uint32_t m, uint32_t k) { return rank[m * (N + 1) + k]; }
DCRX_ASSOC_HD bool flush_cell(uint64_t c, uint32_t row_k, uint32_t tail_ranks) { return c != 0 && row_k < tail_ranks; }

// the grid of a walk over F features and P permutations of W words (W: the instance's), and block (bx, by)'s share of both
DCRX_ASSOC_HD uint32_t slices_for(uint64_t F) { return (uint32_t)((F + SLICE - 1) / SLICE); }
DCRX_ASSOC_HD uint32_t perm_tiles_for(uint32_t P, uint32_t W) { return (P + block_perms(W) - 1) / block_perms(W); }
DCRX_ASSOC_HD void slice_of(uint64_t F, uint32_t bx, uint32_t *f0, uint32_t *f1) {
  const uint64_t a = (uint64_t)bx * SLICE, b = a + SLICE;
  *f0 = (uint32_t)(a < F ? a : F);
  *f1 = (uint32_t)(b < F ? b : F);
}
DCRX_ASSOC_HD uint32_t perm_of(uint32_t by, uint32_t j, uint32_t t, uint32_t W) { return by * block_perms(W) + j * LANES + t; }

// what both entries refuse of the scalars: 0, or 1 (DCRX_E_INVALID) .. 2 (DCRX_E_UNSUPPORTED) with the reason
DCRX_ASSOC_HD int refuse_scalars(uint32_t N, uint64_t F, uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, const char **why) {
  if (N < 2 || N > MAX_SAMPLES) { *why = "2 .. DCRX_ASSOC_WIDE_MAX_SAMPLES (1024) samples"; return 1; }
  if (n_ranks == 0 || n_ranks > cells(N)) { *why = "n_ranks is 1 .. (N + 1)^2"; return 1; }
  if (tail_ranks > n_ranks) { *why = "tail_ranks is above n_ranks"; return 1; }
  if (F >= MAX_FEATURES) { *why = "2^30 or more features"; return 2; }
  if (P > MAX_PERMUTATIONS) { *why = "more than DCRX_ASSOC_MAX_PERMUTATIONS (2^20) permutations"; return 2; }
  return 0;
}
// the case mask, judged after the null arrays (it is one): `strict` (the host entry) refuses a bit at or above N, the device
// entry cuts it off; both refuse n1 of 0 or N.  *n1_out: the cases among the N samples.
DCRX_ASSOC_HD int refuse_cases(uint32_t N, const uint64_t *C, bool strict, uint32_t *n1_out, const char **why) {
  uint32_t n1 = 0;
  for (uint32_t w = 0; w < words_for(N); w++) {
    if (strict && (C[w] & ~word_bits(N, w))) { *why = "the case mask has a bit at or above the number of samples"; return 1; }
    n1 += popcount(C[w] & word_bits(N, w));
  }
  *n1_out = n1;
  if (n1 == 0 || n1 == N) { *why = "the case mask holds no sample or every sample: 1 .. N - 1 cases"; return 1; }
  return 0;
}

}  // namespace dcrx_assoc_wide

// dcrx_rarefy_core.h — what the downsampling step (`overlap --downsample`, dcrx_rarefy.hip) shares with a plain host build
// (tests/host_rarefy): the key of a read, the digits the selection looks at, the sizes of the walk over the reads, and a
// lane's look-up of the row that owns a read.  include/dcrx.h "downsample" holds the contract.
//
// The reads of all samples together form one index space 0 .. total - 1 in row order: row i owns [G[i], G[i + 1]), G the
// exclusive sum of the weights (m + 1 entries).  The space is cut into tiles of TILE consecutive reads; a block stages the
// SLOTS offsets that follow its tile's first row, and a lane finds the row of a read among them — or, behind more rows than
// are staged (rows of weight 0, rows of weight 1), by a search over G.
#pragma once
#include <stdint.h>

#include "../../include/dcrx.h"

#if defined(__HIPCC__)
#define DCRX_RAREFY_HD __host__ __device__ __forceinline__
#else
#define DCRX_RAREFY_HD inline
#endif

namespace dcrx_rar {

constexpr uint32_t LANES = 256;                   // a block (dcrx_group.h's BLOCK)
constexpr uint32_t PER_LANE = 8;                  // reads of a tile a lane takes: g0 + j LANES + lane, j < PER_LANE
constexpr uint32_t TILE = LANES * PER_LANE;       // consecutive reads of a tile
constexpr uint32_t SLOTS = 512;                   // row ends staged per tile
constexpr uint32_t GRID = 1024;                   // blocks of a walk; block b takes tiles [b n, (b + 1) n), n = ceil(tiles / blocks)
constexpr uint32_t BIN_BITS = 12;
constexpr uint32_t BINS = 1u << BIN_BITS;         // histogram bins of one selection level: one digit of the key
constexpr uint32_t LEVELS = 5;                    // levels at most: 60 bits decided leave 16 keys at most in a bin
constexpr uint32_t CANDIDATES = 4096;             // keys of a sample's threshold bin that are written out, at most
constexpr uint32_t MAX_SAMPLES = DCRX_DOWNSAMPLE_MAX_SAMPLES;
constexpr uint64_t MAX_ROWS = 1ull << 30;
constexpr uint64_t MAX_READS = 1ull << 40;
constexpr uint64_t SAMPLE_STEP = 0xD1B54A32D192ED03ull, READ_STEP = 0x9E3779B97F4A7C15ull;
static_assert((1ull << (64 - BIN_BITS * LEVELS)) <= CANDIDATES, "the last level's bin fits the candidates");
static_assert(BINS % LANES == 0 && CANDIDATES % LANES == 0 && SLOTS % LANES == 0, "a lane takes a whole share");

// the finisher of splitmix64: a bijection of the 64-bit integers (xor-shifts and odd multipliers)
DCRX_RAREFY_HD uint64_t fin(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// key(s, r) = fin(sample_seed(seed, s) + (r + 1) READ_STEP): READ_STEP is odd, so r -> the sum is injective mod 2^64 and the
// keys of one sample are pairwise distinct
DCRX_RAREFY_HD uint64_t sample_seed(uint64_t seed, uint64_t s) { return fin(seed + (s + 1) * SAMPLE_STEP); }
DCRX_RAREFY_HD uint64_t key_of(uint64_t s_seed, uint64_t r) { return fin(s_seed + (r + 1) * READ_STEP); }
DCRX_RAREFY_HD uint64_t key(uint64_t seed, uint64_t s, uint64_t r) { return key_of(sample_seed(seed, s), r); }

// the digit of level `level` (0: the top BIN_BITS bits), and the `levels` digits above it as one number
DCRX_RAREFY_HD uint32_t digit(uint64_t k, uint32_t level) { return (uint32_t)(k >> (64 - BIN_BITS * (level + 1))) & (BINS - 1); }
DCRX_RAREFY_HD uint64_t prefix_of(uint64_t k, uint32_t levels) { return levels ? k >> (64 - BIN_BITS * levels) : 0; }

DCRX_RAREFY_HD uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
DCRX_RAREFY_HD uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// the tiles of block `block` of `blocks`: [first, last)
DCRX_RAREFY_HD void block_tiles(uint64_t total, uint32_t block, uint32_t blocks, uint32_t *first, uint32_t *last) {
  const uint32_t tiles = (uint32_t)((total + TILE - 1) / TILE), each = (tiles + blocks - 1) / blocks;
  *first = min_u32(tiles, block * each);      // (each * blocks < 2^29 + 2^10)
  *last = min_u32(tiles, *first + each);
}

// the smallest i in [lo, hi] with off[i] > g (off ascending; off[hi] > g is the caller's)
DCRX_RAREFY_HD uint32_t first_above(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t g) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] > g) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// the smallest i in [0, m] with sample[i] >= s (m where there is none)
DCRX_RAREFY_HD uint32_t first_row_of(const uint32_t *__restrict__ sample, uint32_t m, uint32_t s) {
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (sample[mid] >= s) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// the row that owns read g < G[m]: ends[k] = G[min(i0 + 1 + k, m)], k < n_ends, are the tile's staged ends (i0: the row of
// the tile's first read); behind the staged ends a search over G from the first row that is not staged.  Always < m.
DCRX_RAREFY_HD uint32_t row_of(const uint64_t *ends, uint32_t n_ends, const uint64_t *__restrict__ G, uint32_t i0, uint32_t m, uint64_t g) {
  uint32_t k = 0;      // the first staged end above g
  for (uint32_t hi = n_ends; k < hi;) {
    const uint32_t mid = k + (hi - k) / 2;
    if (ends[mid] > g) hi = mid;
    else k = mid + 1;
  }
  const uint32_t row = k < n_ends ? i0 + k : first_above(G, min_u32(i0 + 1 + n_ends, m), m, g) - 1;
  return min_u32(row, m - 1);
}

// ---- a wave's runs of lanes in one row (the count pass): `heads` has a bit per lane that starts a run, `keeps` a bit per
// lane whose read is kept; the kept reads of the run that starts at `lane` (a head)
DCRX_RAREFY_HD uint32_t popcount64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}
DCRX_RAREFY_HD uint32_t run_kept(uint64_t heads, uint64_t keeps, uint32_t lane) {
  const uint64_t above = lane == 63 ? 0 : heads & (~0ull << (lane + 1));      // the heads behind this one
  const uint64_t upto = above ? (above & (0 - above)) - 1 : ~0ull;            // the lanes below the next head
  return popcount64(keeps & upto & (~0ull << lane));
}

}  // namespace dcrx_rar

// dcrx_overlap_core.h — the per-row and per-pair code of the overlap step (`overlap`, dcrx_overlap.hip), shared by the
// kernels and a plain host build (tests/host_overlap).
//
// Per row (class, bytes): the 64-bit hash of its key — a filter that puts candidates next to each other, never a verdict —
// and the full compare of two keys (class, length, then every byte as it is).
// Per pair of cells: the 32/32 split of the product of two weights < 2^32, and where a pair of samples lies in a plane:
// a full S x S plane is row major, a symmetric plane is kept as a triangle with its diagonal.
// Per cell of the pair kernel: the lane's look-ups of where its group ends.
#pragma once
#include <stdint.h>

#include "../../include/dcrx.h"

#if defined(__HIPCC__)
#define DCRX_OVERLAP_HD __host__ __device__ __forceinline__
#else
#define DCRX_OVERLAP_HD inline
#endif

namespace dcrx_ovl {

constexpr uint32_t MAX_SAMPLES = DCRX_OVERLAP_MAX_SAMPLES;
constexpr uint32_t SAMPLE_BITS = 6;
static_assert((1u << SAMPLE_BITS) == MAX_SAMPLES, "a sample takes six key bits");
constexpr uint32_t P_SHARED = DCRX_OVERLAP_SHARED, P_SHARED_WEIGHT = DCRX_OVERLAP_SHARED_WEIGHT, P_MIN_WEIGHT = DCRX_OVERLAP_MIN_WEIGHT,
                   P_PROD_LO = DCRX_OVERLAP_PROD_LO, P_PROD_HI = DCRX_OVERLAP_PROD_HI, PLANES = DCRX_OVERLAP_PLANES;

DCRX_OVERLAP_HD uint64_t hash_mix(uint64_t h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// the hash of the key (class, bytes): equal keys hash equal; nothing else is promised
DCRX_OVERLAP_HD uint64_t key_hash(uint32_t cls, const uint8_t *s, uint64_t len) {
  uint64_t h = hash_mix(((uint64_t)cls << 32) ^ (len * 0x9e3779b97f4a7c15ull) ^ 0x2545f4914f6cdd1dull);
  for (uint64_t p = 0; p < len; p++) h = (h ^ s[p]) * 0x100000001b3ull;
  return hash_mix(h);
}

// the keys in full: class, length, every byte as it is
DCRX_OVERLAP_HD bool key_equal(uint32_t cls_a, const uint8_t *a, uint64_t len_a, uint32_t cls_b, const uint8_t *b, uint64_t len_b) {
  if (cls_a != cls_b || len_a != len_b) return false;
  for (uint64_t p = 0; p < len_a; p++)
    if (a[p] != b[p]) return false;
  return true;
}

// w_a w_b for weights < 2^32, as (mod 2^32, >> 32)
DCRX_OVERLAP_HD void product_split(uint64_t wa, uint64_t wb, uint64_t *lo, uint64_t *hi) {
  const uint64_t p = wa * wb;
  *lo = p & 0xFFFFFFFFull;
  *hi = p >> 32;
}

// where (a, b) lies in a row-major S x S plane, and where {a, b} lies in a triangle with its diagonal (row max(a, b) holds
// max(a, b) + 1 entries)
DCRX_OVERLAP_HD uint32_t full_index(uint32_t S, uint32_t a, uint32_t b) { return a * S + b; }
DCRX_OVERLAP_HD uint32_t tri_index(uint32_t a, uint32_t b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return hi * (hi + 1) / 2 + lo;
}
DCRX_OVERLAP_HD uint32_t tri_size(uint32_t S) { return S * (S + 1) / 2; }

// the sort key of a row's cell: (group, sample), 36 bits at most
DCRX_OVERLAP_HD uint64_t cell_key(uint32_t group, uint32_t sample) { return ((uint64_t)group << SAMPLE_BITS) | sample; }

// ---- the pair kernel's look-ups (a lane's; tests/host_overlap walks the cells with them) ----

DCRX_OVERLAP_HD uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the smallest g in [lo, hi] with off[g] > c (off ascending; off[hi] > c is the caller's)
DCRX_OVERLAP_HD uint32_t first_above(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint32_t c) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] > c) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// where the walk of cell c stops: the end of c's group.  ends[k] = cell_off[min(g_first + 1 + k, n_groups)], k < n_ends, are
// the tile's staged ends (g_first: the group of the tile's first cell); a lane whose group's end is not among them — behind
// empty groups — searches cell_off from the first group that is not staged.  Never past n_cells nor past c + MAX_SAMPLES (a
// group has at most 64 cells: a walk never runs away on bad offsets).
DCRX_OVERLAP_HD uint32_t group_end(const uint32_t *ends, uint32_t n_ends, const uint32_t *__restrict__ cell_off, uint32_t g_first,
                                   uint32_t n_groups, uint32_t n_cells, uint32_t c) {
  uint32_t k = 0;      // the first staged end above c
  for (uint32_t hi = n_ends; k < hi;) {
    const uint32_t mid = k + (hi - k) / 2;
    if (ends[mid] > c) hi = mid;
    else k = mid + 1;
  }
  const uint32_t end = k < n_ends ? ends[k] : cell_off[first_above(cell_off, min_u32(g_first + 1 + n_ends, n_groups), n_groups, c)];
  return min_u32(min_u32(end, n_cells), c + MAX_SAMPLES);
}

}  // namespace dcrx_ovl

// Test-only: the kernel's per-pair function, tile rule and k clamp (dcrx_umi_core.h) built by g++, for checks against a
// plain DP on the host.
#include "../../decombinator_amd/csrc/dcrx_umi_core.h"

using namespace dcrx_umi;

enum { TILE = 256, REC_WORDS = 16, TILE_WORDS = 8 };          // DCRX_UMI_TILE, _REC_WORDS, _TILE_WORDS of include/dcrx.h

extern "C" int umi_host_pair_distance(const uint32_t *a, const uint32_t *b, int32_t k) { return pair_distance(a, b, k); }

extern "C" int umi_host_tiles_may_match(const uint32_t *ta, const uint32_t *tb, int32_t k) { return tiles_may_match(ta, tb, clamp_k(k)); }

// The kernel's iteration space as a plain loop over dcrx_umi_encode's output: row tile rt, column tiles ct >= rt that the
// tile rule lets through, each row record against each column record (in the diagonal tile: the ones after it).  Returns the
// number of pairs within k and writes the first `cap` keys (min index << 32 | max index).
extern "C" uint64_t umi_host_walk(const uint32_t *recs, const uint32_t *tiles, uint32_t n_tiles, int32_t k, uint64_t *out, uint64_t cap) {
  k = clamp_k(k);
  uint64_t total = 0;
  for (uint32_t rt = 0; rt < n_tiles; rt++)
    for (uint32_t ct = rt; ct < n_tiles; ct++) {
      const uint32_t *rtile = tiles + rt * TILE_WORDS, *ctile = tiles + ct * TILE_WORDS;
      if (!tiles_may_match(rtile, ctile, k)) continue;
      for (uint32_t r = 0; r < rtile[6]; r++)
        for (uint32_t p = ct == rt ? r + 1 : 0; p < ctile[6]; p++) {
          const uint32_t *a = recs + ((uint64_t)rt * TILE + r) * REC_WORDS, *b = recs + ((uint64_t)ct * TILE + p) * REC_WORDS;
          if (pair_distance(a, b, k) > k) continue;
          const uint64_t lo = a[W_INDEX] < b[W_INDEX] ? a[W_INDEX] : b[W_INDEX], hi = a[W_INDEX] ^ b[W_INDEX] ^ lo;
          if (total < cap) out[total] = (lo << 32) | hi;
          total++;
        }
    }
  return total;
}

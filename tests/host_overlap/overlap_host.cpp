// Test-only: the overlap step's per-row and per-pair code (dcrx_overlap_core.h) built by g++, for a check against Python on
// the host, and the pair kernel's walk over the cells written serially around the look-ups the kernel's lanes make.
#include <algorithm>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_overlap_core.h"

using namespace dcrx_ovl;

constexpr uint32_t TILE = 256;      // the pair kernel's tile: BLOCK cells (dcrx_group.h)

extern "C" {
uint32_t overlap_host_max_samples(void) { return MAX_SAMPLES; }
uint32_t overlap_host_sample_bits(void) { return SAMPLE_BITS; }
uint32_t overlap_host_planes(void) { return PLANES; }
uint64_t overlap_host_hash(uint32_t cls, const uint8_t *s, uint64_t len) { return key_hash(cls, s, len); }
int overlap_host_equal(uint32_t cls_a, const uint8_t *a, uint64_t len_a, uint32_t cls_b, const uint8_t *b, uint64_t len_b) {
  return key_equal(cls_a, a, len_a, cls_b, b, len_b) ? 1 : 0;
}
void overlap_host_product(uint64_t wa, uint64_t wb, uint64_t *lo, uint64_t *hi) { product_split(wa, wb, lo, hi); }
uint32_t overlap_host_full_index(uint32_t S, uint32_t a, uint32_t b) { return full_index(S, a, b); }
uint32_t overlap_host_tri_index(uint32_t a, uint32_t b) { return tri_index(a, b); }
uint32_t overlap_host_tri_size(uint32_t S) { return tri_size(S); }
uint64_t overlap_host_cell_key(uint32_t group, uint32_t sample) { return cell_key(group, sample); }

// overlap_pairs_kernel's walk (dcrx_overlap.hip) in its plainest serial form, both PARTs at once: per block its tiles; per
// tile g_first and the staged ends; per cell the look-up the kernel's lane makes (group_end), the diagonal terms and the walk
// to the group's end, onto the block's planes — triangles and a full plane sized by smax, as in LDS —; then the block's one
// flush onto planes (5 x S x S).  Every buffer has the kernel's size and no more, so a look-up outside `ends` or a plane is
// outside a heap block here.  0, or -1 on arguments the launch never makes.
int overlap_host_pairs(uint32_t n_groups, const uint32_t *cell_off, const uint32_t *cell_sample, const uint32_t *cell_weight, uint32_t S,
                       uint32_t smax, uint32_t grid, uint64_t *planes) {
  if (S < 1 || S > MAX_SAMPLES || smax < S || smax > MAX_SAMPLES || !grid || !n_groups) return -1;
  const uint32_t TRI = tri_size(smax), FULL = smax * smax, SS = S * S;
  const uint32_t n_cells = cell_off[n_groups];
  const uint32_t tiles = (n_cells + TILE - 1) / TILE;
  for (uint32_t block = 0; block < grid; block++) {
    std::vector<uint32_t> ends(TILE), cnt(TRI, 0);
    std::vector<uint64_t> min_w(TRI, 0), shared_w(FULL, 0), prod_lo(TRI, 0), prod_hi(TRI, 0);
    for (uint32_t tile = block; tile < tiles; tile += grid) {
      const uint32_t c0 = tile * TILE;
      const uint32_t g_first = first_above(cell_off, 0, n_groups, c0) - 1;
      for (uint32_t t = 0; t < TILE; t++) ends[t] = cell_off[std::min(g_first + 1 + t, n_groups)];
      for (uint32_t t = 0; t < TILE; t++) {
        const uint32_t c = c0 + t;
        if (c >= n_cells) continue;
        const uint32_t end = group_end(ends.data(), TILE, cell_off, g_first, n_groups, n_cells, c);
        const uint32_t a = cell_sample[c];
        if (a >= S) continue;
        const uint64_t wa = cell_weight[c];
        for (uint32_t q = c; q < end; q++) {      // (q = c: the diagonal terms)
          const uint32_t b = cell_sample[q];
          if (b >= S) continue;
          const uint64_t wb = cell_weight[q];
          const uint32_t ti = tri_index(a, b);
          uint64_t lo, hi;
          product_split(wa, wb, &lo, &hi);
          cnt.at(ti) += 1;
          shared_w.at(full_index(S, a, b)) += wa;
          if (q != c) shared_w.at(full_index(S, b, a)) += wb;
          min_w.at(ti) += std::min(wa, wb);
          prod_lo.at(ti) += lo;
          prod_hi.at(ti) += hi;
        }
      }
    }
    for (uint32_t idx = 0; idx < SS; idx++) {
      const uint32_t ti = tri_index(idx / S, idx % S);
      planes[(size_t)P_SHARED * SS + idx] += cnt.at(ti);
      planes[(size_t)P_SHARED_WEIGHT * SS + idx] += shared_w.at(idx);
      planes[(size_t)P_MIN_WEIGHT * SS + idx] += min_w.at(ti);
      planes[(size_t)P_PROD_LO * SS + idx] += prod_lo.at(ti);
      planes[(size_t)P_PROD_HI * SS + idx] += prod_hi.at(ti);
    }
  }
  return 0;
}
}

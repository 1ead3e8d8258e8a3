// Test-only: the overlap step's per-row and per-pair code (dcrx_overlap_core.h) built by g++, for a check against Python on
// the host.
#include "../../decombinator_amd/csrc/dcrx_overlap_core.h"

using namespace dcrx_ovl;

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
}

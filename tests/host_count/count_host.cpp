// Test-only: the count kernels' per-key code (dcrx_count_core.h) built by g++, for a check against Python on the host.
#include "../../decombinator_amd/csrc/dcrx_count_core.h"

extern "C" {
void count_host_insert(const uint8_t *packed, uint32_t len, uint32_t frame, uint32_t ins_start, uint32_t ins_len,
                       const uint16_t *exc_pos, const uint8_t *exc_chr, uint32_t n_exc, uint8_t *out) {
  dcrx_count::insert_bytes(packed, len, frame, ins_start, ins_len, exc_pos, exc_chr, n_exc, out);
}
uint64_t count_host_header(uint32_t v, uint32_t j, uint32_t vdel, uint32_t jdel, uint32_t ins_len) {
  return dcrx_count::header(v, j, vdel, jdel, ins_len);
}
uint64_t count_host_hash(uint64_t hdr, const uint8_t *ins, uint32_t ins_len) { return dcrx_count::key_hash(hdr, ins, ins_len); }
int count_host_equal(uint64_t hdr_a, const uint8_t *a, uint64_t hdr_b, const uint8_t *b) {
  return dcrx_count::key_equal(hdr_a, a, hdr_b, b) ? 1 : 0;
}
}

// Test-only: the CDR3 network's per-node and per-pair code (dcrx_cdr3net_core.h) built by g++, for a check against Python on
// the host.
#include "../../decombinator_amd/csrc/dcrx_cdr3net_core.h"

using namespace dcrx_cdr3net;

extern "C" {
uint32_t cdr3net_host_words(void) { return WORDS; }
uint32_t cdr3net_host_max_len(void) { return MAX_LEN; }
uint64_t cdr3net_host_key_out_of_reach(void) { return KEY_OUT_OF_REACH; }
uint32_t cdr3net_host_key_bits(void) { return KEY_BITS; }
int cdr3net_host_in_reach(uint64_t len) { return in_reach(len) ? 1 : 0; }
uint64_t cdr3net_host_key(uint32_t cls, uint64_t len) { return node_key(cls, len); }
void cdr3net_host_pack(const uint8_t *s, uint64_t len, uint32_t *out) { pack(s, len, out); }
uint32_t cdr3net_host_distance(const uint32_t *a, const uint32_t *b, uint32_t limit) { return distance(a, b, limit); }
}

// Test-only: the CDR3 network's Levenshtein pair test and what it stands on (dcrx_cdr3net_core.h) built by g++, for a check
// against a plain DP in Python on the host.
#include "../../decombinator_amd/csrc/dcrx_cdr3net_core.h"

using namespace dcrx_cdr3net;

extern "C" {
// a string of 0 .. 32 bytes into eight words as the kernels hold it (zero beyond the length; pack() alone refuses length 0)
void cdr3lev_host_pack(const uint8_t *s, uint64_t len, uint32_t *out) {
  for (uint32_t w = 0; w < WORDS; w++) out[w] = 0;
  for (uint32_t p = 0; p < (uint32_t)len && p < MAX_LEN; p++) out[p / 4] |= (uint32_t)s[p] << (8 * (p % 4));
}
uint32_t cdr3lev_host_lev_within(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb, uint32_t limit) {
  return lev_within(a, la, b, lb, limit);
}
// many pairs at once: pair k is strings 2k and 2k + 1 of `text` (offsets off[2n + 1]); out[k] = lev_within
void cdr3lev_host_lev_within_many(const uint8_t *text, const uint64_t *off, uint64_t n, uint32_t limit, uint32_t *out) {
  for (uint64_t k = 0; k < n; k++) {
    uint32_t a[WORDS], b[WORDS];
    const uint64_t la = off[2 * k + 1] - off[2 * k], lb = off[2 * k + 2] - off[2 * k + 1];
    cdr3lev_host_pack(text + off[2 * k], la, a);
    cdr3lev_host_pack(text + off[2 * k + 1], lb, b);
    out[k] = lev_within(a, (uint32_t)la, b, (uint32_t)lb, limit);
  }
}
uint32_t cdr3lev_host_presence(const uint32_t *w, uint32_t len) { return presence(w, len); }
int cdr3lev_host_presence_allows(uint32_t pa, uint32_t pb, uint32_t limit) { return presence_allows(pa, pb, limit) ? 1 : 0; }
uint64_t cdr3lev_host_key_class(uint64_t key) { return key_class(key); }
uint32_t cdr3lev_host_key_length(uint64_t key) { return key_length(key); }
}

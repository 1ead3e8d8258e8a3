// Test-only: the motif step's shared code (dcrx_motif_core.h) built by g++, for a check against Python on the host.
#include <cstring>

#include "../../decombinator_amd/csrc/dcrx_motif_core.h"

using namespace dcrx_motif;

extern "C" {

uint32_t motif_host_block() { return BLOCK; }
uint32_t motif_host_bins() { return BINS; }
uint32_t motif_host_levels() { return LEVELS; }
uint32_t motif_host_candidates() { return CANDIDATES; }
uint32_t motif_host_motifs() { return MOTIFS; }
uint32_t motif_host_max_windows() { return MAX_WINDOWS; }
uint32_t motif_host_max_chunk() { return MAX_CHUNK; }
uint32_t motif_host_chunk_of(uint64_t n) { return chunk_of(n); }
uint32_t motif_host_digit(uint64_t k, uint32_t level) { return digit(k, level); }
uint64_t motif_host_prefix(uint64_t k, uint32_t levels) { return prefix_of(k, levels); }
uint32_t motif_host_window_count(uint32_t L, uint32_t N, uint32_t C, uint32_t k) { return window_count(L, N, C, k); }

// 1: the unit takes part, 0: it does not
int motif_host_takes_part(const uint8_t *s, uint64_t len) {
  uint32_t w[WORDS];
  dcrx_cdr3net::pack(s, len, w);
  return takes_part(w, len) ? 1 : 0;
}

// the code of the k letters at p of a unit that takes part
uint32_t motif_host_code_at(const uint8_t *s, uint64_t len, uint32_t p, uint32_t k) {
  uint32_t w[WORDS];
  dcrx_cdr3net::pack(s, len, w);
  return code_at(w, 1, p, k);
}
uint32_t motif_host_motif_id(uint32_t k, uint32_t code) { return motif_id(k, code); }
uint32_t motif_host_id_k(uint32_t id) { return id_k(id); }
uint32_t motif_host_id_code(uint32_t id) { return id_code(id); }

// a unit's motifs of one k, each once, in window order: their numbers into out (MAX_WINDOWS entries), their count returned;
// -1 for a unit that takes no part
int motif_host_unit_motifs(const uint8_t *s, uint64_t len, uint32_t N, uint32_t C, uint32_t k, uint32_t *out) {
  uint32_t w[WORDS], codes[MAX_WINDOWS];
  dcrx_cdr3net::pack(s, len, w);
  if (!takes_part(w, len)) return -1;
  int n = 0;
  unit_motifs(w, 1, (uint32_t)len, N, C, k, codes, 1, [&](uint32_t id) { out[n++] = id; });
  return n;
}

}  // extern "C"

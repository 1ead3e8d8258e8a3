// Test-only: the host walk of `match` (../host_cdr3walk/cdr3walk_host.h: Bipartite with Hamming or Levenshtein) and the look-ups
// of dcrx_cdr3match_core.h built by g++, for a check against Python on the host.
#include "../host_cdr3walk/cdr3walk_host.h"

using namespace cdr3walk_host;

extern "C" {
uint32_t cdr3match_host_queries(void) { return QUERIES; }
uint32_t cdr3match_host_tile(void) { return TILE; }
uint32_t cdr3match_host_first_at_or_above(const uint64_t *key, uint32_t n, uint64_t k, int lev) {
  return lev ? first_at_or_above<true>(key, n, k) : first_at_or_above<false>(key, n, k);
}
// degree (m_q), hit_off (m_q + 1) and, where they fit hit_cap, the hits; returns the need
uint64_t cdr3match_host_match(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q,
                              const uint32_t *q_cls, const uint64_t *q_off, const uint8_t *q_text, uint32_t limit, uint32_t metric,
                              uint32_t *degree, uint64_t *hit_off, uint32_t *hit, uint64_t hit_cap) {
  return flat(match(m_t, t_cls, t_off, t_text, m_q, q_cls, q_off, q_text, limit, metric), degree, hit_off, hit, nullptr, hit_cap);
}
}

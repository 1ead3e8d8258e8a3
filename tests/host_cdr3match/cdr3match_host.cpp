// Test-only: the host walk of `match` (cdr3match_walk.h) and the look-ups of dcrx_cdr3match_core.h built by g++, for a check
// against Python on the host.
#include "cdr3match_walk.h"

using namespace cdr3match_host;

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
  const auto hits = match(m_t, t_cls, t_off, t_text, m_q, q_cls, q_off, q_text, limit, metric);
  uint64_t at = 0;
  for (uint64_t i = 0; i < m_q; i++) {
    degree[i] = (uint32_t)hits[i].size();
    hit_off[i] = at;
    for (uint32_t j : hits[i]) {
      if (at < hit_cap) hit[at] = j;
      at++;
    }
  }
  hit_off[m_q] = at;
  return at;
}
}

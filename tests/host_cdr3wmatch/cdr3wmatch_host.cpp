// Test-only: the host walk of the weighted `match` (../host_cdr3walk/cdr3walk_host.h: Bipartite with Weighted) and the pair test
// of dcrx_cdr3w_core.h built by g++, for a check against Python on the host.
#include "../host_cdr3walk/cdr3walk_host.h"

using namespace cdr3walk_host;

extern "C" {
// weighted_within of two byte strings (1 .. 32 bytes each), as the kernel calls it: a packed in words, b as 32 bytes
uint32_t cdr3wmatch_host_within(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, const uint8_t *sub, uint32_t gap,
                                uint32_t ntrim, uint32_t ctrim, uint32_t radius) {
  uint32_t wa[WORDS], wb[WORDS];
  pack(a, la, wa);
  pack(b, lb, wb);
  uint8_t other[MAX_LEN];
  std::memcpy(other, wb, MAX_LEN);
  return weighted_within(wa, la, other, lb, Cost{sub, gap, ntrim, ctrim}, radius);
}
// ... of n pairs: strings of 32 bytes each (zero behind the length), out[n]
void cdr3wmatch_host_within_many(uint64_t n, const uint8_t *a, const uint8_t *la, const uint8_t *b, const uint8_t *lb, const uint8_t *sub,
                                 uint32_t gap, uint32_t ntrim, uint32_t ctrim, uint32_t radius, uint32_t *out) {
  for (uint64_t k = 0; k < n; k++)
    out[k] = cdr3wmatch_host_within(a + k * MAX_LEN, la[k], b + k * MAX_LEN, lb[k], sub, gap, ntrim, ctrim, radius);
}
// ... of every one of n_a strings of la bytes (the own ones) against every one of n_b strings of lb bytes: out[n_a * n_b]
void cdr3wmatch_host_within_grid(uint64_t n_a, const uint8_t *a, uint32_t la, uint64_t n_b, const uint8_t *b, uint32_t lb,
                                 const uint8_t *sub, uint32_t gap, uint32_t ntrim, uint32_t ctrim, uint32_t radius, uint32_t *out) {
  for (uint64_t i = 0; i < n_a; i++)
    for (uint64_t j = 0; j < n_b; j++)
      out[i * n_b + j] = cdr3wmatch_host_within(a + i * MAX_LEN, la, b + j * MAX_LEN, lb, sub, gap, ntrim, ctrim, radius);
}
int cdr3wmatch_host_letters(const uint8_t *a, uint32_t la) {
  uint32_t wa[WORDS];
  pack(a, la, wa);
  return letters_only(wa, in_reach(la) ? la : 0) ? 1 : 0;
}
// degree (m_q), hit_off (m_q + 1) and, where they fit hit_cap, the hits and their distances; returns the need
uint64_t cdr3wmatch_host_match(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q,
                               const uint32_t *q_cls, const uint64_t *q_off, const uint8_t *q_text, const uint8_t *sub, uint32_t gap,
                               uint32_t ntrim, uint32_t ctrim, uint32_t radius, uint32_t *degree, uint64_t *hit_off,
                               uint32_t *hit, uint32_t *hit_dist, uint64_t hit_cap) {
  return flat(match(m_t, t_cls, t_off, t_text, m_q, q_cls, q_off, q_text, weighted(sub, gap, ntrim, ctrim, radius)), degree, hit_off, hit,
              hit_dist, hit_cap);
}
}

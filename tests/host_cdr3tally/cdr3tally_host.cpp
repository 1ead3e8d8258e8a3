// Test-only: the tally's walk on the host (cdr3tally_walk.h) and what the host entry refuses of the radii
// (dcrx_cdr3pair_core.h: refuse_radii), built by g++ for a check against Python on the host.
#include "cdr3tally_walk.h"

using namespace cdr3tally_host;

extern "C" {
// 1 when the host entry refuses these radii
int cdr3tally_host_refuses(const uint32_t *radius, uint64_t m_t) { return refuse_radii(radius, m_t) ? 1 : 0; }
// t_count[m_t], t_weight[m_t], q_degree[m_q]; returns the (block, staged entry) pairs that reached the accumulators
uint64_t cdr3tally_host_tally(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q,
                              const uint32_t *q_cls, const uint64_t *q_off, const uint8_t *q_text, const uint64_t *weight, const uint8_t *sub,
                              uint32_t gap, uint32_t ntrim, uint32_t ctrim, const uint32_t *radius, uint32_t *t_count, uint64_t *t_weight,
                              uint32_t *q_degree) {
  const Totals out = tally(m_t, t_cls, t_off, t_text, m_q, q_cls, q_off, q_text, weight, weighted_per(sub, gap, ntrim, ctrim, radius));
  std::copy(out.t_count.begin(), out.t_count.end(), t_count);
  std::copy(out.t_weight.begin(), out.t_weight.end(), t_weight);
  std::copy(out.q_degree.begin(), out.q_degree.end(), q_degree);
  return out.flushes;
}
}

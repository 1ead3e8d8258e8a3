// Test-only: bin_of of dcrx_cdr3profile_core.h and the host walk with the histogram sink (../host_cdr3walk/cdr3walk_host.h:
// Bipartite with Weighted and Histogram) built by g++, for a check against Python on the host.
#include "../host_cdr3walk/cdr3walk_host.h"

using namespace cdr3walk_host;
using dcrx_cdr3profile::bin_of;

extern "C" {
// bin_of(d, step) for every d in 0 .. n - 1
void cdr3profile_host_bins(uint32_t n, uint32_t step, uint32_t *out) {
  for (uint32_t d = 0; d < n; d++) out[d] = bin_of(d, step);
}
// 1 when the entries refuse (step, bins)
int cdr3profile_host_refuses(uint32_t step, uint32_t bins) { return dcrx_cdr3profile::refuse_ladder(step, bins) ? 1 : 0; }
// profile[m_q * bins]; -1 for a ladder the entries refuse
int cdr3profile_host_profile(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q,
                             const uint32_t *q_cls, const uint64_t *q_off, const uint8_t *q_text, const uint8_t *sub, uint32_t gap,
                             uint32_t ntrim, uint32_t ctrim, uint32_t step, uint32_t bins, uint32_t *profile) {
  if (dcrx_cdr3profile::refuse_ladder(step, bins)) return -1;
  const std::vector<uint32_t> out = cdr3walk_host::profile(m_t, t_cls, t_off, t_text, m_q, q_cls, q_off, q_text, weighted(sub, gap, ntrim, ctrim, 0), step, bins);
  std::copy(out.begin(), out.end(), profile);
  return 0;
}
}

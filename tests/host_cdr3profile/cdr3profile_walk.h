// Test-only: the weighted walk with the histogram sink (cdr3_walk_kernel<false, Bipartite, Weighted, Profile>,
// decombinator_amd/csrc/dcrx_cdr3walk.h) on the host.  The walk is the weighted match's host walk (../host_cdr3wmatch/
// cdr3wmatch_walk.h: the kernel's look-ups, staging and pair test) at radius step * (bins - 1); what is the sink's is done as the
// kernel does it: a block's counters are ONE array of bins * 256 cells, cell b * 256 + lane, zeroed per block, one added per hit
// at bin_of(d, step) (dcrx_cdr3profile_core.h), and read out per valid lane into the row of its rank.  Every access is an at().
#pragma once
#include "../../decombinator_amd/csrc/dcrx_cdr3profile_core.h"
#include "../host_cdr3wmatch/cdr3wmatch_walk.h"

namespace cdr3profile_host {

using namespace cdr3wmatch_host;
using dcrx_cdr3profile::bin_of;

// profile[m_q * bins]; every cell is written.  Returns -1 for a ladder the entries refuse.
inline int profile(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q, const uint32_t *q_cls,
                   const uint64_t *q_off, const uint8_t *q_text, const Cost &C, uint32_t step, uint32_t bins, std::vector<uint32_t> &out) {
  if (dcrx_cdr3profile::refuse_ladder(step, bins)) return -1;
  const uint32_t radius = step * (bins - 1);
  const Side Q = prepare(m_q, q_cls, q_off, q_text), T = prepare(m_t, t_cls, t_off, t_text);
  const auto hits = walk(Q, T, C, radius);      // per query rank, in the order the walk meets them
  out.assign(m_q * bins, 0xA5A5A5A5u);           // (what the read-out does not write stays visible)
  for (uint32_t s0 = 0; s0 < (uint32_t)m_q; s0 += QUERIES) {
    std::vector<uint32_t> hist((size_t)bins * QUERIES, 0u);
    for (uint32_t lane = 0; lane < QUERIES && s0 + lane < m_q; lane++)
      for (const Hit &h : hits.at(Q.idx.at(s0 + lane))) hist.at((size_t)bin_of(h.dist, step) * QUERIES + lane) += 1;
    for (uint32_t lane = 0; lane < QUERIES && s0 + lane < m_q; lane++)
      for (uint32_t b = 0; b < bins; b++) out.at((size_t)Q.idx.at(s0 + lane) * bins + b) = hist.at((size_t)b * QUERIES + lane);
  }
  return 0;
}

}  // namespace cdr3profile_host

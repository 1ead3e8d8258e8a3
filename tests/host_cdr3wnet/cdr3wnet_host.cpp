// Test-only: the host walk of the weighted CDR3 network (cdr3wnet_walk.h) built by g++, for a check against Python on the host.
#include "cdr3wnet_walk.h"

using namespace cdr3wnet_host;

extern "C" {
// degree (m), adj_off (m + 1) and, where they fit adj_cap, the neighbours and their distances; returns the need
uint64_t cdr3wnet_host_network(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text, const uint8_t *sub, uint32_t gap,
                               uint32_t ntrim, uint32_t ctrim, uint32_t radius, uint32_t *degree, uint64_t *adj_off, uint32_t *adj,
                               uint32_t *adj_dist, uint64_t adj_cap) {
  const auto hits = network(m, cls, off, text, Cost{sub, gap, ntrim, ctrim}, radius);
  uint64_t at = 0;
  for (uint64_t i = 0; i < m; i++) {
    degree[i] = (uint32_t)hits[i].size();
    adj_off[i] = at;
    for (const Hit &h : hits[i]) {
      if (at < adj_cap) { adj[at] = h.node; adj_dist[at] = h.dist; }
      at++;
    }
  }
  adj_off[m] = at;
  return at;
}
}

// Test-only: the host walk of the weighted CDR3 network (../host_cdr3walk/cdr3walk_host.h: Within with Weighted) built by g++,
// for a check against Python on the host.
#include "../host_cdr3walk/cdr3walk_host.h"

using namespace cdr3walk_host;

extern "C" {
// degree (m), adj_off (m + 1) and, where they fit adj_cap, the neighbours and their distances; returns the need
uint64_t cdr3wnet_host_network(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text, const uint8_t *sub, uint32_t gap,
                               uint32_t ntrim, uint32_t ctrim, uint32_t radius, uint32_t *degree, uint64_t *adj_off, uint32_t *adj,
                               uint32_t *adj_dist, uint64_t adj_cap) {
  return flat(network(m, cls, off, text, weighted(sub, gap, ntrim, ctrim, radius)), degree, adj_off, adj, adj_dist, adj_cap);
}
}

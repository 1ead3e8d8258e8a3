// Test-only: the rank-sum null's shared code (dcrx_assoc_ranksum_core.h) built by g++, for a check against Python on the host, and
// the primitive's steps (dcrx_assoc_ranksum.hip) written serially around what the kernels' lanes do: a block's slice of the
// features in groups of RS_GROUP and what is left one by one, its tile of relabelings, an LDS-shaped array of exceed counters
// that gets one add per (wave, feature), the tail cells and their flush.  Every buffer has the kernels' size and no more, and is
// indexed with bounds checks.
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_assoc_ranksum_core.h"

using namespace dcrx_assoc_rs;

extern "C" {
uint32_t assoc_ranksum_host_lanes(void) { return LANES; }
uint32_t assoc_ranksum_host_perms_per_lane(void) { return PERMS_PER_LANE; }
uint32_t assoc_ranksum_host_block_perms(void) { return BLOCK_PERMS; }
uint32_t assoc_ranksum_host_slice(void) { return SLICE; }
uint32_t assoc_ranksum_host_group(void) { return RS_GROUP; }
uint32_t assoc_ranksum_host_planes(void) { return PLANES; }
uint32_t assoc_ranksum_host_shift(void) { return SHIFT; }
uint32_t assoc_ranksum_host_max_edges(void) { return MAX_EDGES; }
uint32_t assoc_ranksum_host_weighted_sum(const uint64_t *planes, uint64_t L) { return weighted_sum(planes, L); }
uint32_t assoc_ranksum_host_score_of(uint32_t W, uint32_t N, uint32_t offset, uint32_t scale, uint32_t alternative) {
  return score_of(W, N, offset, scale, alternative);
}
// the cell of t, or 0xFFFFFFFF
uint32_t assoc_ranksum_host_edge_of(const uint32_t *edges, uint32_t E, uint32_t t) { return edge_of(edges, E, t); }
// 0, 1 (invalid) or 2 (unsupported), as both entries judge the scalars
int assoc_ranksum_host_refuse(uint32_t N, uint64_t C, uint32_t alternative, uint64_t F, uint32_t E, uint32_t P) {
  const char *why = nullptr;
  return refuse_scalars(N, C, alternative, F, E, P, &why);
}

// dcrx_assoc_ranksum_device's steps in their plainest serial form, on arrays it trusts as little as the device entry does.
// counts_out (may be null): [0] the LDS adds onto exceed counters (one per (wave, feature) with a hit), [1] the global adds onto
// exceed[], [2] the global adds onto tail[], [3] the pairs that entered the tail branch.  0, or -1 on arguments the entry refuses.
int assoc_ranksum_host_run(uint32_t N, uint64_t C, uint32_t alternative, uint32_t F, const uint64_t *plane, const uint32_t *offset,
                           const uint32_t *scale, const uint32_t *mult, uint32_t E, const uint32_t *edges, uint32_t P, uint64_t seed,
                           uint32_t *obs_score, uint64_t *labels, uint32_t *perm_max, uint32_t *exceed, uint64_t *tail, uint64_t *counts_out) {
  if (assoc_ranksum_host_refuse(N, C, alternative, F, E, P)) return -1;
  const uint32_t n1 = popcount(C);
  const uint64_t bits = sample_bits(N);
  // assoc_ranksum_prepare_kernel
  for (uint32_t j = 0; j < E; j++) tail[j] = 0;
  for (uint32_t f = 0; f < F; f++) {
    uint64_t pl[PLANES];
    for (uint32_t b = 0; b < PLANES; b++) pl[b] = plane[(uint64_t)f * PLANES + b] & bits;
    exceed[f] = 0;
    obs_score[f] = score_of(weighted_sum(pl, C), N, offset[f], scale[f], alternative);
  }
  // assoc_ranksum_labels_kernel
  for (uint32_t p = 0; p < P; p++) {
    std::vector<uint64_t> lds((size_t)MAX_SAMPLES * LABEL_LANES, 0);
    const uint32_t lane = p % LABEL_LANES;
    stage_keys(lds.data() + lane, LABEL_LANES, seed, p, N);
    labels[p] = labels_from_keys(lds.data() + lane, LABEL_LANES, N, n1);
    perm_max[p] = 0;
  }
  // assoc_ranksum_permute_kernel
  uint64_t counts[4] = {0, 0, 0, 0};
  if (F && P)
    for (uint32_t by = 0; by < perm_tiles_for(P); by++)
      for (uint32_t bx = 0; bx < slices_for(F); bx++) {
        std::vector<uint64_t> cell(E, 0);
        std::vector<uint32_t> edge(edges, edges + E), over(SLICE, 0);
        const uint32_t lowest = E ? edges[0] : NO_EDGE, second = E > 1 ? edges[1] : NO_EDGE;
        std::vector<uint64_t> L(BLOCK_PERMS, 0);
        std::vector<uint32_t> best(BLOCK_PERMS, 0), floor_of(BLOCK_PERMS, NO_EDGE);
        std::vector<char> live(BLOCK_PERMS, 0);
        for (uint32_t t = 0; t < LANES; t++)
          for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
            const uint32_t p = perm_of(by, j, t), q = j * LANES + t;
            if (p < P) { L.at(q) = labels[p]; live.at(q) = 1; floor_of.at(q) = lowest; }
          }
        uint32_t f, f_end;
        slice_of(F, bx, &f, &f_end);
        const uint32_t f0 = f;
        auto pairs = [&](uint32_t feature) {
          const uint32_t slot = feature - f0, w = mult[feature], seen = obs_score[feature];
          uint64_t pl[PLANES];
          for (uint32_t b = 0; b < PLANES; b++) pl[b] = plane[(uint64_t)feature * PLANES + b] & bits;
          for (uint32_t wave = 0; wave < LANES / 64; wave++) {
            uint32_t hits = 0, low = 0;
            for (uint32_t j = 0; j < PERMS_PER_LANE; j++)
              for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t q = j * LANES + wave * 64 + lane;
                uint32_t W = 0;
                for (uint32_t b = 0; b < PLANES; b++)
                  if (pl[b]) W += popcount(pl[b] & L.at(q)) << b;      // (a plane of 0 is skipped)
                const uint32_t s = score_of(W, N, offset[feature], scale[feature], alternative);
                if (live.at(q) && s >= seen) hits++;
                if (!w) continue;
                best.at(q) = best.at(q) > s ? best.at(q) : s;
                if (s >= floor_of.at(q)) {
                  counts[3]++;
                  if (s < second) { low++; continue; }      // cell 0: counted for the wave, added once
                  const uint32_t e = edge_of(edge.data(), E, s);
                  if (e < E) cell.at(e) += w;
                }
              }
            if (hits) { over.at(slot) += hits; counts[0]++; }
            if (low) cell.at(0) += (uint64_t)low * w;
          }
        };
        for (; f + RS_GROUP <= f_end; f += RS_GROUP)
          for (uint32_t g = 0; g < RS_GROUP; g++) pairs(f + g);
        for (; f < f_end; f++) pairs(f);
        for (uint32_t t = 0; t < LANES; t++)
          for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
            const uint32_t p = perm_of(by, j, t), q = j * LANES + t;
            if (p < P && best[q] > perm_max[p]) perm_max[p] = best[q];
          }
        for (uint32_t j = 0; j < E; j++)
          if (cell[j]) { tail[j] += cell[j]; counts[2]++; }
        for (uint32_t k = 0; k < f_end - f0; k++)
          if (over.at(k)) { exceed[f0 + k] += over[k]; counts[1]++; }
      }
  if (counts_out)
    for (int i = 0; i < 4; i++) counts_out[i] = counts[i];
  return 0;
}
}

// Test-only: the permutation null's shared code (dcrx_assoc_core.h) built by g++, for a check against Python on the host, and
// the primitive's two steps (dcrx_assoc.hip) written serially around the selection and the scoring step the kernels' lanes make:
// a block's slice of the features, its tile of relabelings, its tail cells and their flush.  Every buffer has the kernels' size
// and no more, and is indexed with bounds checks.
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_assoc_core.h"

using namespace dcrx_assoc;

extern "C" {
uint32_t assoc_host_lanes(void) { return LANES; }
uint32_t assoc_host_label_lanes(void) { return LABEL_LANES; }
uint32_t assoc_host_perms_per_lane(void) { return PERMS_PER_LANE; }
uint32_t assoc_host_block_perms(void) { return BLOCK_PERMS; }
uint32_t assoc_host_slice(void) { return SLICE; }
uint32_t assoc_host_max_samples(void) { return MAX_SAMPLES; }
uint32_t assoc_host_max_permutations(void) { return MAX_PERMUTATIONS; }
// a relabeling as lane `lane` of a block of the label selection finds it: its keys a column of the block's LDS
uint64_t assoc_host_select_labels(uint64_t seed, uint32_t p, uint32_t N, uint32_t n1) {
  std::vector<uint64_t> lds((size_t)MAX_SAMPLES * LABEL_LANES, 0);
  const uint32_t lane = p % LABEL_LANES;
  stage_keys(lds.data() + lane, LABEL_LANES, seed, p, N);
  return labels_from_keys(lds.data() + lane, LABEL_LANES, N, n1);
}
uint32_t assoc_host_score(const uint16_t *rank, uint32_t N, uint64_t M, uint64_t L) { return score(rank, N, M, L); }
int assoc_host_feasible(uint32_t N, uint32_t n1, uint32_t m, uint32_t k) { return feasible(N, n1, m, k) ? 1 : 0; }
// 0, 1 (invalid) or 2 (unsupported), as both entries judge the scalars
int assoc_host_refuse(uint32_t N, uint64_t C, uint64_t F, uint32_t n_ranks, uint32_t tail_ranks, uint32_t P) {
  const char *why = nullptr;
  return refuse_scalars(N, C, F, n_ranks, tail_ranks, P, &why);
}

// dcrx_assoc_permute_device's steps in their plainest serial form.  flushes_out (may be null): the global adds onto tail[] the
// blocks made (one per non-zero tail cell of a block).  0, or -1 on arguments the entry refuses.
int assoc_host_permute(uint32_t N, uint64_t C, uint32_t F, const uint64_t *mask, const uint32_t *mult, const uint16_t *rank_in,
                       uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, uint64_t seed, uint32_t *obs_rank, uint64_t *labels,
                       uint32_t *perm_min, uint64_t *tail, uint64_t *flushes_out) {
  if (assoc_host_refuse(N, C, F, n_ranks, tail_ranks, P)) return -1;
  const uint32_t n1 = popcount(C);
  const uint64_t bits = sample_bits(N);
  const std::vector<uint16_t> rank(rank_in, rank_in + cells(N));
  // assoc_labels_kernel, assoc_prepare_kernel
  for (uint32_t p = 0; p < P; p++) { labels[p] = assoc_host_select_labels(seed, p, N, n1); perm_min[p] = n_ranks; }
  for (uint32_t r = 0; r < tail_ranks; r++) tail[r] = 0;
  for (uint32_t f = 0; f < F; f++) obs_rank[f] = rank.at(row_of(mask[f] & bits, N) + popcount(mask[f] & bits & C));
  // assoc_permute_kernel
  uint64_t flushes = 0;
  if (F && P)
    for (uint32_t by = 0; by < perm_tiles_for(P); by++)
      for (uint32_t bx = 0; bx < slices_for(F); bx++) {
        std::vector<uint16_t> table(rank);
        std::vector<uint64_t> cell(tail_ranks, 0);
        std::vector<uint64_t> L(BLOCK_PERMS, 0);
        std::vector<uint32_t> least(BLOCK_PERMS, 0xFFFFFFFFu), limit(BLOCK_PERMS, 0);
        for (uint32_t t = 0; t < LANES; t++)
          for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
            const uint32_t p = perm_of(by, j, t);
            if (p < P) { L.at(j * LANES + t) = labels[p]; limit.at(j * LANES + t) = tail_ranks; }
          }
        uint32_t f, f_end;
        slice_of(F, bx, &f, &f_end);
        for (; f < f_end; f++) {
          const uint32_t w = mult[f];
          if (!w) continue;
          const uint64_t M = mask[f] & bits;
          const uint32_t row = row_of(M, N);
          for (uint32_t q = 0; q < BLOCK_PERMS; q++) {
            if (row + popcount(M & L[q]) >= table.size()) return -1;
            const uint32_t r = score_at(table.data(), row, M, L[q]);
            least[q] = least[q] < r ? least[q] : r;
            if (r < limit[q]) cell.at(r) += w;
          }
        }
        for (uint32_t t = 0; t < LANES; t++)
          for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
            const uint32_t p = perm_of(by, j, t), q = j * LANES + t;
            if (p < P && least[q] < n_ranks && least[q] < perm_min[p]) perm_min[p] = least[q];
          }
        for (uint32_t r = 0; r < tail_ranks; r++)
          if (cell[r]) { tail[r] += cell[r]; flushes++; }
      }
  if (flushes_out) *flushes_out = flushes;
  return 0;
}
}

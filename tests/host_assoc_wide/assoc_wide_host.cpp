// Test-only: the wide permutation null's shared code (dcrx_assoc_wide_core.h) built by g++, for a check against Python on the
// host, and the primitive's steps (dcrx_assoc_wide.hip) written serially around what the kernels' lanes do: the label selection
// from an LDS-shaped array of keys, a block's slice of the features walked in runs of equal popcount, its tile of relabelings,
// the row, the cells and their flush.  Every buffer has the kernels' size and no more, and is indexed with bounds checks.
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_assoc_wide_core.h"

using namespace dcrx_assoc_wide;

extern "C" {
uint32_t assoc_wide_host_lanes(void) { return LANES; }
uint32_t assoc_wide_host_slice(void) { return SLICE; }
uint32_t assoc_wide_host_max_samples(void) { return MAX_SAMPLES; }
uint32_t assoc_wide_host_max_permutations(void) { return MAX_PERMUTATIONS; }
uint32_t assoc_wide_host_words_for(uint32_t N) { return words_for(N); }
uint32_t assoc_wide_host_perms_per_lane(uint32_t W) { return perms_per_lane(W); }
uint32_t assoc_wide_host_block_perms(uint32_t W) { return block_perms(W); }
uint64_t assoc_wide_host_word_bits(uint32_t N, uint32_t w) { return word_bits(N, w); }

// a relabeling as a block of the label selection finds it: the keys once into the block's array, every lane its samples, a
// wave's 64 answers one word
void assoc_wide_host_select_labels(uint64_t seed, uint32_t p, uint32_t N, uint32_t n1, uint64_t *out) {
  std::vector<uint64_t> lds(MAX_SAMPLES, 0);
  const uint64_t p_seed = perm_seed(seed, p);
  for (uint32_t t = 0; t < LANES; t++)
    for (uint32_t s = t; s < N; s += LANES) stage_key(lds.data(), p_seed, s);
  std::vector<uint64_t> words(MAX_WORDS, 0);
  for (uint32_t t = 0; t < LANES; t++) {
    bool in[LABEL_ITEMS];
    labels_in(lds.data(), N, n1, t, in);
    for (uint32_t i = 0; i < LABEL_ITEMS; i++)
      if (in[i]) words.at((t + i * LANES) >> 6) |= 1ull << (t & 63);
  }
  for (uint32_t w = 0; w < words_for(N); w++) out[w] = words[w];
}
// 0, 1 (invalid) or 2 (unsupported), as both entries judge the scalars, and then the case mask
int assoc_wide_host_refuse(uint32_t N, uint64_t F, uint32_t n_ranks, uint32_t tail_ranks, uint32_t P) {
  const char *why = nullptr;
  return refuse_scalars(N, F, n_ranks, tail_ranks, P, &why);
}
int assoc_wide_host_refuse_cases(uint32_t N, const uint64_t *C, int strict) {
  const char *why = nullptr;
  uint32_t n1 = 0;
  return refuse_cases(N, C, strict != 0, &n1, &why);
}

// dcrx_assoc_permute_wide_device's steps in their plainest serial form.  counts_out (may be null): [0] the global adds onto
// tail[] the blocks made, [1] the runs the blocks walked (a change of m each).  0, or -1 on arguments the entry refuses or an
// index outside a buffer.
int assoc_wide_host_permute(uint32_t N, const uint64_t *C_in, uint32_t F, const uint64_t *mask, const uint32_t *mult, const uint32_t *rank_in,
                            uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, uint64_t seed, uint32_t *obs_rank, uint64_t *labels,
                            uint32_t *perm_min, uint64_t *tail, uint64_t *counts_out) {
  uint32_t n1 = 0;
  const char *why = nullptr;
  if (refuse_scalars(N, F, n_ranks, tail_ranks, P, &why) || refuse_cases(N, C_in, false, &n1, &why)) return -1;
  const uint32_t W = words_for(N), PPL = perms_per_lane(W), BLOCK = block_perms(W);
  std::vector<uint64_t> C(W);
  for (uint32_t w = 0; w < W; w++) C[w] = C_in[w] & word_bits(N, w);
  const std::vector<uint32_t> rank(rank_in, rank_in + cells(N));
  // assoc_wide_labels_kernel, assoc_wide_prepare_kernel
  for (uint32_t p = 0; p < P; p++) { assoc_wide_host_select_labels(seed, p, N, n1, labels + (uint64_t)p * W); perm_min[p] = n_ranks; }
  for (uint32_t r = 0; r < tail_ranks; r++) tail[r] = 0;
  for (uint32_t f = 0; f < F; f++) {
    uint32_t m = 0, k = 0;
    for (uint32_t w = 0; w < W; w++) {
      const uint64_t M = mask[(uint64_t)f * W + w] & word_bits(N, w);
      m += popcount(M);
      k += popcount(M & C[w]);
    }
    obs_rank[f] = rank.at(m * (N + 1) + k);
  }
  // assoc_wide_permute_kernel
  uint64_t flushes = 0, runs = 0;
  if (F && P)
    for (uint32_t by = 0; by < perm_tiles_for(P, W); by++)
      for (uint32_t bx = 0; bx < slices_for(F); bx++) {
        std::vector<uint64_t> cell(MAX_SAMPLES + 1, 0);
        std::vector<uint32_t> row(MAX_SAMPLES + 1, 0);
        std::vector<uint64_t> L((size_t)BLOCK * W, 0);
        std::vector<uint32_t> least(BLOCK, 0xFFFFFFFFu), limit(BLOCK, 0);
        for (uint32_t t = 0; t < LANES; t++)
          for (uint32_t j = 0; j < PPL; j++) {
            const uint32_t p = perm_of(by, j, t, W), q = j * LANES + t;
            if (p < P) {
              for (uint32_t w = 0; w < W; w++) L.at((size_t)q * W + w) = labels[(uint64_t)p * W + w];
              limit.at(q) = tail_ranks;
            }
          }
        uint32_t run_m = NO_RUN;
        auto flush = [&]() {
          for (uint32_t k = 0; k <= N; k++) {
            if (!cell.at(k)) continue;
            const uint32_t r = row.at(k);
            if (flush_cell(cell[k], r, tail_ranks)) { tail[r] += cell[k]; flushes++; }
            cell[k] = 0;
          }
        };
        uint32_t f, f_end;
        slice_of(F, bx, &f, &f_end);
        std::vector<uint64_t> M(W);
        for (; f < f_end; f++) {
          const uint32_t wt = mult[f];
          if (!wt) continue;
          uint32_t m = 0;
          for (uint32_t w = 0; w < W; w++) { M[w] = mask[(uint64_t)f * W + w] & word_bits(N, w); m += popcount(M[w]); }
          if (m != run_m) {
            flush();
            if (m > N) return -1;
            for (uint32_t k = 0; k <= m; k++) row.at(k) = row_cell(rank.data(), N, m, k);
            run_m = m;
            runs++;
          }
          for (uint32_t q = 0; q < BLOCK; q++) {
            uint32_t k = 0;
            for (uint32_t w = 0; w < W; w++)
              if (M[w]) k += popcount(M[w] & L[(size_t)q * W + w]);
            if (k > m) return -1;
            const uint32_t r = row.at(k);
            least[q] = least[q] < r ? least[q] : r;
            if (r < limit[q]) cell.at(k) += wt;
          }
        }
        for (uint32_t t = 0; t < LANES; t++)
          for (uint32_t j = 0; j < PPL; j++) {
            const uint32_t p = perm_of(by, j, t, W), q = j * LANES + t;
            if (p < P && least[q] < n_ranks && least[q] < perm_min[p]) perm_min[p] = least[q];
          }
        flush();
      }
  if (counts_out) { counts_out[0] = flushes; counts_out[1] = runs; }
  return 0;
}
}

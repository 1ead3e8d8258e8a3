// dcrx_assoc_wide.hip — the permutation null of `associate` for cohorts of up to 1024 samples; include/dcrx.h "association, wide"
// holds the contract, dcrx_assoc_wide_core.h the sizes, the selection of a relabeling, a run's row and cells and the refusals.
//
// The primitive (dcrx_assoc_permute_wide_device), on the caller's stream, nothing copied back, no work space:
//   prepare  assoc_wide_prepare_kernel<W>, a lane per index i: tail[i] = 0 (i < tail_ranks), obs_rank[i] (i < F)
//   labels   assoc_wide_labels_kernel, a BLOCK per relabeling p: its N keys once into LDS (8 KB at 1024 samples), then every
//            lane counts, for its up to four samples, the keys smaller than theirs from broadcast reads; a wave's ballot is one
//            word of L_p, and perm_min[p] = n_ranks.  No array of keys in registers.
//   permute  assoc_wide_permute_kernel<W>, one instance per W = 1 .. 16 (the cohort's words, a constant in it), grid (slices of
//            SLICE features, tiles of block_perms(W) relabelings): a lane's perms_per_lane(W) relabelings of W words and their
//            minima in registers; the block walks its slice in runs of equal popcount m with only the row of m (N + 1 ranks of
//            32 bits) and one 64-bit cell per k in LDS.  A feature's words and multiplicity are indexed from blockIdx and the
//            loop counter alone — the same for every lane and every wave, so the barriers around a change of m are uniform —
//            and a word that is 0 is skipped (a scalar branch up to W = 8; from W = 9 on hipcc makes it a select).  Per pair
//            and non-zero word an AND and a popcount; per pair an LDS read, a min, a compare, and only below the lane's tail limit an LDS add whose result is not read.  At the end one global
//            atomic min per (lane, relabeling) that saw a feature, and a global 64-bit add per non-zero cell.
// The table is the caller's: nothing assumes it monotone in k, and the device entry trusts neither it nor the masks (the last
// word of every mask is ANDed with the N-bit remainder, a row is indexed with k <= m <= N alone, a rank adds to the tail only
// below tail_ranks).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_assoc_wide_core.h"
#include "dcrx_group.h"

using dcrx::set_err;
using namespace dcrx_assoc_wide;
using dcrx_group::Pool;
using dcrx_group::to_device;
using dcrx_group::to_host;

namespace {

struct Args {
  const uint64_t *mask;
  const uint32_t *mult;
  const uint32_t *rank;
  uint32_t *obs_rank;
  uint64_t *labels;
  uint32_t *perm_min;
  unsigned long long *tail;
  uint64_t seed;
  uint32_t N, W, n1, F, P, n_ranks, tail_ranks;
  uint64_t C[MAX_WORDS];      // the case mask, cut to N bits; 0 from word W on
};

// a block per relabeling: the N keys once into LDS, N broadcast reads a lane, a ballot a word
__global__ __launch_bounds__(LANES) void assoc_wide_labels_kernel(Args A) {
  __shared__ uint64_t keys[MAX_SAMPLES];
  const uint32_t p = blockIdx.x, t = threadIdx.x, N = A.N;
  const uint64_t p_seed = perm_seed(A.seed, p);
  for (uint32_t s = t; s < N; s += LANES) stage_key(keys, p_seed, s);
  __syncthreads();
  bool in[LABEL_ITEMS];
  labels_in(keys, N, A.n1, t, in);
#pragma unroll
  for (uint32_t i = 0; i < LABEL_ITEMS; i++) {
    const uint64_t word = __ballot(in[i]);
    const uint32_t w = (t + i * LANES) >> 6;      // (one value for the wave)
    if ((t & 63) == 0 && w < A.W) A.labels[(uint64_t)p * A.W + w] = word;
  }
  if (t == 0) A.perm_min[p] = A.n_ranks;
}

// a lane per index: tail[i] = 0 and obs_rank[i]
template <uint32_t W>
__global__ __launch_bounds__(LANES) void assoc_wide_prepare_kernel(Args A) {
  const uint32_t i = blockIdx.x * LANES + threadIdx.x;
  if (i < A.tail_ranks) A.tail[i] = 0;
  if (i >= A.F) return;
  uint32_t m = 0, k = 0;
#pragma unroll
  for (uint32_t w = 0; w < W; w++) {
    const uint64_t M = A.mask[(uint64_t)i * W + w] & word_bits(A.N, w);
    m += popcount(M);
    k += popcount(M & A.C[w]);
  }
  A.obs_rank[i] = row_cell(A.rank, A.N, m, k);
}

// (mask and mult come as parameters of their own, read-only and unaliased: their loads may then stay off the vector lanes)
template <uint32_t W>
__global__ __launch_bounds__(LANES) void assoc_wide_permute_kernel(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ mult, Args A) {
  constexpr uint32_t PPL = perms_per_lane(W), GROUP = group(W);
  __shared__ unsigned long long cell[MAX_SAMPLES + 1];      // per k of the run's row: what the block's pairs at (m, k) weigh
  __shared__ uint32_t row[MAX_SAMPLES + 1];                 // rank[m][0 .. m] of the run
  const uint32_t t = threadIdx.x, N = A.N, tail_ranks = A.tail_ranks;
  uint64_t L[PPL][W];
  uint32_t least[PPL], limit[PPL];      // limit: tail_ranks, or 0 where the lane has no relabeling
#pragma unroll
  for (uint32_t j = 0; j < PPL; j++) {
    const uint32_t p = perm_of(blockIdx.y, j, t, W);
    const bool valid = p < A.P;
#pragma unroll
    for (uint32_t w = 0; w < W; w++) L[j][w] = valid ? A.labels[(uint64_t)p * W + w] : 0;
    least[j] = 0xFFFFFFFFu;
    limit[j] = valid ? tail_ranks : 0;
  }
  for (uint32_t k = t; k <= N; k += LANES) cell[k] = 0;      // (lane t owns the cells and the row at k = t + i LANES throughout)
  uint32_t run_m = NO_RUN;
  // the cells a lane owns onto the tail: after a barrier, so that every add of the run has landed
  auto flush = [&]() {
    for (uint32_t k = t; k <= N; k += LANES) {
      const unsigned long long c = cell[k];
      if (!c) continue;      // (a cell is non-zero only at k <= run_m, where the row is staged)
      const uint32_t r = row[k];
      if (flush_cell(c, r, tail_ranks)) atomicAdd(&A.tail[r], c);
      cell[k] = 0;
    }
  };
  uint32_t f, f_end;
  slice_of(A.F, blockIdx.x, &f, &f_end);
  // (f comes from blockIdx and the loop counter: one value for the block.  GROUP features' words are asked for together, so the
  // wave waits for memory once a group; what is left of the slice goes one by one)
  auto pairs = [&](const uint64_t (&M)[W], uint32_t wt) {
    if (!wt) return;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; w++) m += popcount(M[w]);
    if (m != run_m) {      // the same for every wave of the block, as the words are: the barriers are uniform
      __syncthreads();
      flush();
      for (uint32_t k = t; k <= m; k += LANES) row[k] = row_cell(A.rank, N, m, k);
      run_m = m;
      __syncthreads();
    }
    uint32_t k[PPL];
#pragma unroll
    for (uint32_t j = 0; j < PPL; j++) k[j] = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; w++)
      if (M[w]) {
#pragma unroll
        for (uint32_t j = 0; j < PPL; j++) k[j] += popcount(M[w] & L[j][w]);
      }
#pragma unroll
    for (uint32_t j = 0; j < PPL; j++) {      // k[j] <= m: the popcount of a subset
      const uint32_t r = row[k[j]];
      least[j] = least[j] < r ? least[j] : r;
      if (r < limit[j]) atomicAdd(&cell[k[j]], (unsigned long long)wt);
    }
  };
  const uint64_t last_bits = word_bits(N, W - 1);      // (the words before the last are whole)
  auto words_of = [&](uint32_t feature, uint64_t (&M)[W]) {
#pragma unroll
    for (uint32_t w = 0; w < W; w++) M[w] = mask[(uint64_t)feature * W + w] & (w == W - 1 ? last_bits : ~0ull);
  };
  for (; f + GROUP <= f_end; f += GROUP) {
    uint64_t M[GROUP][W];
    uint32_t wt[GROUP];
#pragma unroll
    for (uint32_t g = 0; g < GROUP; g++) { words_of(f + g, M[g]); wt[g] = mult[f + g]; }
#pragma unroll
    for (uint32_t g = 0; g < GROUP; g++) pairs(M[g], wt[g]);
  }
  if constexpr (GROUP > 1)
    for (; f < f_end; f++) {
      uint64_t M[W];
      words_of(f, M);
      pairs(M, mult[f]);
    }
#pragma unroll
  for (uint32_t j = 0; j < PPL; j++) {
    const uint32_t p = perm_of(blockIdx.y, j, t, W);
    if (p < A.P && least[j] < A.n_ranks) atomicMin(&A.perm_min[p], least[j]);
  }
  __syncthreads();
  flush();
}

static_assert(LANES == (uint32_t)dcrx_group::BLOCK, "grid_for() sizes the prepare kernel's grid: a lane per index in blocks of LANES");

template <uint32_t W>
int launch(const Args &A, hipStream_t s) {
  const uint64_t most = std::max<uint64_t>(A.F, A.tail_ranks);
  if (most) {
    assoc_wide_prepare_kernel<W><<<dcrx_group::grid_for(most), LANES, 0, s>>>(A);
    HIP_TRY(hipGetLastError());
  }
  if (A.P) {
    assoc_wide_labels_kernel<<<A.P, LANES, 0, s>>>(A);
    HIP_TRY(hipGetLastError());
  }
  if (A.F && A.P) {
    assoc_wide_permute_kernel<W><<<dim3(slices_for(A.F), perm_tiles_for(A.P, W)), LANES, 0, s>>>(A.mask, A.mult, A);
    HIP_TRY(hipGetLastError());
  }
  return DCRX_OK;
}

// an instance per number of words: W is a constant in every index and every loop
template <uint32_t W = 1>
int run_permute(const Args &A, hipStream_t s) {
  if (A.W == W) return launch<W>(A, s);
  if constexpr (W < MAX_WORDS) return run_permute<W + 1>(A, s);
  return set_err(DCRX_E_INVALID, "dcrx_assoc_permute_wide_device: no instance for this number of words");
}

int refused(const char *who, int kind, const char *why) {
  static thread_local char msg[200];
  std::snprintf(msg, sizeof msg, "%s: %s", who, why);
  return set_err(kind == 1 ? DCRX_E_INVALID : DCRX_E_UNSUPPORTED, msg);
}

bool null_array(const void *cases, uint64_t F, const void *mask, const void *mult, const void *rank, uint32_t tail_ranks, uint32_t P,
                const void *obs_rank, const void *labels, const void *perm_min, const void *tail) {
  return !cases || !rank || (F && (!mask || !mult || !obs_rank)) || (P && (!labels || !perm_min)) || (tail_ranks && !tail);
}

Args args_of(uint32_t N, const uint64_t *C, uint32_t n1, uint64_t F, const uint64_t *mask, const uint32_t *mult, const uint32_t *rank,
             uint32_t n_ranks, uint32_t tail_ranks, uint32_t P, uint64_t seed, uint32_t *obs_rank, uint64_t *labels, uint32_t *perm_min,
             uint64_t *tail) {
  Args A{};
  A.mask = mask; A.mult = mult; A.rank = rank; A.obs_rank = obs_rank; A.labels = labels; A.perm_min = perm_min;
  A.tail = reinterpret_cast<unsigned long long *>(tail);
  A.seed = seed; A.N = N; A.W = words_for(N); A.n1 = n1; A.F = (uint32_t)F; A.P = P; A.n_ranks = n_ranks; A.tail_ranks = tail_ranks;
  for (uint32_t w = 0; w < A.W; w++) A.C[w] = C[w] & word_bits(N, w);
  return A;
}

// L_p on the host, for the calls that touch no device: the n1 smallest of the N keys
void host_labels(uint64_t seed, uint32_t p, uint32_t N, uint32_t n1, uint64_t *out) {
  std::vector<std::pair<uint64_t, uint32_t>> keys(N);
  const uint64_t p_seed = perm_seed(seed, p);
  for (uint32_t s = 0; s < N; s++) keys[s] = {dcrx_rar::key_of(p_seed, s), s};
  std::nth_element(keys.begin(), keys.begin() + n1, keys.end());
  for (uint32_t w = 0; w < words_for(N); w++) out[w] = 0;
  for (uint32_t i = 0; i < n1; i++) out[keys[i].second >> 6] |= 1ull << (keys[i].second & 63);
}

}  // namespace

extern "C" {

int dcrx_assoc_permute_wide_device(uint32_t n_samples, const uint64_t *case_mask, uint64_t n_features, const uint64_t *d_mask,
                                   const uint32_t *d_mult, const uint32_t *d_rank, uint32_t n_ranks, uint32_t tail_ranks,
                                   uint32_t permutations, uint64_t seed, uint32_t *d_obs_rank, uint64_t *d_labels, uint32_t *d_perm_min,
                                   uint64_t *d_tail, void *hip_stream) {
  const char *who = "dcrx_assoc_permute_wide_device", *why = nullptr;
  int kind;
  uint32_t n1 = 0;
  if ((kind = refuse_scalars(n_samples, n_features, n_ranks, tail_ranks, permutations, &why))) return refused(who, kind, why);
  if (null_array(case_mask, n_features, d_mask, d_mult, d_rank, tail_ranks, permutations, d_obs_rank, d_labels, d_perm_min, d_tail))
    return set_err(DCRX_E_INVALID, "dcrx_assoc_permute_wide_device: null argument");
  if ((kind = refuse_cases(n_samples, case_mask, false, &n1, &why))) return refused(who, kind, why);
  return run_permute<>(args_of(n_samples, case_mask, n1, n_features, d_mask, d_mult, d_rank, n_ranks, tail_ranks, permutations, seed,
                             d_obs_rank, d_labels, d_perm_min, d_tail),
                     (hipStream_t)hip_stream);
}

int dcrx_assoc_permute_wide(uint32_t n_samples, const uint64_t *case_mask, uint64_t n_features, const uint64_t *mask, const uint32_t *mult,
                            const uint32_t *rank, uint32_t n_ranks, uint32_t tail_ranks, uint32_t permutations, uint64_t seed,
                            uint32_t *obs_rank_out, uint64_t *labels_out, uint32_t *perm_min_out, uint64_t *tail_out,
                            dcrx_assoc_stats_t *stats_out) {
  const char *who = "dcrx_assoc_permute_wide", *why = nullptr;
  int kind, rc;
  const uint32_t N = n_samples, P = permutations;
  const uint64_t F = n_features;
  uint32_t n1 = 0;
  if ((kind = refuse_scalars(N, F, n_ranks, tail_ranks, P, &why))) return refused(who, kind, why);
  if (null_array(case_mask, F, mask, mult, rank, tail_ranks, P, obs_rank_out, labels_out, perm_min_out, tail_out))
    return set_err(DCRX_E_INVALID, "dcrx_assoc_permute_wide: null argument");
  if ((kind = refuse_cases(N, case_mask, true, &n1, &why))) return refused(who, kind, why);
  const uint32_t W = words_for(N);
  for (uint32_t m = 0; m <= N; m++)
    for (uint32_t k = 0; k <= m; k++)
      if (feasible(N, n1, m, k) && rank[m * (N + 1) + k] >= n_ranks)
        return set_err(DCRX_E_INVALID, "dcrx_assoc_permute_wide: a feasible cell of the rank table is at or above n_ranks");
  dcrx_assoc_stats_t st{};
  st.features = F;
  st.permutations = P;
  st.min_perm_rank = n_ranks;
  for (uint64_t f = 0; f < F; f++)      // (a pass of its own: every mask is judged before any multiplicity is summed)
    if (mask[f * W + W - 1] & ~word_bits(N, W - 1))
      return set_err(DCRX_E_INVALID, "dcrx_assoc_permute_wide: a presence mask has a bit at or above the number of samples");
  for (uint64_t f = 0; f < F; f++) {
    st.features_weighted += mult[f] ? 1 : 0;
    if ((st.weight += mult[f]) >= MAX_WEIGHT) return set_err(DCRX_E_UNSUPPORTED, "dcrx_assoc_permute_wide: the multiplicities sum to 2^32 or more");
  }
  if (!F || !P) {      // answered here: no device is touched
    for (uint64_t f = 0; f < F; f++) {
      uint32_t m = 0, k = 0;
      for (uint32_t w = 0; w < W; w++) { m += popcount(mask[f * W + w]); k += popcount(mask[f * W + w] & case_mask[w]); }
      obs_rank_out[f] = row_cell(rank, N, m, k);
    }
    for (uint32_t p = 0; p < P; p++) {
      host_labels(seed, p, N, n1, labels_out + (uint64_t)p * W);
      perm_min_out[p] = n_ranks;
    }
    for (uint32_t r = 0; r < tail_ranks; r++) tail_out[r] = 0;
    if (stats_out) *stats_out = st;
    return DCRX_OK;
  }
  Pool pool;
  uint64_t *d_mask, *d_labels, *d_tail;
  uint32_t *d_mult, *d_obs, *d_min, *d_rank;
  for (int pass = 0; pass < 2; pass++) {
    pool.get(&d_mask, F * W); pool.get(&d_mult, F); pool.get(&d_rank, cells(N)); pool.get(&d_obs, F); pool.get(&d_labels, (uint64_t)P * W);
    pool.get(&d_min, P); pool.get(&d_tail, tail_ranks);
    if (pass == 0 && (rc = pool.allocate())) return rc;
  }
  if ((rc = to_device(d_mask, mask, F * W)) || (rc = to_device(d_mult, mult, F)) || (rc = to_device(d_rank, rank, cells(N))) ||
      (rc = run_permute<>(args_of(N, case_mask, n1, F, d_mask, d_mult, d_rank, n_ranks, tail_ranks, P, seed, d_obs, d_labels, d_min, d_tail), nullptr)) ||
      (rc = to_host(obs_rank_out, d_obs, F)) || (rc = to_host(labels_out, d_labels, (uint64_t)P * W)) || (rc = to_host(perm_min_out, d_min, P)) ||
      (rc = to_host(tail_out, d_tail, tail_ranks)))
    return rc;
  for (uint32_t r = 0; r < tail_ranks; r++) st.tail_total += tail_out[r];
  for (uint32_t p = 0; p < P; p++) st.min_perm_rank = std::min<uint64_t>(st.min_perm_rank, perm_min_out[p]);
  if (stats_out) *stats_out = st;
  return DCRX_OK;
}

}  // extern "C"

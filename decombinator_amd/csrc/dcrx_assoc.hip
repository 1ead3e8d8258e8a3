// dcrx_assoc.hip — the permutation null of `associate`; include/dcrx.h "association" holds the contract, dcrx_assoc_core.h the
// sizes, the selection of a relabeling, the scoring step and the refusals.
//
// The primitive (dcrx_assoc_permute_device), on the caller's stream, nothing copied back, no work space:
//   prepare  assoc_prepare_kernel, a lane per index i: tail[i] = 0 (i < tail_ranks), obs_rank[i] (i < F)
//   labels   assoc_labels_kernel, a lane per relabeling p in blocks of LABEL_LANES: its N keys once into its own column of
//            LDS, then N^2 compares from there; labels[p] = L_p and perm_min[p] = n_ranks.  No array of keys in registers.
//   permute  assoc_permute_kernel, grid (slices of SLICE features, tiles of BLOCK_PERMS relabelings): the rank table and the
//            block's tail cells in dynamic LDS (tail cells first: 64 bits wide, 16-byte aligned base), a lane's PERMS_PER_LANE
//            relabelings and minima in registers.  A feature's mask, row and multiplicity are indexed from blockIdx and the
//            loop counter alone: the same for every lane.  Per pair an AND, a popcount, an LDS read, a min, a compare; only
//            below the lane's tail limit an LDS add whose result is not read.  At the end one global atomic min per (lane,
//            relabeling) that saw a feature, and one global 64-bit atomic add per non-zero tail cell.
// The table is the caller's: nothing assumes it monotone in k, and the device entry trusts neither it nor the masks (masks are
// ANDed with the N-bit mask, a rank adds to the tail only below tail_ranks).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_assoc_core.h"
#include "dcrx_group.h"

using dcrx::set_err;
using namespace dcrx_assoc;
using dcrx_group::Pool;
using dcrx_group::to_device;
using dcrx_group::to_host;

namespace {

struct Args {
  const uint64_t *mask;
  const uint32_t *mult;
  const uint16_t *rank;
  uint32_t *obs_rank;
  uint64_t *labels;
  uint32_t *perm_min;
  unsigned long long *tail;
  uint64_t C, seed;
  uint32_t N, n1, F, P, n_ranks, tail_ranks;
};

// a lane per relabeling: its N keys once into its column of LDS (32 KB a block at 64 samples), then the N^2 compares from there
__global__ __launch_bounds__(LABEL_LANES) void assoc_labels_kernel(Args A) {
  __shared__ uint64_t keys[MAX_SAMPLES * LABEL_LANES];
  const uint32_t p = blockIdx.x * LABEL_LANES + threadIdx.x;
  if (p >= A.P) return;      // (no barrier below: a lane reads its own column alone)
  stage_keys(keys + threadIdx.x, LABEL_LANES, A.seed, p, A.N);
  A.labels[p] = labels_from_keys(keys + threadIdx.x, LABEL_LANES, A.N, A.n1);
  A.perm_min[p] = A.n_ranks;
}

// a lane per index: tail[i] = 0 and obs_rank[i]
__global__ __launch_bounds__(LANES) void assoc_prepare_kernel(Args A) {
  const uint32_t i = blockIdx.x * LANES + threadIdx.x;
  if (i < A.tail_ranks) A.tail[i] = 0;
  if (i < A.F) A.obs_rank[i] = score(A.rank, A.N, A.mask[i] & sample_bits(A.N), A.C);
}

// (mask and mult come as parameters of their own, read-only and unaliased: their loads may then stay off the vector lanes)
__global__ __launch_bounds__(LANES) void assoc_permute_kernel(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ mult, Args A) {
  extern __shared__ unsigned long long lds[];      // tail_ranks cells of 64 bits, then (N + 1)^2 ranks of 16
  unsigned long long *cell = lds;
  uint16_t *table = reinterpret_cast<uint16_t *>(lds + A.tail_ranks);
  const uint32_t t = threadIdx.x, N = A.N, n_cells = cells(N), tail_ranks = A.tail_ranks;
  const uint64_t bits = sample_bits(N);
  for (uint32_t k = t; k < n_cells; k += LANES) table[k] = A.rank[k];
  for (uint32_t k = t; k < tail_ranks; k += LANES) cell[k] = 0;
  uint64_t L[PERMS_PER_LANE];
  uint32_t least[PERMS_PER_LANE], limit[PERMS_PER_LANE];      // limit: tail_ranks, or 0 where the lane has no relabeling
#pragma unroll
  for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
    const uint32_t p = perm_of(blockIdx.y, j, t);
    const bool valid = p < A.P;
    L[j] = valid ? A.labels[p] : 0;
    least[j] = 0xFFFFFFFFu;
    limit[j] = valid ? tail_ranks : 0;
  }
  __syncthreads();
  uint32_t f, f_end;
  slice_of(A.F, blockIdx.x, &f, &f_end);
  // (f comes from blockIdx and the loop counter: one value for the wave.  GROUP features' words are asked for together, so the
  // wave waits for memory once a group and not twice a feature; what is left of the slice goes one by one)
  auto pairs = [&](uint64_t M_raw, uint32_t w) {
    if (!w) return;
    const uint64_t M = M_raw & bits;
    const uint32_t row = row_of(M, N);
#pragma unroll
    for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
      const uint32_t r = score_at(table, row, M, L[j]);
      least[j] = least[j] < r ? least[j] : r;
      if (r < limit[j]) atomicAdd(&cell[r], (unsigned long long)w);
    }
  };
  for (; f + GROUP <= f_end; f += GROUP) {
    uint64_t M[GROUP];
    uint32_t w[GROUP];
#pragma unroll
    for (uint32_t g = 0; g < GROUP; g++) { M[g] = mask[f + g]; w[g] = mult[f + g]; }
#pragma unroll
    for (uint32_t g = 0; g < GROUP; g++) pairs(M[g], w[g]);
  }
  for (; f < f_end; f++) pairs(mask[f], mult[f]);
#pragma unroll
  for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
    const uint32_t p = perm_of(blockIdx.y, j, t);
    if (p < A.P && least[j] < A.n_ranks) atomicMin(&A.perm_min[p], least[j]);
  }
  __syncthreads();
  for (uint32_t k = t; k < tail_ranks; k += LANES) {
    const unsigned long long c = cell[k];
    if (c) atomicAdd(&A.tail[k], c);
  }
}

size_t permute_lds_bytes(uint32_t N, uint32_t tail_ranks) { return (size_t)tail_ranks * 8 + (size_t)cells(N) * 2; }

int run_permute(const Args &A, hipStream_t s) {
  const uint64_t most = std::max<uint64_t>(A.F, A.tail_ranks);
  if (most) {
    assoc_prepare_kernel<<<dcrx_group::grid_for(most), LANES, 0, s>>>(A);
    HIP_TRY(hipGetLastError());
  }
  if (A.P) {
    assoc_labels_kernel<<<(A.P + LABEL_LANES - 1) / LABEL_LANES, LABEL_LANES, 0, s>>>(A);
    HIP_TRY(hipGetLastError());
  }
  if (A.F && A.P) {
    assoc_permute_kernel<<<dim3(slices_for(A.F), perm_tiles_for(A.P)), LANES, permute_lds_bytes(A.N, A.tail_ranks), s>>>(A.mask, A.mult, A);
    HIP_TRY(hipGetLastError());
  }
  return DCRX_OK;
}

int refuse(const char *who, uint32_t N, uint64_t C, uint64_t F, uint32_t n_ranks, uint32_t tail_ranks, uint32_t P) {
  static thread_local char msg[200];
  const char *why = nullptr;
  const int kind = refuse_scalars(N, C, F, n_ranks, tail_ranks, P, &why);
  if (!kind) return DCRX_OK;
  std::snprintf(msg, sizeof msg, "%s: %s", who, why);
  return set_err(kind == 1 ? DCRX_E_INVALID : DCRX_E_UNSUPPORTED, msg);
}

bool null_array(uint64_t F, const void *mask, const void *mult, const void *rank, uint32_t tail_ranks, uint32_t P, const void *obs_rank,
                const void *labels, const void *perm_min, const void *tail) {
  return !rank || (F && (!mask || !mult || !obs_rank)) || (P && (!labels || !perm_min)) || (tail_ranks && !tail);
}

Args args_of(uint32_t N, uint64_t C, uint64_t F, const uint64_t *mask, const uint32_t *mult, const uint16_t *rank, uint32_t n_ranks,
             uint32_t tail_ranks, uint32_t P, uint64_t seed, uint32_t *obs_rank, uint64_t *labels, uint32_t *perm_min, uint64_t *tail) {
  Args A{};
  A.mask = mask; A.mult = mult; A.rank = rank; A.obs_rank = obs_rank; A.labels = labels; A.perm_min = perm_min;
  A.tail = reinterpret_cast<unsigned long long *>(tail);
  A.C = C; A.seed = seed; A.N = N; A.n1 = popcount(C); A.F = (uint32_t)F; A.P = P; A.n_ranks = n_ranks; A.tail_ranks = tail_ranks;
  return A;
}

}  // namespace

extern "C" {

int dcrx_assoc_permute_device(uint32_t n_samples, uint64_t case_mask, uint64_t n_features, const uint64_t *d_mask, const uint32_t *d_mult,
                              const uint16_t *d_rank, uint32_t n_ranks, uint32_t tail_ranks, uint32_t permutations, uint64_t seed,
                              uint32_t *d_obs_rank, uint64_t *d_labels, uint32_t *d_perm_min, uint64_t *d_tail, void *hip_stream) {
  int rc;
  if ((rc = refuse("dcrx_assoc_permute_device", n_samples, case_mask, n_features, n_ranks, tail_ranks, permutations))) return rc;
  if (null_array(n_features, d_mask, d_mult, d_rank, tail_ranks, permutations, d_obs_rank, d_labels, d_perm_min, d_tail))
    return set_err(DCRX_E_INVALID, "dcrx_assoc_permute_device: null argument");
  return run_permute(args_of(n_samples, case_mask, n_features, d_mask, d_mult, d_rank, n_ranks, tail_ranks, permutations, seed, d_obs_rank,
                             d_labels, d_perm_min, d_tail),
                     (hipStream_t)hip_stream);
}

int dcrx_assoc_permute(uint32_t n_samples, uint64_t case_mask, uint64_t n_features, const uint64_t *mask, const uint32_t *mult,
                       const uint16_t *rank, uint32_t n_ranks, uint32_t tail_ranks, uint32_t permutations, uint64_t seed,
                       uint32_t *obs_rank_out, uint64_t *labels_out, uint32_t *perm_min_out, uint64_t *tail_out,
                       dcrx_assoc_stats_t *stats_out) {
  int rc;
  const uint32_t N = n_samples, P = permutations;
  const uint64_t F = n_features;
  if ((rc = refuse("dcrx_assoc_permute", N, case_mask, F, n_ranks, tail_ranks, P))) return rc;
  if (null_array(F, mask, mult, rank, tail_ranks, P, obs_rank_out, labels_out, perm_min_out, tail_out))
    return set_err(DCRX_E_INVALID, "dcrx_assoc_permute: null argument");
  const uint32_t n1 = popcount(case_mask);
  for (uint32_t m = 0; m <= N; m++)
    for (uint32_t k = 0; k <= m; k++)
      if (feasible(N, n1, m, k) && rank[m * (N + 1) + k] >= n_ranks)
        return set_err(DCRX_E_INVALID, "dcrx_assoc_permute: a feasible cell of the rank table is at or above n_ranks");
  dcrx_assoc_stats_t st{};
  st.features = F;
  st.permutations = P;
  st.min_perm_rank = n_ranks;
  for (uint64_t f = 0; f < F; f++) {
    if (mask[f] & ~sample_bits(N)) return set_err(DCRX_E_INVALID, "dcrx_assoc_permute: a presence mask has a bit at or above the number of samples");
    st.features_weighted += mult[f] ? 1 : 0;
    if ((st.weight += mult[f]) >= MAX_WEIGHT) return set_err(DCRX_E_UNSUPPORTED, "dcrx_assoc_permute: the multiplicities sum to 2^32 or more");
  }
  if (!F || !P) {      // answered here: no device is touched
    for (uint64_t f = 0; f < F; f++) obs_rank_out[f] = score(rank, N, mask[f], case_mask);
    uint64_t keys[MAX_SAMPLES];
    for (uint32_t p = 0; p < P; p++) {
      stage_keys(keys, 1, seed, p, N);
      labels_out[p] = labels_from_keys(keys, 1, N, n1);
      perm_min_out[p] = n_ranks;
    }
    for (uint32_t r = 0; r < tail_ranks; r++) tail_out[r] = 0;
    if (stats_out) *stats_out = st;
    return DCRX_OK;
  }
  Pool pool;
  uint64_t *d_mask, *d_labels, *d_tail;
  uint32_t *d_mult, *d_obs, *d_min;
  uint16_t *d_rank;
  for (int pass = 0; pass < 2; pass++) {
    pool.get(&d_mask, F); pool.get(&d_mult, F); pool.get(&d_rank, cells(N)); pool.get(&d_obs, F); pool.get(&d_labels, P);
    pool.get(&d_min, P); pool.get(&d_tail, tail_ranks);
    if (pass == 0 && (rc = pool.allocate())) return rc;
  }
  if ((rc = to_device(d_mask, mask, F)) || (rc = to_device(d_mult, mult, F)) || (rc = to_device(d_rank, rank, cells(N))) ||
      (rc = run_permute(args_of(N, case_mask, F, d_mask, d_mult, d_rank, n_ranks, tail_ranks, P, seed, d_obs, d_labels, d_min, d_tail), nullptr)) ||
      (rc = to_host(obs_rank_out, d_obs, F)) || (rc = to_host(labels_out, d_labels, P)) || (rc = to_host(perm_min_out, d_min, P)) ||
      (rc = to_host(tail_out, d_tail, tail_ranks)))
    return rc;
  for (uint32_t r = 0; r < tail_ranks; r++) st.tail_total += tail_out[r];
  for (uint32_t p = 0; p < P; p++) st.min_perm_rank = std::min<uint64_t>(st.min_perm_rank, perm_min_out[p]);
  if (stats_out) *stats_out = st;
  return DCRX_OK;
}

}  // extern "C"

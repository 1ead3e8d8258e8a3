// dcrx_assoc_ranksum.hip — the rank-sum null of `associate --test rank-sum`; include/dcrx.h "association, rank-sum" holds the
// contract, dcrx_assoc_ranksum_core.h the weighted popcount, the score, the search of the edges and the refusals, and
// dcrx_assoc_core.h the sizes of the walk and the selection of a relabeling, which is the presence null's.
//
// The primitive (dcrx_assoc_ranksum_device), on the caller's stream, nothing copied back, no work space:
//   prepare  assoc_ranksum_prepare_kernel, a lane per index i: tail[i] = 0 (i < E), exceed[i] = 0 and obs_score[i] (i < F)
//   labels   assoc_ranksum_labels_kernel: stage_keys and labels_from_keys as assoc_labels_kernel calls them; perm_max[p] = 0
//   permute  assoc_ranksum_permute_kernel<alternative>, grid (slices of SLICE features, tiles of BLOCK_PERMS relabelings): the
//            block's tail cells (64 bits, first), the edges and the slice's exceed counters in static LDS, 16 KB; a lane's
//            PERMS_PER_LANE relabelings, rank sums and maxima in registers.  A feature's eleven words are indexed from blockIdx
//            and the loop counter alone, through read-only unaliased parameters: the same for every lane, asked for RS_GROUP
//            features at a time.  A plane that is 0 is branched over by the whole wave.  exceed is counted by ballot, one LDS add
//            per (wave, feature); the tail is entered only at or above edges[0], and below edges[1] — cell 0, where most pairs
//            of a null fall — it is counted by ballot too, one 64-bit LDS add per (wave, feature).  At the end one global atomic max per (lane,
//            relabeling) above 0, one global 64-bit add per non-zero tail cell and one global add per non-zero exceed counter.
// The device entry trusts no array: planes are ANDed with the N-bit mask, u is clamped, the edges are searched inside 0 .. E - 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "../../include/dcrx.h"
#include "dcrx_assoc_ranksum_core.h"
#include "dcrx_group.h"

using dcrx::set_err;
using namespace dcrx_assoc_rs;
using dcrx_group::Pool;
using dcrx_group::to_device;
using dcrx_group::to_host;

namespace {

struct Args {
  const uint64_t *plane;
  const uint32_t *offset, *scale, *mult, *edges;
  uint32_t *obs_score;
  uint64_t *labels;
  uint32_t *perm_max, *exceed;
  unsigned long long *tail;
  uint64_t C, seed;
  uint32_t N, n1, alternative, F, E, P;
};

// a lane per relabeling: "association"'s selection, its keys a column of LDS
__global__ __launch_bounds__(LABEL_LANES) void assoc_ranksum_labels_kernel(Args A) {
  __shared__ uint64_t keys[MAX_SAMPLES * LABEL_LANES];
  const uint32_t p = blockIdx.x * LABEL_LANES + threadIdx.x;
  if (p >= A.P) return;      // (no barrier below: a lane reads its own column alone)
  stage_keys(keys + threadIdx.x, LABEL_LANES, A.seed, p, A.N);
  A.labels[p] = labels_from_keys(keys + threadIdx.x, LABEL_LANES, A.N, A.n1);
  A.perm_max[p] = 0;
}

// a lane per index: tail[i] = 0, exceed[i] = 0 and obs_score[i]
__global__ __launch_bounds__(LANES) void assoc_ranksum_prepare_kernel(Args A) {
  const uint32_t i = blockIdx.x * LANES + threadIdx.x;
  if (i < A.E) A.tail[i] = 0;
  if (i < A.F) {
    const uint64_t bits = sample_bits(A.N);
    uint64_t pl[PLANES];
#pragma unroll
    for (uint32_t b = 0; b < PLANES; b++) pl[b] = A.plane[(uint64_t)i * PLANES + b] & bits;
    A.exceed[i] = 0;
    A.obs_score[i] = score_of(weighted_sum(pl, A.C), A.N, A.offset[i], A.scale[i], A.alternative);
  }
}

// (the per-feature arrays come as parameters of their own, read-only and unaliased: their loads may then stay off the vector lanes)
template <uint32_t ALT>
__global__ __launch_bounds__(LANES) void assoc_ranksum_permute_kernel(const uint64_t *__restrict__ plane, const uint32_t *__restrict__ offset,
                                                                      const uint32_t *__restrict__ scale, const uint32_t *__restrict__ mult,
                                                                      const uint32_t *__restrict__ obs, Args A) {
  __shared__ unsigned long long cell[MAX_EDGES];      // the block's tail cells
  __shared__ uint32_t edge[MAX_EDGES];
  __shared__ uint32_t over[SLICE];                    // the slice's exceed counters
  const uint32_t t = threadIdx.x, N = A.N, E = A.E;
  const uint64_t bits = sample_bits(N);
  for (uint32_t k = t; k < E; k += LANES) { cell[k] = 0; edge[k] = A.edges[k]; }
  for (uint32_t k = t; k < SLICE; k += LANES) over[k] = 0;
  const uint32_t lowest = E ? A.edges[0] : NO_EDGE;      // (no score reaches NO_EDGE: T_MAX)
  const uint32_t second = E > 1 ? A.edges[1] : NO_EDGE;      // from edges[0] up to here a pair is in cell 0: no search
  uint64_t L[PERMS_PER_LANE];
  uint32_t best[PERMS_PER_LANE], floor_of[PERMS_PER_LANE];      // floor_of: edges[0], or NO_EDGE where the lane has no relabeling
  bool live[PERMS_PER_LANE];
#pragma unroll
  for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
    const uint32_t p = perm_of(blockIdx.y, j, t);
    live[j] = p < A.P;
    L[j] = live[j] ? A.labels[p] : 0;
    best[j] = 0;
    floor_of[j] = live[j] ? lowest : NO_EDGE;
  }
  __syncthreads();
  uint32_t f, f_end;
  slice_of(A.F, blockIdx.x, &f, &f_end);
  const uint32_t f0 = f;
  // (f comes from blockIdx and the loop counter: one value for the wave)
  auto pairs = [&](uint32_t slot, const uint64_t *pl, uint32_t off, uint32_t sc, uint32_t w, uint32_t seen) {
    uint32_t W[PERMS_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < PERMS_PER_LANE; j++) W[j] = 0;
#pragma unroll
    for (uint32_t b = 0; b < PLANES; b++) {
      const uint64_t m = pl[b] & bits;
      if (m) {
#pragma unroll
        for (uint32_t j = 0; j < PERMS_PER_LANE; j++) W[j] += popcount(m & L[j]) << b;
      }
    }
    uint32_t hits = 0, low = 0;      // low: the wave's pairs in cell 0, the fattest cell of a null: counted by ballot, added once
#pragma unroll
    for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
      const uint32_t s = score_of(W[j], N, off, sc, ALT);
      hits += (uint32_t)__popcll(__ballot(live[j] && s >= seen));
      if (w) {
        best[j] = best[j] > s ? best[j] : s;
        const bool in_tail = s >= floor_of[j];
        low += (uint32_t)__popcll(__ballot(in_tail && s < second));
        if (in_tail && s >= second) {
          const uint32_t e = edge_of(edge, E, s);
          if (e < E) atomicAdd(&cell[e], (unsigned long long)w);
        }
      }
    }
    if ((t & 63u) == 0) {
      if (hits) atomicAdd(&over[slot], hits);
      if (low) atomicAdd(&cell[0], (unsigned long long)low * w);
    }
  };
  for (; f + RS_GROUP <= f_end; f += RS_GROUP) {
    uint64_t pl[RS_GROUP][PLANES];
    uint32_t off[RS_GROUP], sc[RS_GROUP], w[RS_GROUP], seen[RS_GROUP];
#pragma unroll
    for (uint32_t g = 0; g < RS_GROUP; g++) {
#pragma unroll
      for (uint32_t b = 0; b < PLANES; b++) pl[g][b] = plane[(uint64_t)(f + g) * PLANES + b];
      off[g] = offset[f + g]; sc[g] = scale[f + g]; w[g] = mult[f + g]; seen[g] = obs[f + g];
    }
#pragma unroll
    for (uint32_t g = 0; g < RS_GROUP; g++) pairs(f + g - f0, pl[g], off[g], sc[g], w[g], seen[g]);
  }
  for (; f < f_end; f++) {
    uint64_t pl[PLANES];
#pragma unroll
    for (uint32_t b = 0; b < PLANES; b++) pl[b] = plane[(uint64_t)f * PLANES + b];
    pairs(f - f0, pl, offset[f], scale[f], mult[f], obs[f]);
  }
#pragma unroll
  for (uint32_t j = 0; j < PERMS_PER_LANE; j++) {
    const uint32_t p = perm_of(blockIdx.y, j, t);
    if (p < A.P && best[j]) atomicMax(&A.perm_max[p], best[j]);
  }
  __syncthreads();
  for (uint32_t k = t; k < E; k += LANES) {
    const unsigned long long c = cell[k];
    if (c) atomicAdd(&A.tail[k], c);
  }
  for (uint32_t k = t; k < f_end - f0; k += LANES) {
    const uint32_t c = over[k];
    if (c) atomicAdd(&A.exceed[f0 + k], c);
  }
}

static_assert(LANES == (uint32_t)dcrx_group::BLOCK, "grid_for() sizes the prepare kernel's grid: a lane per index in blocks of LANES");

int run_ranksum(const Args &A, hipStream_t s) {
  const uint64_t most = std::max<uint64_t>(A.F, A.E);
  if (most) {
    assoc_ranksum_prepare_kernel<<<dcrx_group::grid_for(most), LANES, 0, s>>>(A);
    HIP_TRY(hipGetLastError());
  }
  if (A.P) {
    assoc_ranksum_labels_kernel<<<(A.P + LABEL_LANES - 1) / LABEL_LANES, LABEL_LANES, 0, s>>>(A);
    HIP_TRY(hipGetLastError());
  }
  if (A.F && A.P) {
    const dim3 grid(slices_for(A.F), perm_tiles_for(A.P));
    if (A.alternative == 0) assoc_ranksum_permute_kernel<0><<<grid, LANES, 0, s>>>(A.plane, A.offset, A.scale, A.mult, A.obs_score, A);
    else if (A.alternative == 1) assoc_ranksum_permute_kernel<1><<<grid, LANES, 0, s>>>(A.plane, A.offset, A.scale, A.mult, A.obs_score, A);
    else assoc_ranksum_permute_kernel<2><<<grid, LANES, 0, s>>>(A.plane, A.offset, A.scale, A.mult, A.obs_score, A);
    HIP_TRY(hipGetLastError());
  }
  return DCRX_OK;
}

int refuse(const char *who, uint32_t N, uint64_t C, uint32_t alternative, uint64_t F, uint32_t E, uint32_t P) {
  static thread_local char msg[200];
  const char *why = nullptr;
  const int kind = refuse_scalars(N, C, alternative, F, E, P, &why);
  if (!kind) return DCRX_OK;
  std::snprintf(msg, sizeof msg, "%s: %s", who, why);
  return set_err(kind == 1 ? DCRX_E_INVALID : DCRX_E_UNSUPPORTED, msg);
}

bool null_array(uint64_t F, const void *plane, const void *offset, const void *scale, const void *mult, uint32_t E, const void *edges,
                uint32_t P, const void *obs_score, const void *labels, const void *perm_max, const void *exceed, const void *tail) {
  return (F && (!plane || !offset || !scale || !mult || !obs_score || !exceed)) || (E && (!edges || !tail)) || (P && (!labels || !perm_max));
}

Args args_of(uint32_t N, uint64_t C, uint32_t alternative, uint64_t F, const uint64_t *plane, const uint32_t *offset, const uint32_t *scale,
             const uint32_t *mult, uint32_t E, const uint32_t *edges, uint32_t P, uint64_t seed, uint32_t *obs_score, uint64_t *labels,
             uint32_t *perm_max, uint32_t *exceed, uint64_t *tail) {
  Args A{};
  A.plane = plane; A.offset = offset; A.scale = scale; A.mult = mult; A.edges = edges; A.obs_score = obs_score; A.labels = labels;
  A.perm_max = perm_max; A.exceed = exceed;
  A.tail = reinterpret_cast<unsigned long long *>(tail);
  A.C = C; A.seed = seed; A.N = N; A.n1 = popcount(C); A.alternative = alternative; A.F = (uint32_t)F; A.E = E; A.P = P;
  return A;
}

}  // namespace

extern "C" {

int dcrx_assoc_ranksum_device(uint32_t n_samples, uint64_t case_mask, uint32_t alternative, uint64_t n_features, const uint64_t *d_plane,
                              const uint32_t *d_offset, const uint32_t *d_scale, const uint32_t *d_mult, uint32_t n_edges,
                              const uint32_t *d_edges, uint32_t permutations, uint64_t seed, uint32_t *d_obs_score, uint64_t *d_labels,
                              uint32_t *d_perm_max, uint32_t *d_exceed, uint64_t *d_tail, void *hip_stream) {
  int rc;
  if ((rc = refuse("dcrx_assoc_ranksum_device", n_samples, case_mask, alternative, n_features, n_edges, permutations))) return rc;
  if (null_array(n_features, d_plane, d_offset, d_scale, d_mult, n_edges, d_edges, permutations, d_obs_score, d_labels, d_perm_max, d_exceed,
                 d_tail))
    return set_err(DCRX_E_INVALID, "dcrx_assoc_ranksum_device: null argument");
  return run_ranksum(args_of(n_samples, case_mask, alternative, n_features, d_plane, d_offset, d_scale, d_mult, n_edges, d_edges, permutations,
                             seed, d_obs_score, d_labels, d_perm_max, d_exceed, d_tail),
                     (hipStream_t)hip_stream);
}

int dcrx_assoc_ranksum(uint32_t n_samples, uint64_t case_mask, uint32_t alternative, uint64_t n_features, const uint64_t *plane,
                       const uint32_t *offset, const uint32_t *scale, const uint32_t *mult, uint32_t n_edges, const uint32_t *edges,
                       uint32_t permutations, uint64_t seed, uint32_t *obs_score_out, uint64_t *labels_out, uint32_t *perm_max_out,
                       uint32_t *exceed_out, uint64_t *tail_out, dcrx_assoc_ranksum_stats_t *stats_out) {
  int rc;
  const uint32_t N = n_samples, P = permutations, E = n_edges;
  const uint64_t F = n_features;
  if ((rc = refuse("dcrx_assoc_ranksum", N, case_mask, alternative, F, E, P))) return rc;
  if (null_array(F, plane, offset, scale, mult, E, edges, P, obs_score_out, labels_out, perm_max_out, exceed_out, tail_out))
    return set_err(DCRX_E_INVALID, "dcrx_assoc_ranksum: null argument");
  for (uint64_t i = 0; i < F * PLANES; i++)
    if (plane[i] & ~sample_bits(N)) return set_err(DCRX_E_INVALID, "dcrx_assoc_ranksum: a plane has a bit at or above the number of samples");
  for (uint32_t j = 1; j < E; j++)
    if (edges[j] <= edges[j - 1]) return set_err(DCRX_E_INVALID, "dcrx_assoc_ranksum: the edges are not strictly ascending");
  dcrx_assoc_ranksum_stats_t st{};
  st.features = F;
  st.permutations = P;
  for (uint64_t f = 0; f < F; f++) {
    st.features_weighted += mult[f] ? 1 : 0;
    if ((st.weight += mult[f]) >= MAX_WEIGHT) return set_err(DCRX_E_UNSUPPORTED, "dcrx_assoc_ranksum: the multiplicities sum to 2^32 or more");
  }
  if (!F || !P) {      // answered here: no device is touched
    const uint32_t n1 = popcount(case_mask);
    for (uint64_t f = 0; f < F; f++) {
      obs_score_out[f] = score_of(weighted_sum(plane + f * PLANES, case_mask), N, offset[f], scale[f], alternative);
      exceed_out[f] = 0;
    }
    uint64_t keys[MAX_SAMPLES];
    for (uint32_t p = 0; p < P; p++) {
      stage_keys(keys, 1, seed, p, N);
      labels_out[p] = labels_from_keys(keys, 1, N, n1);
      perm_max_out[p] = 0;
    }
    for (uint32_t j = 0; j < E; j++) tail_out[j] = 0;
    if (stats_out) *stats_out = st;
    return DCRX_OK;
  }
  Pool pool;
  uint64_t *d_plane, *d_labels, *d_tail;
  uint32_t *d_offset, *d_scale, *d_mult, *d_edges, *d_obs, *d_max, *d_exceed;
  for (int pass = 0; pass < 2; pass++) {
    pool.get(&d_plane, F * PLANES); pool.get(&d_labels, P); pool.get(&d_tail, E); pool.get(&d_offset, F); pool.get(&d_scale, F);
    pool.get(&d_mult, F); pool.get(&d_edges, E); pool.get(&d_obs, F); pool.get(&d_max, P); pool.get(&d_exceed, F);
    if (pass == 0 && (rc = pool.allocate())) return rc;
  }
  if ((rc = to_device(d_plane, plane, F * PLANES)) || (rc = to_device(d_offset, offset, F)) || (rc = to_device(d_scale, scale, F)) ||
      (rc = to_device(d_mult, mult, F)) || (rc = to_device(d_edges, edges, E)) ||
      (rc = run_ranksum(args_of(N, case_mask, alternative, F, d_plane, d_offset, d_scale, d_mult, E, d_edges, P, seed, d_obs, d_labels, d_max,
                                d_exceed, d_tail),
                        nullptr)) ||
      (rc = to_host(obs_score_out, d_obs, F)) || (rc = to_host(labels_out, d_labels, P)) || (rc = to_host(perm_max_out, d_max, P)) ||
      (rc = to_host(exceed_out, d_exceed, F)) || (rc = to_host(tail_out, d_tail, E)))
    return rc;
  for (uint32_t j = 0; j < E; j++) st.tail_total += tail_out[j];
  for (uint32_t p = 0; p < P; p++) st.max_perm_score = std::max<uint64_t>(st.max_perm_score, perm_max_out[p]);
  if (stats_out) *stats_out = st;
  return DCRX_OK;
}

}  // extern "C"

// dcrx_overlap.hip — the overlap step (`overlap`): which keys (class, bytes) the rows of several samples share, the
// S x S matrices of what every two samples share, and the public rows; include/dcrx.h holds the contract,
// dcrx_overlap_core.h the per-row and per-pair code.
//
// The host entry (dcrx_overlap_run), on the null stream:
//   keys     overlap_keys_kernel, one lane per row: the hash of (class, bytes)
//   group    a stable radix sort of (hash, rank), then the exact groups under the hash (dcrx_group.h's rounds, with SameKey
//            below as the full-key test).  A run is in rank order, so a group's first row is its head.  The heads flagged in
//            rank order and scanned number the groups.
//   cells    a stable sort of (group, sample) over the bits in use (36 at most), run heads, the rows' weights added onto
//            their run's head by 64-bit atomics whose results are not read, the heads compacted in order; a cell sum of
//            2^32 or more raises a flag that comes back with the number of cells.  n_samples and the group's weight by
//            atomics onto the group, cell_off by an exclusive sum.
//   pairs    dcrx_overlap_pairs_device, below
//   public   flag, compact, the stable sorts (head, weight descending, n_samples descending) and a gather of the cells
// The primitive (dcrx_overlap_pairs_device), on the caller's stream: overlap_pairs_kernel<SMAX, PART>.  A fixed grid of
// blocks takes tiles of 256 cells, one lane per cell.  The block finds the group of the tile's first cell (a binary search
// over cell_off, the same for every lane) and stages the ends of the 256 groups from there in LDS; a lane finds its own
// group's end among them (a tile of 256 cells meets at most 256 groups that hold a cell; behind empty groups a lane falls
// back to a search over cell_off).  The lane adds its diagonal terms and walks the cells from its own to that end — none for
// a group of one cell — adding each pair's terms to the block's planes in LDS; when the block's tiles are done it adds what
// is not zero to the planes in global memory.  PART 0 holds shared (a triangle of uint32), shared_weight (full, uint64) and
// min_weight (a triangle of uint64); PART 1 the two product planes (triangles of uint64).  SMAX (8, 16, 32, 64) sizes the
// planes in LDS for the call's number of samples.
// The sorts, scans, run heads, compactions and those rounds are dcrx_group.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_group.h"
#include "dcrx_overlap_core.h"
#include "dcrx_text.h"

using dcrx::set_err;
using namespace dcrx_ovl;
using namespace dcrx_group;

struct dcrx_overlap {
  uint32_t S = 0;
  uint64_t m = 0;
  dcrx_overlap_stats_t stats{};
  std::vector<uint64_t> planes, rows_per_sample, weight, cell_off, cell_weight;
  std::vector<uint32_t> group_of, head, n_samples, cell_sample;
};

namespace {

constexpr uint64_t MAX_ROWS = 1ull << 30;
constexpr uint64_t MAX_WEIGHT = 1ull << 32;
constexpr unsigned PAIR_GRID = 2048;      // blocks of the pair kernel at most: each takes every PAIR_GRID-th tile
std::atomic<uint32_t> g_hash_bits{64};

struct Rows {
  const uint32_t *cls;
  const uint64_t *off;
  const uint8_t *text;
};

__global__ __launch_bounds__(BLOCK) void overlap_keys_kernel(Rows R, uint32_t m, uint64_t mask, uint64_t *__restrict__ key,
                                                             uint32_t *__restrict__ rank) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= m) return;
  const uint64_t a = R.off[i];
  key[i] = key_hash(R.cls[i], R.text + a, R.off[i + 1] - a) & mask;
  rank[i] = i;
}

// the full-key test of the rounds: two rows' (class, bytes)
struct SameKey {
  Rows R;
  __device__ bool operator()(uint32_t ea, uint32_t eb) const {
    const uint64_t aa = R.off[ea], ab = R.off[eb];
    return key_equal(R.cls[ea], R.text + aa, R.off[ea + 1] - aa, R.cls[eb], R.text + ab, R.off[eb + 1] - ab);
  }
};

// the heads, flagged at their rank: their exclusive sum numbers the groups by head ascending
__global__ __launch_bounds__(BLOCK) void overlap_heads_kernel(const uint32_t *__restrict__ head_of, const uint32_t *__restrict__ rank,
                                                              uint32_t m, uint32_t *__restrict__ is_head) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s < m) is_head[rank[s]] = head_of[s] == s ? 1u : 0u;
}

__global__ __launch_bounds__(BLOCK) void overlap_group_of_kernel(const uint32_t *__restrict__ head_of, const uint32_t *__restrict__ rank,
                                                                 const uint32_t *__restrict__ number, uint32_t m,
                                                                 uint32_t *__restrict__ group_of, uint32_t *__restrict__ head_rank) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= m) return;
  const uint32_t h = head_of[s], g = number[rank[h]];
  group_of[rank[s]] = g;
  if (h == s) head_rank[g] = rank[s];
}

__global__ __launch_bounds__(BLOCK) void overlap_cell_keys_kernel(const uint32_t *__restrict__ group_of, const uint32_t *__restrict__ sample,
                                                                  uint32_t m, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= m) return;
  key[i] = cell_key(group_of[i], sample[i]);
  idx[i] = i;
}

// what the compaction leaves of a cell, and what the cell adds to its group
struct PutCell {
  const uint64_t *key;
  const unsigned long long *sum;
  uint32_t *cell_sample, *cell_weight, *n_samples, *over;
  unsigned long long *group_weight;
  __device__ void operator()(uint32_t slot, uint32_t pos) const {
    const uint64_t k = key[pos];
    const unsigned long long w = sum[pos];
    const uint32_t g = (uint32_t)(k >> SAMPLE_BITS);
    cell_sample[slot] = (uint32_t)k & (MAX_SAMPLES - 1);
    cell_weight[slot] = (uint32_t)w;
    if (w >= MAX_WEIGHT) *over = 1u;
    atomicAdd(&n_samples[g], 1u);
    atomicAdd(&group_weight[g], w);
  }
};

__global__ __launch_bounds__(BLOCK) void overlap_public_flag_kernel(const uint32_t *__restrict__ n_samples, uint32_t n_groups,
                                                                    uint32_t min_samples, uint32_t *__restrict__ flag) {
  const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
  if (g < n_groups) flag[g] = n_samples[g] >= min_samples ? 1u : 0u;
}

__global__ __launch_bounds__(BLOCK) void overlap_public_rows_kernel(const uint32_t *__restrict__ list, uint32_t rows,
                                                                    const uint32_t *__restrict__ head_rank,
                                                                    const uint32_t *__restrict__ n_samples,
                                                                    const unsigned long long *__restrict__ group_weight,
                                                                    uint32_t *__restrict__ head_out, uint32_t *__restrict__ ns_out,
                                                                    uint64_t *__restrict__ weight_out) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r > rows) return;
  if (r == rows) { ns_out[r] = 0; return; }      // (the scan's last entry: the number of public cells)
  const uint32_t g = list[r];
  head_out[r] = head_rank[g]; ns_out[r] = n_samples[g]; weight_out[r] = group_weight[g];
}

__global__ __launch_bounds__(BLOCK) void overlap_public_cells_kernel(const uint32_t *__restrict__ list, uint32_t rows,
                                                                     const uint32_t *__restrict__ cell_off,
                                                                     const uint32_t *__restrict__ cell_sample,
                                                                     const uint32_t *__restrict__ cell_weight,
                                                                     const uint32_t *__restrict__ out_off,
                                                                     uint32_t *__restrict__ sample_out, uint32_t *__restrict__ weight_out) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= rows) return;
  const uint32_t g = list[r], from = cell_off[g], n = cell_off[g + 1] - from, to = out_off[r];
  for (uint32_t k = 0; k < n; k++) {
    sample_out[to + k] = cell_sample[from + k];
    weight_out[to + k] = cell_weight[from + k];
  }
}

// ---- the pair kernel ----

// (first_above and group_end, a lane's look-ups, are dcrx_overlap_core.h's: the host walk of tests/host_overlap shares them)
template <int SMAX, int PART>
__global__ __launch_bounds__(BLOCK) void overlap_pairs_kernel(const uint32_t *__restrict__ cell_off, uint32_t n_groups,
                                                              const uint32_t *__restrict__ cell_sample,
                                                              const uint32_t *__restrict__ cell_weight, uint32_t S,
                                                              unsigned long long *__restrict__ planes) {
  constexpr uint32_t TRI = SMAX * (SMAX + 1) / 2, FULL = SMAX * SMAX;
  __shared__ uint32_t ends[BLOCK];
  __shared__ unsigned long long acc0[TRI];                          // PART 0: min_weight; PART 1: prod_lo
  __shared__ unsigned long long acc1[PART == 0 ? FULL : TRI];       // PART 0: shared_weight (S x S, row major); PART 1: prod_hi
  __shared__ uint32_t cnt[PART == 0 ? TRI : 1];                     // PART 0: shared
  const uint32_t t = threadIdx.x;
  for (uint32_t k = t; k < TRI; k += BLOCK) {
    acc0[k] = 0;
    if (PART == 0) cnt[k] = 0;
    else acc1[k] = 0;
  }
  if (PART == 0)
    for (uint32_t k = t; k < FULL; k += BLOCK) acc1[k] = 0;
  const uint32_t n_cells = cell_off[n_groups];
  const uint32_t tiles = (n_cells + BLOCK - 1) / BLOCK;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t c0 = tile * BLOCK, c = c0 + t;
    // the group of the tile's first cell: the last g with cell_off[g] <= c0 (cell_off[n_groups] = n_cells > c0)
    const uint32_t g_first = first_above(cell_off, 0, n_groups, c0) - 1;
    __syncthreads();      // the previous tile's ends are no longer read (and, the first time, the planes are zero)
    ends[t] = cell_off[min(g_first + 1 + t, n_groups)];
    __syncthreads();
    if (c >= n_cells) continue;
    const uint32_t end = group_end(ends, BLOCK, cell_off, g_first, n_groups, n_cells, c);
    const uint32_t a = cell_sample[c];
    if (a >= S) continue;                               // (outside the contract: never outside the planes)
    const unsigned long long wa = cell_weight[c];
    if (PART == 0) {
      atomicAdd(&cnt[tri_index(a, a)], 1u);
      atomicAdd(&acc1[full_index(S, a, a)], wa);
      atomicAdd(&acc0[tri_index(a, a)], wa);
    } else {
      uint64_t lo, hi;
      product_split(wa, wa, &lo, &hi);
      atomicAdd(&acc0[tri_index(a, a)], (unsigned long long)lo);
      atomicAdd(&acc1[tri_index(a, a)], (unsigned long long)hi);
    }
    for (uint32_t q = c + 1; q < end; q++) {
      const uint32_t b = cell_sample[q];
      if (b >= S) continue;
      const unsigned long long wb = cell_weight[q];
      const uint32_t ti = tri_index(a, b);
      if (PART == 0) {
        atomicAdd(&cnt[ti], 1u);
        atomicAdd(&acc1[full_index(S, a, b)], wa);
        atomicAdd(&acc1[full_index(S, b, a)], wb);
        atomicAdd(&acc0[ti], min(wa, wb));
      } else {
        uint64_t lo, hi;
        product_split(wa, wb, &lo, &hi);
        atomicAdd(&acc0[ti], (unsigned long long)lo);
        atomicAdd(&acc1[ti], (unsigned long long)hi);
      }
    }
  }
  __syncthreads();
  // the block's one flush: what is not zero, onto the planes (a triangle's entry goes to both of its places)
  const uint32_t SS = S * S;
  for (uint32_t idx = t; idx < SS; idx += BLOCK) {
    const uint32_t a = idx / S, b = idx % S, ti = tri_index(a, b);
    if (PART == 0) {
      const unsigned long long n = cnt[ti], sw = acc1[idx], mw = acc0[ti];
      if (n) atomicAdd(&planes[(size_t)P_SHARED * SS + idx], n);
      if (sw) atomicAdd(&planes[(size_t)P_SHARED_WEIGHT * SS + idx], sw);
      if (mw) atomicAdd(&planes[(size_t)P_MIN_WEIGHT * SS + idx], mw);
    } else {
      const unsigned long long lo = acc0[ti], hi = acc1[ti];
      if (lo) atomicAdd(&planes[(size_t)P_PROD_LO * SS + idx], lo);
      if (hi) atomicAdd(&planes[(size_t)P_PROD_HI * SS + idx], hi);
    }
  }
}

template <int SMAX> int launch_pairs(uint32_t n_groups, const uint32_t *d_cell_off, const uint32_t *d_cell_sample,
                                     const uint32_t *d_cell_weight, uint32_t S, unsigned long long *d_planes, hipStream_t s) {
  // (the number of cells is on the device: the grid is sized by the most cells the groups can hold, and a block takes every
  // gridDim.x-th tile of those there are)
  const unsigned grid = (unsigned)std::min<uint64_t>(PAIR_GRID, std::max<uint64_t>(1, ((uint64_t)n_groups * S + BLOCK - 1) / BLOCK));
  overlap_pairs_kernel<SMAX, 0><<<grid, BLOCK, 0, s>>>(d_cell_off, n_groups, d_cell_sample, d_cell_weight, S, d_planes);
  HIP_TRY(hipGetLastError());
  overlap_pairs_kernel<SMAX, 1><<<grid, BLOCK, 0, s>>>(d_cell_off, n_groups, d_cell_sample, d_cell_weight, S, d_planes);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

int run_pairs(uint32_t n_groups, const uint32_t *d_cell_off, const uint32_t *d_cell_sample, const uint32_t *d_cell_weight, uint32_t S,
              unsigned long long *d_planes, hipStream_t s) {
  if (S <= 8) return launch_pairs<8>(n_groups, d_cell_off, d_cell_sample, d_cell_weight, S, d_planes, s);
  if (S <= 16) return launch_pairs<16>(n_groups, d_cell_off, d_cell_sample, d_cell_weight, S, d_planes, s);
  if (S <= 32) return launch_pairs<32>(n_groups, d_cell_off, d_cell_sample, d_cell_weight, S, d_planes, s);
  return launch_pairs<64>(n_groups, d_cell_off, d_cell_sample, d_cell_weight, S, d_planes, s);
}

int bits_for(uint64_t values) {      // the bits that hold 0 .. values - 1
  int b = 1;
  while (b < 64 && (1ull << b) < values) b++;
  return b;
}

// the step, into O; a negative dcrx_error otherwise
int run(uint32_t S, uint64_t m, const uint32_t *sample, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
        uint32_t min_samples, dcrx_overlap &O) {
  const uint32_t m32 = (uint32_t)m, SS = S * S;
  const uint64_t text_bytes = off[m] - off[0];
  size_t cub_bytes = 0;
  int rc;
  if ((rc = sort_pairs_bytes<uint32_t>(m, 64, &cub_bytes)) || (rc = exclusive_sum_bytes<uint32_t>(m + 1, &cub_bytes)) ||
      (rc = run_heads_bytes(m, &cub_bytes))) return rc;

  Pool P;
  uint32_t *d_sample, *d_cls, *d_rank[2], *d_head_of, *d_flag, *d_group_of, *d_head_rank, *d_cell_sample, *d_cell_weight, *d_ns,
      *d_cell_off, *d_list[2], *d_kept, *d_pub_head, *d_pub_ns, *d_pub_off, *d_pub_sample, *d_pub_cw;
  GroupWork W;      // (its mark, first and slot serve the cells and the public rows too)
  uint64_t *d_off, *d_weight, *d_key[2], *d_pub_weight;
  unsigned long long *d_sum, *d_gweight, *d_planes;
  uint8_t *d_text, *d_cub;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_sample, m); P.get(&d_cls, m); P.get(&d_off, m + 1); P.get(&d_text, text_bytes); P.get(&d_weight, m);
    P.get(&d_key[0], m); P.get(&d_key[1], m); P.get(&d_rank[0], m); P.get(&d_rank[1], m); W.get(P, m);
    P.get(&d_head_of, m); P.get(&d_flag, m + 1); P.get(&d_group_of, m); P.get(&d_head_rank, m); P.get(&d_sum, m);
    P.get(&d_cell_sample, m); P.get(&d_cell_weight, m); P.get(&d_ns, m + 1); P.get(&d_gweight, m); P.get(&d_cell_off, m + 1);
    P.get(&d_list[0], m); P.get(&d_list[1], m); P.get(&d_kept, 2); P.get(&d_planes, (uint64_t)PLANES * SS); P.get(&d_pub_head, m);
    P.get(&d_pub_ns, m + 1); P.get(&d_pub_off, m + 1); P.get(&d_pub_weight, m); P.get(&d_pub_sample, m); P.get(&d_pub_cw, m);
    P.get(&d_cub, cub_bytes);
    if (pass == 0 && (rc = P.allocate())) return rc;
  }
  if ((rc = upload_spans(m, off, text, d_off, d_text)) || (rc = to_device(d_sample, sample, m)) || (rc = to_device(d_cls, cls, m)) ||
      (rc = to_device(d_weight, weight, m))) return rc;
  const Rows R{d_cls, d_off, d_text};
  const Scratch cub{d_cub, cub_bytes};

  // keys, the sort by hash, the rounds: head_of
  overlap_keys_kernel<<<grid_for(m), BLOCK>>>(R, m32, low_bits(g_hash_bits.load()), d_key[0], d_rank[0]);
  HIP_TRY(hipGetLastError());
  if ((rc = sort_pairs(cub, d_key[0], d_key[1], d_rank[0], d_rank[1], m, 64, nullptr))) return rc;
  const uint32_t *d_sorted = d_rank[1];
  if ((rc = exact_groups(cub, d_key[1], d_sorted, m32, SameKey{R}, W, d_head_of, "dcrx_overlap_run: a round resolved nothing", nullptr)))
    return rc;

  // the groups, numbered by head ascending
  overlap_heads_kernel<<<grid_for(m), BLOCK>>>(d_head_of, d_sorted, m32, d_flag);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_sum(cub, d_flag, W.slot, m, nullptr))) return rc;
  overlap_group_of_kernel<<<grid_for(m), BLOCK>>>(d_head_of, d_sorted, W.slot, m32, d_group_of, d_head_rank);
  HIP_TRY(hipGetLastError());
  uint32_t last[2] = {0, 0};
  if ((rc = to_host(&last[0], W.slot + (m - 1), 1)) || (rc = to_host(&last[1], d_flag + (m - 1), 1))) return rc;
  const uint32_t n_groups = last[0] + last[1];

  // cells: the rows sorted (stably) by (group, sample); a run is a cell
  overlap_cell_keys_kernel<<<grid_for(m), BLOCK>>>(d_group_of, d_sample, m32, d_key[0], d_rank[0]);
  HIP_TRY(hipGetLastError());
  if ((rc = sort_pairs(cub, d_key[0], d_key[1], d_rank[0], d_rank[1], m, bits_for(n_groups) + (int)SAMPLE_BITS, nullptr))) return rc;
  HIP_TRY(hipMemsetAsync(d_ns, 0, ((uint64_t)n_groups + 1) * 4, nullptr));
  HIP_TRY(hipMemsetAsync(d_gweight, 0, (uint64_t)n_groups * 8, nullptr));
  HIP_TRY(hipMemsetAsync(d_kept, 0, 8, nullptr));
  if ((rc = cell_sums(cub, d_key[1], d_rank[1], d_weight, m32, W.mark, W.first, d_sum, d_flag, nullptr))) return rc;
  if ((rc = compact(cub, d_flag, W.slot, m32, PutCell{d_key[1], d_sum, d_cell_sample, d_cell_weight, d_ns, d_kept + 1, d_gweight}, d_kept,
                    nullptr))) return rc;
  uint32_t kept[2] = {0, 0};      // the number of cells, and with it the flag of a cell that passed 2^32
  if ((rc = to_host(kept, d_kept, 2))) return rc;
  if (kept[1]) return set_err(DCRX_E_UNSUPPORTED, "dcrx_overlap_run: a cell's weight (the sum of one sample's rows under one key) is 2^32 or more");
  const uint32_t n_cells = kept[0];
  if ((rc = exclusive_sum(cub, d_ns, d_cell_off, (uint64_t)n_groups + 1, nullptr))) return rc;

  // pairs
  HIP_TRY(hipMemsetAsync(d_planes, 0, (uint64_t)PLANES * SS * 8, nullptr));
  if ((rc = run_pairs(n_groups, d_cell_off, d_cell_sample, d_cell_weight, S, d_planes, nullptr))) return rc;

  // public rows: flag, compact (group order is head order), weight descending, n_samples descending
  overlap_public_flag_kernel<<<grid_for(n_groups), BLOCK>>>(d_ns, n_groups, min_samples, d_flag);
  HIP_TRY(hipGetLastError());
  if ((rc = compact(cub, d_flag, W.slot, n_groups, PutIndex{d_list[0]}, d_kept, nullptr))) return rc;
  uint32_t rows = 0;
  if ((rc = to_host(&rows, d_kept, 1))) return rc;
  if ((rc = most_common_order(cub, d_list, d_key, d_head_rank, 32, d_gweight, rows, nullptr))) return rc;
  const uint32_t *d_order = d_list[0];
  if (rows) {
    if ((rc = gather(d_ns, d_list[0], rows, 1, d_key[0], nullptr)) ||
        (rc = sort_pairs(cub, d_key[0], d_key[1], d_list[0], d_list[1], rows, SAMPLE_BITS + 1, nullptr))) return rc;
    d_order = d_list[1];
  }
  overlap_public_rows_kernel<<<grid_for((uint64_t)rows + 1), BLOCK>>>(d_order, rows, d_head_rank, d_ns, d_gweight, d_pub_head, d_pub_ns,
                                                                      d_pub_weight);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_sum(cub, d_pub_ns, d_pub_off, (uint64_t)rows + 1, nullptr))) return rc;
  if (rows) {
    overlap_public_cells_kernel<<<grid_for(rows), BLOCK>>>(d_order, rows, d_cell_off, d_cell_sample, d_cell_weight, d_pub_off, d_pub_sample,
                                                           d_pub_cw);
    HIP_TRY(hipGetLastError());
  }

  // back to the host
  std::vector<uint32_t> ns(n_groups), off32((size_t)rows + 1), cw32;
  if ((rc = to_host(O.planes.data(), reinterpret_cast<const uint64_t *>(d_planes), (uint64_t)PLANES * SS)) ||
      (rc = to_host(O.group_of.data(), d_group_of, m)) || (rc = to_host(ns.data(), d_ns, n_groups)) ||
      (rc = to_host(off32.data(), d_pub_off, (uint64_t)rows + 1))) return rc;
  const uint32_t pub_cells = off32[rows];
  O.head.resize(rows); O.n_samples.resize(rows); O.weight.resize(rows);
  O.cell_off.assign(off32.begin(), off32.end());
  O.cell_sample.resize(pub_cells); O.cell_weight.resize(pub_cells); cw32.resize(pub_cells);
  if ((rc = to_host(O.head.data(), d_pub_head, rows)) || (rc = to_host(O.n_samples.data(), d_pub_ns, rows)) ||
      (rc = to_host(O.weight.data(), d_pub_weight, rows)) || (rc = to_host(O.cell_sample.data(), d_pub_sample, pub_cells)) ||
      (rc = to_host(cw32.data(), d_pub_cw, pub_cells))) return rc;
  for (uint32_t k = 0; k < pub_cells; k++) O.cell_weight[k] = cw32[k];
  dcrx_overlap_stats_t &T = O.stats;
  T.groups = n_groups;
  for (uint32_t g = 0; g < n_groups; g++) {
    if (ns[g] == 1) T.private_groups++;
    else T.shared_groups++;
    if (ns[g] == S) T.in_all_samples++;
    T.largest_n_samples = std::max<uint64_t>(T.largest_n_samples, ns[g]);
  }
  T.public_rows = rows;
  T.public_cells = pub_cells;
  (void)n_cells;
  return DCRX_OK;
}

}  // namespace

extern "C" {

int dcrx_overlap_set_hash_bits(uint32_t bits) {
  if (bits > 64) return set_err(DCRX_E_INVALID, "dcrx_overlap_set_hash_bits: 0 .. 64 bits");
  g_hash_bits.store(bits);
  return DCRX_OK;
}

dcrx_overlap_t *dcrx_overlap_run(uint32_t n_samples, uint64_t m, const uint32_t *sample, const uint32_t *cls, const uint64_t *off,
                                 const char *text, const uint64_t *weight, uint32_t min_samples, int *error_out) {
  auto fail = [&](int code, const char *what) -> dcrx_overlap_t * {
    const int rc = what ? set_err(code, what) : code;      // (what == nullptr: the message is set already)
    if (error_out) *error_out = rc;
    return nullptr;
  };
  if (error_out) *error_out = DCRX_OK;
  if (n_samples < 1 || n_samples > MAX_SAMPLES) return fail(DCRX_E_INVALID, "dcrx_overlap_run: 1 .. DCRX_OVERLAP_MAX_SAMPLES (64) samples");
  if (!min_samples) return fail(DCRX_E_INVALID, "dcrx_overlap_run: min_samples is 1 or more");
  if (m >= MAX_ROWS) return fail(DCRX_E_UNSUPPORTED, "dcrx_overlap_run: 2^30 or more rows");
  if (m && (!sample || !cls || !off || !weight)) return fail(DCRX_E_INVALID, "dcrx_overlap_run: null argument");
  dcrx_overlap *O = nullptr;
  try {
    O = new dcrx_overlap();
    O->S = n_samples;
    O->m = m;
    O->stats.rows_in = m;
    O->planes.assign((size_t)PLANES * n_samples * n_samples, 0);
    O->rows_per_sample.assign(n_samples, 0);
    O->group_of.assign(m, 0);
    O->cell_off.assign(1, 0);
  } catch (const std::exception &e) {
    delete O;
    return fail(DCRX_E_NOMEM, e.what());
  }
  for (uint64_t k = 0; k < m; k++) {
    const char *bad = nullptr;
    int code = DCRX_E_INVALID;
    if (sample[k] >= n_samples) bad = "dcrx_overlap_run: a sample id outside 0 .. n_samples - 1";
    else if (off[k + 1] < off[k]) bad = "dcrx_overlap_run: offsets go backwards";
    else if (weight[k] >= MAX_WEIGHT) { bad = "dcrx_overlap_run: a row's weight is 2^32 or more"; code = DCRX_E_UNSUPPORTED; }
    if (bad) { delete O; return fail(code, bad); }
    O->rows_per_sample[sample[k]]++;
  }
  if (m && off[m] > off[0] && !text) { delete O; return fail(DCRX_E_INVALID, "dcrx_overlap_run: text is null"); }
  if (m) {
    int rc;
    try {
      rc = run(n_samples, m, sample, cls, off, text, weight, min_samples, *O);
    } catch (const std::exception &e) {
      rc = set_err(DCRX_E_NOMEM, e.what());
    }
    if (rc) { delete O; return fail(rc, nullptr); }
  }
  return O;
}

void dcrx_overlap_destroy(dcrx_overlap_t *O) { delete O; }

int dcrx_overlap_info(const dcrx_overlap_t *O, uint32_t *n_samples, uint64_t *n_rows, uint64_t *n_public, uint64_t *n_public_cells,
                      dcrx_overlap_stats_t *stats) {
  if (!O) return set_err(DCRX_E_INVALID, "dcrx_overlap_info: null handle");
  if (n_samples) *n_samples = O->S;
  if (n_rows) *n_rows = O->m;
  if (n_public) *n_public = O->head.size();
  if (n_public_cells) *n_public_cells = O->cell_sample.size();
  if (stats) *stats = O->stats;
  return DCRX_OK;
}

int dcrx_overlap_export(const dcrx_overlap_t *O, uint64_t *planes, uint32_t *group_of, uint64_t *rows_per_sample, uint32_t *head,
                        uint32_t *n_samples, uint64_t *weight, uint64_t *cell_off, uint32_t *cell_sample, uint64_t *cell_weight) {
  if (!O) return set_err(DCRX_E_INVALID, "dcrx_overlap_export: null handle");
  auto copy = [](auto *dst, const auto &src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0]));
  };
  copy(planes, O->planes); copy(group_of, O->group_of); copy(rows_per_sample, O->rows_per_sample); copy(head, O->head);
  copy(n_samples, O->n_samples); copy(weight, O->weight); copy(cell_off, O->cell_off); copy(cell_sample, O->cell_sample);
  copy(cell_weight, O->cell_weight);
  return DCRX_OK;
}

int dcrx_overlap_pairs_device(uint64_t n_groups, const uint32_t *d_cell_off, const uint32_t *d_cell_sample, const uint32_t *d_cell_weight,
                              uint32_t n_samples, uint64_t *d_planes, void *hip_stream) {
  if (n_samples < 1 || n_samples > MAX_SAMPLES)
    return set_err(DCRX_E_INVALID, "dcrx_overlap_pairs_device: 1 .. DCRX_OVERLAP_MAX_SAMPLES (64) samples");
  if (n_groups >= MAX_ROWS) return set_err(DCRX_E_UNSUPPORTED, "dcrx_overlap_pairs_device: 2^30 or more groups");
  if (!n_groups) return DCRX_OK;
  if (!d_cell_off || !d_cell_sample || !d_cell_weight || !d_planes) return set_err(DCRX_E_INVALID, "dcrx_overlap_pairs_device: null argument");
  return run_pairs((uint32_t)n_groups, d_cell_off, d_cell_sample, d_cell_weight, n_samples, reinterpret_cast<unsigned long long *>(d_planes),
                   (hipStream_t)hip_stream);
}

int64_t dcrx_format_overlap_public(uint64_t n_public, const uint32_t *head, const uint32_t *n_samples, const uint64_t *weight,
                                   const uint64_t *cell_off, const uint32_t *cell_sample, const uint64_t *cell_weight,
                                   uint32_t n_sample_names, const char *sample_names, const uint32_t *sample_name_off, uint64_t m,
                                   const uint32_t *v_idx, const uint32_t *j_idx, uint32_t n_v, const char *v_calls,
                                   const uint32_t *v_call_off, uint32_t n_j, const char *j_calls, const uint32_t *j_call_off,
                                   const uint64_t *off, const char *text, char *out, uint64_t out_cap) {
  static const char header[] = "v_call\tj_call\tjunction_aa\tn_samples\tduplicate_count";
  const uint32_t S = n_sample_names;
  if (S < 1 || S > MAX_SAMPLES) return set_err(DCRX_E_INVALID, "dcrx_format_overlap_public: 1 .. DCRX_OVERLAP_MAX_SAMPLES (64) samples");
  if (!sample_names || !sample_name_off ||
      (n_public && (!head || !n_samples || !weight || !cell_off || !cell_sample || !cell_weight || !v_idx || !j_idx || !v_calls ||
                    !v_call_off || !j_calls || !j_call_off || !off)))
    return set_err(DCRX_E_INVALID, "dcrx_format_overlap_public: null argument");
  dcrx::TextOut T{out, out_cap};
  T.put(header, sizeof header - 1);
  for (uint32_t s = 0; s < S; s++) {
    T.put("\t", 1);
    T.put_span(sample_names, sample_name_off, s);
  }
  T.put("\n", 1);
  for (uint64_t r = 0; r < n_public; r++) {
    const uint64_t e = head[r];
    if (e >= m) return set_err(DCRX_E_INVALID, "dcrx_format_overlap_public: a head outside the rows");
    const uint32_t vi = v_idx[e], ji = j_idx[e];
    if (vi >= n_v || ji >= n_j) return set_err(DCRX_E_INVALID, "dcrx_format_overlap_public: a gene outside its table");
    if (off[e + 1] < off[e] || cell_off[r + 1] < cell_off[r]) return set_err(DCRX_E_INVALID, "dcrx_format_overlap_public: offsets go backwards");
    T.put_span(v_calls, v_call_off, vi); T.put("\t", 1);
    T.put_span(j_calls, j_call_off, ji); T.put("\t", 1);
    T.put_span(text, off, e); T.put("\t", 1);
    T.unum(n_samples[r]); T.put("\t", 1);
    T.unum(weight[r]);
    uint64_t k = cell_off[r];
    for (uint32_t s = 0; s < S; s++) {
      T.put("\t", 1);
      if (k < cell_off[r + 1] && cell_sample[k] == s) T.unum(cell_weight[k++]);
      else T.put("0", 1);
    }
    if (k != cell_off[r + 1]) return set_err(DCRX_E_INVALID, "dcrx_format_overlap_public: a row's cells are not samples ascending below the number of samples");
    T.put("\n", 1);
  }
  return (int64_t)T.at;
}

}  // extern "C"

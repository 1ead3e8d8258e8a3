// dcrx_rarefy.hip — the downsampling step (`overlap --downsample`) and the abundance classes of `overlap --diversity`;
// include/dcrx.h "downsample" holds the contract, dcrx_rarefy_core.h the key, the digits, the sizes and a lane's row look-up.
//
// The primitive (dcrx_downsample_device), on the caller's stream, nothing copied back:
//   offsets    G = the exclusive sum of the weights (hipCUB): one index space over the reads of all samples
//   samples    rarefy_samples_kernel, a lane per sample: its first row (a search over the sample ids), its reads, n_s, its seed,
//              and whether it takes part in the selection (n_s < X_s)
//   select     LEVELS times rarefy_walk_kernel<HIST> and rarefy_bin_kernel: a level's histogram of one 12-bit digit over the
//              keys that carry the sample's digits so far, then the bin of the wanted rank, a block per sample; a sample goes
//              on to the next level while its bin holds more than CANDIDATES keys.  A level nobody needs returns at once.
//   collect    rarefy_walk_kernel<COLLECT>: the keys of every sample's bin, written out (4096 per sample at most)
//   threshold  rarefy_threshold_kernel, a block per sample: the key with `rank` smaller keys among them
//   count      rarefy_walk_kernel<COUNT>: key < T per read; per run of a wave's lanes in one row one add onto kept[row]
// rarefy_walk_kernel is the walk over the reads: a block takes a run of tiles of TILE consecutive reads; per tile it finds the
// first row by a search over G (the same for every lane), stages the SLOTS offsets behind it in LDS, and a lane takes reads
// g0 + j LANES + lane.  A tile inside one row (a heavy row) needs no look-up, and in the count pass one add per wave.
// dcrx_abundance_classes is made of dcrx_group.h's helpers alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_group.h"
#include "dcrx_overlap_core.h"
#include "dcrx_rarefy_core.h"

using dcrx::set_err;
using namespace dcrx_group;
using namespace dcrx_rar;

static_assert(LANES == BLOCK, "a block of the walk is dcrx_group.h's");

namespace {

constexpr uint32_t NO_SAMPLE = 0xFFFFFFFFu, NO_ROW = 0xFFFFFFFFu;
enum { HIST = 0, COLLECT = 1, COUNT = 2 };

struct Control {
  unsigned long long total;          // the reads the walks cover: the sum of the weights, or 0 where it is 2^40 or more
  uint32_t n_active[LEVELS + 1];     // samples that need a level's histogram
  uint32_t n_collect;                // samples whose bin is written out
};

// what a walk reads and writes: all in the caller's work space but the first two and the last
struct State {
  const uint32_t *sample;
  const uint64_t *weight;
  uint64_t *G;                       // m + 1 offsets
  uint64_t *base;                    // S + 1: a sample's first read in the index space
  uint64_t *s_seed, *rank, *prefix;  // per sample: its seed, the rank wanted inside the prefix, the digits decided so far
  uint32_t *levels, *active, *all, *cand_n;      // per sample: digits decided, needs a further level, keeps every read, keys written
  unsigned long long *hist;          // S x BINS
  uint64_t *cand;                    // S x CANDIDATES
  Control *ctl;
  uint64_t *threshold;
  unsigned long long *kept;
  uint32_t m, S;
};

__global__ __launch_bounds__(BLOCK) void rarefy_samples_kernel(State Q, const uint64_t *__restrict__ depth, uint64_t seed,
                                                               uint64_t *__restrict__ reads, uint64_t *__restrict__ depth_used) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s > Q.S) return;
  const uint32_t m = Q.m;
  const uint64_t sum = m ? Q.G[m - 1] + Q.weight[m - 1] : 0;
  const bool fits = sum < MAX_READS;
  if (s == Q.S) {
    Q.G[m] = sum;
    Q.base[s] = sum;
    Q.ctl->total = fits ? sum : 0;
    return;
  }
  const uint32_t lo = first_row_of(Q.sample, m, s), hi = first_row_of(Q.sample, m, s + 1);
  const uint64_t b0 = lo < m ? Q.G[lo] : sum, b1 = hi < m ? Q.G[hi] : sum;
  const uint64_t X = b1 - b0, n = fits ? min_u64(depth[s], X) : 0;
  const bool all = fits && n == X;
  reads[s] = X;
  depth_used[s] = n;
  Q.threshold[s] = all ? ~0ull : 0;
  Q.base[s] = b0;
  Q.s_seed[s] = sample_seed(seed, s);
  Q.rank[s] = n;
  Q.prefix[s] = 0;
  Q.levels[s] = 0;
  Q.all[s] = all ? 1u : 0u;
  Q.cand_n[s] = 0;
  const bool active = fits && !all;
  Q.active[s] = active ? 1u : 0u;
  if (active) atomicAdd(&Q.ctl->n_active[0], 1u);
}

// a block's histogram onto the sample's (what is not zero), and zero again
__device__ __forceinline__ void flush_hist(uint32_t *lh, unsigned long long *__restrict__ to, bool add) {
  for (uint32_t k = threadIdx.x; k < BINS; k += BLOCK) {
    const uint32_t c = lh[k];
    if (add && c) atomicAdd(&to[k], (unsigned long long)c);
    lh[k] = 0;
  }
}

template <int MODE> __global__ __launch_bounds__(BLOCK) void rarefy_walk_kernel(State Q, uint32_t level) {
  __shared__ uint64_t ends[SLOTS];
  __shared__ uint32_t lh[MODE == HIST ? BINS : 1];
  if (MODE == HIST && Q.ctl->n_active[level] == 0) return;
  if (MODE == COLLECT && Q.ctl->n_collect == 0) return;
  const uint64_t total = Q.ctl->total;
  const uint32_t t = threadIdx.x, m = Q.m, S = Q.S;
  uint32_t tile, tile_end, cur = NO_SAMPLE;      // cur: the sample the block's histogram in LDS belongs to
  block_tiles(total, blockIdx.x, gridDim.x, &tile, &tile_end);
  for (; tile < tile_end; tile++) {
    const uint64_t g0 = (uint64_t)tile * TILE, g_end = min_u64(g0 + TILE, total);
    // the row of the tile's first read: the last i with G[i] <= g0 (G[m] = total > g0)
    const uint32_t i0 = first_above(Q.G, 0, m, g0) - 1;
    __syncthreads();      // the previous tile's ends and its adds to the histogram are done
    if (MODE == HIST) {
      const uint32_t s0 = Q.sample[i0];
      if (s0 != cur) {      // (the same for every lane: samples go up along a block's tiles, so a block flushes once per sample)
        flush_hist(lh, Q.hist + (size_t)min_u32(cur, S - 1) * BINS, cur < S);
        cur = s0;
      }
    }
    for (uint32_t k = t; k < SLOTS; k += BLOCK) ends[k] = Q.G[min_u32(i0 + 1 + k, m)];
    __syncthreads();
    const bool one_row = ends[0] >= g_end;      // the whole tile lies in row i0
    unsigned long long mine = 0;                // COUNT, one_row: this lane's kept reads
#pragma unroll 2
    for (uint32_t j = 0; j < PER_LANE; j++) {
      const uint64_t g = g0 + (uint64_t)j * BLOCK + t;
      const bool valid = g < g_end;
      uint32_t row = NO_ROW, s = NO_SAMPLE;
      if (valid) {
        row = one_row ? i0 : row_of(ends, SLOTS, Q.G, i0, m, g);
        s = Q.sample[row];
        if (s >= S) s = NO_SAMPLE;      // (outside the contract: never outside the arrays)
      }
      bool keep = false;
      if (s != NO_SAMPLE) {
        if (MODE == HIST) {
          if (Q.active[s]) {
            const uint64_t k = key_of(Q.s_seed[s], g - Q.base[s]);
            if (prefix_of(k, level) == Q.prefix[s]) {
              if (s == cur) atomicAdd(&lh[digit(k, level)], 1u);
              else atomicAdd(&Q.hist[(size_t)s * BINS + digit(k, level)], 1ull);
            }
          }
        } else if (MODE == COLLECT) {
          const uint32_t L = Q.levels[s];
          if (L) {
            const uint64_t k = key_of(Q.s_seed[s], g - Q.base[s]);
            if (prefix_of(k, L) == Q.prefix[s]) {
              const uint32_t slot = atomicAdd(&Q.cand_n[s], 1u);
              if (slot < CANDIDATES) Q.cand[(size_t)s * CANDIDATES + slot] = k;
            }
          }
        } else {
          keep = Q.all[s] || key_of(Q.s_seed[s], g - Q.base[s]) < Q.threshold[s];
        }
      }
      if (MODE == COUNT) {
        if (one_row) {
          mine += keep ? 1 : 0;
        } else {
          // the wave's runs of lanes in one row: one add per run (rows go up along the lanes; a lane without a read has no row)
          const uint32_t lane = t & 63u;
          const uint32_t before = __shfl_up(row, 1);
          const uint64_t heads = __ballot(lane == 0 || before != row), keeps = __ballot(keep);
          if ((heads >> lane & 1) && row != NO_ROW) {
            const uint32_t n = run_kept(heads, keeps, lane);
            if (n) atomicAdd(&Q.kept[row], (unsigned long long)n);
          }
        }
      }
    }
    if (MODE == COUNT && one_row) {
      mine = wave_sum(mine);
      if ((t & 63u) == 0 && mine) atomicAdd(&Q.kept[i0], mine);
    }
  }
  if (MODE == HIST) {
    __syncthreads();
    flush_hist(lh, Q.hist + (size_t)min_u32(cur, S - 1) * BINS, cur < S);
  }
}

// a level's verdict for a sample, a block per sample: the bin that holds the key of the wanted rank becomes the next digit
__global__ __launch_bounds__(BLOCK) void rarefy_bin_kernel(State Q, uint32_t level) {
  constexpr uint32_t SHARE = BINS / BLOCK;
  __shared__ unsigned long long part[BLOCK];
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  if (!Q.active[s]) return;      // (the same for the whole block)
  const unsigned long long rank = Q.rank[s];      // (read by every lane before the one that finds the bin writes it)
  unsigned long long *h = Q.hist + (size_t)s * BINS;
  unsigned long long sum = 0;
  for (uint32_t k = 0; k < SHARE; k++) sum += h[t * SHARE + k];
  part[t] = sum;
  __syncthreads();
  unsigned long long below = 0;
  for (uint32_t k = 0; k < t; k++) below += part[k];
  if (rank >= below && rank < below + sum) {      // one lane: the ranks of its bins hold the wanted one
    uint32_t b = t * SHARE;
    unsigned long long c = h[b];
    while (rank >= below + c) { below += c; c = h[++b]; }      // (stops inside the lane's share: rank < below + sum)
    Q.rank[s] = rank - below;
    Q.prefix[s] = (Q.prefix[s] << BIN_BITS) | b;
    Q.levels[s] = level + 1;
    if (c <= CANDIDATES || level + 1 == LEVELS) {
      Q.active[s] = 0;
      atomicAdd(&Q.ctl->n_collect, 1u);
    } else {
      atomicAdd(&Q.ctl->n_active[level + 1], 1u);
    }
  }
  __syncthreads();
  for (uint32_t k = t; k < BINS; k += BLOCK) h[k] = 0;      // for the next level, and the next call
}

// a block per sample: the key with `rank` smaller keys among the sample's candidates (keys are distinct: there is one)
__global__ __launch_bounds__(BLOCK) void rarefy_threshold_kernel(State Q) {
  __shared__ uint64_t keys[CANDIDATES];
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  if (!Q.levels[s]) return;
  const uint32_t n = min_u32(Q.cand_n[s], CANDIDATES);
  for (uint32_t k = t; k < n; k += BLOCK) keys[k] = Q.cand[(size_t)s * CANDIDATES + k];
  __syncthreads();
  const uint64_t rank = Q.rank[s];
  for (uint32_t k = t; k < n; k += BLOCK) {
    const uint64_t mine = keys[k];
    uint32_t smaller = 0;
    for (uint32_t q = 0; q < n; q++) smaller += keys[q] < mine ? 1u : 0u;
    if (smaller == rank) Q.threshold[s] = mine;
  }
}

// ---- work space of the primitive: what of a State lies there, and hipCUB's scratch
struct Work {
  State Q{};
  Scratch cub;
  int carve(Pool &P, uint64_t m, uint32_t S) {
    size_t b = 0;
    const int rc = exclusive_sum_bytes<uint64_t>(std::max<uint64_t>(m, 1), &b);
    if (rc) return rc;
    P.get(&Q.G, m + 1); P.get(&Q.base, (uint64_t)S + 1); P.get(&Q.s_seed, S); P.get(&Q.rank, S); P.get(&Q.prefix, S);
    P.get(&Q.levels, S); P.get(&Q.active, S); P.get(&Q.all, S); P.get(&Q.cand_n, S); P.get(&Q.hist, (uint64_t)S * BINS);
    P.get(&Q.cand, (uint64_t)S * CANDIDATES); P.get(&Q.ctl, 1); P.get(&cub, b);
    return DCRX_OK;
  }
};

int run_downsample(uint32_t S, uint64_t m, const uint32_t *d_sample, const uint64_t *d_weight, const uint64_t *d_depth, uint64_t seed,
                   uint64_t *d_kept, uint64_t *d_reads, uint64_t *d_depth_used, uint64_t *d_threshold, const Work &W, hipStream_t s) {
  State Q = W.Q;
  Q.sample = d_sample; Q.weight = d_weight;
  Q.threshold = d_threshold; Q.kept = reinterpret_cast<unsigned long long *>(d_kept);
  Q.m = (uint32_t)m; Q.S = S;
  int rc;
  HIP_TRY(hipMemsetAsync(Q.ctl, 0, sizeof(Control), s));
  if (m) {
    HIP_TRY(hipMemsetAsync(Q.hist, 0, (uint64_t)S * BINS * 8, s));
    HIP_TRY(hipMemsetAsync(d_kept, 0, m * 8, s));
    if ((rc = exclusive_sum(W.cub, d_weight, Q.G, m, s))) return rc;
  }
  rarefy_samples_kernel<<<grid_for((uint64_t)S + 1), BLOCK, 0, s>>>(Q, d_depth, seed, d_reads, d_depth_used);
  HIP_TRY(hipGetLastError());
  if (!m) return DCRX_OK;
  for (uint32_t level = 0; level < LEVELS; level++) {
    rarefy_walk_kernel<HIST><<<GRID, BLOCK, 0, s>>>(Q, level);
    HIP_TRY(hipGetLastError());
    rarefy_bin_kernel<<<S, BLOCK, 0, s>>>(Q, level);
    HIP_TRY(hipGetLastError());
  }
  rarefy_walk_kernel<COLLECT><<<GRID, BLOCK, 0, s>>>(Q, 0);
  HIP_TRY(hipGetLastError());
  rarefy_threshold_kernel<<<S, BLOCK, 0, s>>>(Q);
  HIP_TRY(hipGetLastError());
  rarefy_walk_kernel<COUNT><<<GRID, BLOCK, 0, s>>>(Q, 0);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// ---- the abundance classes ----

constexpr uint64_t MAX_ITEMS = 1ull << 30;
constexpr uint64_t MAX_WEIGHT = 1ull << 32;

__global__ __launch_bounds__(BLOCK) void classes_cell_keys_kernel(const uint32_t *__restrict__ sample, const uint32_t *__restrict__ group,
                                                                  uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  key[i] = ((uint64_t)sample[i] << 32) | group[i];
  idx[i] = i;
}

// the cells that stay: the heads whose sum is not zero
__global__ __launch_bounds__(BLOCK) void classes_cell_flags_kernel(const uint32_t *__restrict__ head, const unsigned long long *__restrict__ sum,
                                                                   uint32_t n, uint32_t *__restrict__ flag) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s < n) flag[s] = head[s] == s && sum[s] ? 1u : 0u;
}

struct PutClassKey {      // a cell's (sample, weight), and the flag of a sum that passed 2^32
  const uint64_t *key;
  const unsigned long long *sum;
  uint64_t *out;
  uint32_t *idx, *over;
  __device__ void operator()(uint32_t slot, uint32_t pos) const {
    const unsigned long long w = sum[pos];
    if (w >= MAX_WEIGHT) *over = 1u;
    out[slot] = (key[pos] >> 32 << 32) | (uint32_t)w;
    idx[slot] = slot;
  }
};

__global__ __launch_bounds__(BLOCK) void classes_head_flags_kernel(const uint32_t *__restrict__ head, uint32_t n, uint32_t *__restrict__ flag) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s < n) flag[s] = head[s] == s ? 1u : 0u;
}

int run_classes(uint32_t S, uint64_t n, const uint32_t *sample, const uint32_t *group, const uint64_t *weight, std::vector<uint64_t> &keys,
                std::vector<uint32_t> &starts, uint32_t *n_cells_out) {
  const uint32_t n32 = (uint32_t)n;
  size_t cub_bytes = 0;
  int rc;
  if ((rc = sort_pairs_bytes<uint32_t>(n, 64, &cub_bytes)) || (rc = exclusive_sum_bytes<uint32_t>(n + 1, &cub_bytes)) ||
      (rc = run_heads_bytes(n, &cub_bytes))) return rc;
  Pool P;
  uint32_t *d_sample, *d_group, *d_idx[2], *d_mark, *d_head, *d_flag, *d_slot, *d_kept, *d_list;
  uint64_t *d_weight, *d_key[2];
  unsigned long long *d_sum;
  uint8_t *d_cub;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_sample, n); P.get(&d_group, n); P.get(&d_weight, n); P.get(&d_key[0], n); P.get(&d_key[1], n); P.get(&d_idx[0], n);
    P.get(&d_idx[1], n); P.get(&d_mark, n); P.get(&d_head, n); P.get(&d_flag, n + 1); P.get(&d_slot, n + 1); P.get(&d_kept, 2);
    P.get(&d_list, n); P.get(&d_sum, n); P.get(&d_cub, cub_bytes);
    if (pass == 0 && (rc = P.allocate())) return rc;
  }
  if ((rc = to_device(d_sample, sample, n)) || (rc = to_device(d_group, group, n)) || (rc = to_device(d_weight, weight, n))) return rc;
  const Scratch cub{d_cub, cub_bytes};

  // cells: the items sorted (stably) by (sample, group); a run is a cell
  classes_cell_keys_kernel<<<grid_for(n), BLOCK>>>(d_sample, d_group, n32, d_key[0], d_idx[0]);
  HIP_TRY(hipGetLastError());
  if ((rc = sort_pairs(cub, d_key[0], d_key[1], d_idx[0], d_idx[1], n, 32 + (int)dcrx_ovl::SAMPLE_BITS, nullptr))) return rc;
  HIP_TRY(hipMemsetAsync(d_kept, 0, 2 * sizeof *d_kept, nullptr));
  if ((rc = cell_sums(cub, d_key[1], d_idx[1], d_weight, n32, d_mark, d_head, d_sum, d_flag, nullptr))) return rc;
  classes_cell_flags_kernel<<<grid_for(n), BLOCK>>>(d_head, d_sum, n32, d_flag);
  HIP_TRY(hipGetLastError());
  if ((rc = compact(cub, d_flag, d_slot, n32, PutClassKey{d_key[1], d_sum, d_key[0], d_idx[0], d_kept + 1}, d_kept, nullptr))) return rc;
  uint32_t kept[2] = {0, 0};      // the number of cells, and with it the flag of a cell that passed 2^32
  if ((rc = to_host(kept, d_kept, 2))) return rc;
  if (kept[1]) return set_err(DCRX_E_UNSUPPORTED, "dcrx_abundance_classes: a cell's weight (the sum of one sample's items of one group) is 2^32 or more");
  const uint32_t n_cells = kept[0];
  *n_cells_out = n_cells;
  keys.clear(); starts.clear();
  if (!n_cells) return DCRX_OK;

  // classes: the cells sorted by (sample, weight); a run is a class, and its head's position tells where it starts
  if ((rc = sort_pairs(cub, d_key[0], d_key[1], d_idx[0], d_idx[1], n_cells, 32 + (int)dcrx_ovl::SAMPLE_BITS, nullptr))) return rc;
  if ((rc = run_marks(d_key[1], n_cells, d_mark, nullptr)) || (rc = run_heads(cub, d_mark, d_head, n_cells, nullptr))) return rc;
  classes_head_flags_kernel<<<grid_for(n_cells), BLOCK>>>(d_head, n_cells, d_flag);
  HIP_TRY(hipGetLastError());
  if ((rc = compact(cub, d_flag, d_slot, n_cells, PutIndex{d_list}, d_kept, nullptr))) return rc;
  uint32_t n_classes = 0;
  if ((rc = to_host(&n_classes, d_kept, 1))) return rc;
  starts.resize(n_classes);
  keys.resize(n_classes);
  if ((rc = to_host(starts.data(), d_list, n_classes)) || (rc = gather(d_key[1], d_list, n_classes, 0, d_key[0], nullptr))) return rc;
  return to_host(keys.data(), d_key[0], n_classes);
}

int check_device_args(const char *who, uint32_t S, uint64_t m) {
  static thread_local char msg[160];
  if (S < 1 || S > MAX_SAMPLES) {
    std::snprintf(msg, sizeof msg, "%s: 1 .. DCRX_DOWNSAMPLE_MAX_SAMPLES (4096) samples", who);
    return set_err(DCRX_E_INVALID, msg);
  }
  if (m >= MAX_ROWS) {
    std::snprintf(msg, sizeof msg, "%s: 2^30 or more rows", who);
    return set_err(DCRX_E_UNSUPPORTED, msg);
  }
  return DCRX_OK;
}

}  // namespace

extern "C" {

uint64_t dcrx_downsample_work_bytes(uint64_t m, uint32_t n_samples) {
  Pool P;
  Work W;
  if (n_samples < 1 || n_samples > MAX_SAMPLES || m >= MAX_ROWS || W.carve(P, m, n_samples) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_downsample_device(uint32_t n_samples, uint64_t m, const uint32_t *d_sample, const uint64_t *d_weight, const uint64_t *d_depth,
                           uint64_t seed, uint64_t *d_kept, uint64_t *d_reads, uint64_t *d_depth_used, uint64_t *d_threshold, void *d_work,
                           uint64_t work_bytes, void *hip_stream) {
  int rc;
  if ((rc = check_device_args("dcrx_downsample_device", n_samples, m))) return rc;
  if (!d_depth || !d_reads || !d_depth_used || !d_threshold || !d_work || (m && (!d_sample || !d_weight || !d_kept)))
    return set_err(DCRX_E_INVALID, "dcrx_downsample_device: null argument");
  Pool P(d_work);
  Work W;
  if ((rc = W.carve(P, m, n_samples))) return rc;
  if (work_bytes < P.bytes()) return set_err(DCRX_E_INVALID, "dcrx_downsample_device: the work space is smaller than dcrx_downsample_work_bytes(m, n_samples)");
  return run_downsample(n_samples, m, d_sample, d_weight, d_depth, seed, d_kept, d_reads, d_depth_used, d_threshold, W,
                        (hipStream_t)hip_stream);
}

int dcrx_downsample(uint32_t n_samples, uint64_t m, const uint32_t *sample, const uint64_t *weight, const uint64_t *depth, uint64_t seed,
                    uint64_t *kept_out, uint64_t *reads_out, uint64_t *depth_used_out, uint64_t *threshold_out) {
  int rc;
  if ((rc = check_device_args("dcrx_downsample", n_samples, m))) return rc;
  if (!depth || !reads_out || !depth_used_out || !threshold_out || (m && (!sample || !weight || !kept_out)))
    return set_err(DCRX_E_INVALID, "dcrx_downsample: null argument");
  const uint32_t S = n_samples;
  uint64_t total = 0;
  for (uint64_t k = 0; k < m; k++) {
    if (sample[k] >= S) return set_err(DCRX_E_INVALID, "dcrx_downsample: a sample id outside 0 .. n_samples - 1");
    if (k && sample[k] < sample[k - 1]) return set_err(DCRX_E_INVALID, "dcrx_downsample: the sample ids go down (the rows come sample by sample)");
    if (weight[k] >= MAX_READS || (total += weight[k]) >= MAX_READS)
      return set_err(DCRX_E_UNSUPPORTED, "dcrx_downsample: 2^40 reads or more in all");
  }
  if (!m) {
    for (uint32_t s = 0; s < S; s++) { reads_out[s] = 0; depth_used_out[s] = 0; threshold_out[s] = ~0ull; }
    return DCRX_OK;
  }
  Pool P;
  Work W;
  uint32_t *d_sample;
  uint64_t *d_weight, *d_depth, *d_kept, *d_reads, *d_used, *d_thr;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_sample, m); P.get(&d_weight, m); P.get(&d_depth, S); P.get(&d_kept, m); P.get(&d_reads, S); P.get(&d_used, S);
    P.get(&d_thr, S);
    if ((rc = W.carve(P, m, S)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = to_device(d_sample, sample, m)) || (rc = to_device(d_weight, weight, m)) || (rc = to_device(d_depth, depth, S)) ||
      (rc = run_downsample(S, m, d_sample, d_weight, d_depth, seed, d_kept, d_reads, d_used, d_thr, W, nullptr)) ||
      (rc = to_host(kept_out, d_kept, m)) || (rc = to_host(reads_out, d_reads, S)) || (rc = to_host(depth_used_out, d_used, S)))
    return rc;
  return to_host(threshold_out, d_thr, S);
}

int64_t dcrx_abundance_classes(uint32_t n_samples, uint64_t n, const uint32_t *sample, const uint32_t *group, const uint64_t *weight,
                               uint64_t *class_off_out, uint32_t *class_count_out, uint64_t *class_mult_out) {
  const uint32_t S = n_samples;
  if (S < 1 || S > dcrx_ovl::MAX_SAMPLES) return set_err(DCRX_E_INVALID, "dcrx_abundance_classes: 1 .. DCRX_OVERLAP_MAX_SAMPLES (64) samples");
  if (n >= MAX_ITEMS) return set_err(DCRX_E_UNSUPPORTED, "dcrx_abundance_classes: 2^30 or more items");
  if (!class_off_out || (n && (!sample || !group || !weight || !class_count_out || !class_mult_out)))
    return set_err(DCRX_E_INVALID, "dcrx_abundance_classes: null argument");
  for (uint64_t k = 0; k < n; k++) {
    if (sample[k] >= S) return set_err(DCRX_E_INVALID, "dcrx_abundance_classes: a sample id outside 0 .. n_samples - 1");
    if (weight[k] >= MAX_WEIGHT) return set_err(DCRX_E_UNSUPPORTED, "dcrx_abundance_classes: an item's weight is 2^32 or more");
  }
  for (uint32_t s = 0; s <= S; s++) class_off_out[s] = 0;
  if (!n) return 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> starts;
  uint32_t n_cells = 0;
  int rc;
  try {
    rc = run_classes(S, n, sample, group, weight, keys, starts, &n_cells);
  } catch (const std::exception &e) {
    rc = set_err(DCRX_E_NOMEM, e.what());
  }
  if (rc) return rc;
  const size_t C = keys.size();
  for (size_t c = 0; c < C; c++) {
    class_count_out[c] = (uint32_t)keys[c];
    class_mult_out[c] = (c + 1 < C ? starts[c + 1] : n_cells) - starts[c];
    class_off_out[(keys[c] >> 32) + 1]++;
  }
  for (uint32_t s = 0; s < S; s++) class_off_out[s + 1] += class_off_out[s];
  return (int64_t)C;
}

}  // extern "C"

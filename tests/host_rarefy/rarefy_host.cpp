// Test-only: the downsampling step's shared code (dcrx_rarefy_core.h) built by g++, for a check against Python on the host, and
// the primitive's steps (dcrx_rarefy.hip) written serially around the look-ups and digit steps the kernels' lanes make.
#include <algorithm>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_rarefy_core.h"

using namespace dcrx_rar;

namespace {

constexpr uint32_t NO_SAMPLE = 0xFFFFFFFFu, NO_ROW = 0xFFFFFFFFu;

struct Walk {
  uint32_t S, m, grid;
  const uint32_t *sample;
  std::vector<uint64_t> G, base, s_seed;
  uint64_t total;

  // rarefy_walk_kernel's walk: per block its tiles; per tile the first row and the staged ends (a heap block of SLOTS entries and
  // no more); per wave of 64 lanes and per j the rows and samples of the lanes' reads.  on_tile(block, s0) before a tile's
  // reads; on_wave(rows, samples, reads) with NO_ROW / NO_SAMPLE where a lane has no read.
  template <class OnTile, class OnWave> void run(OnTile on_tile, OnWave on_wave) const {
    for (uint32_t block = 0; block < grid; block++) {
      uint32_t tile, tile_end;
      block_tiles(total, block, grid, &tile, &tile_end);
      for (; tile < tile_end; tile++) {
        const uint64_t g0 = (uint64_t)tile * TILE, g_end = min_u64(g0 + TILE, total);
        const uint32_t i0 = first_above(G.data(), 0, m, g0) - 1;
        on_tile(block, sample[i0]);
        std::vector<uint64_t> ends(SLOTS);
        for (uint32_t k = 0; k < SLOTS; k++) ends[k] = G.at(min_u32(i0 + 1 + k, m));
        const bool one_row = ends[0] >= g_end;
        for (uint32_t wave = 0; wave < LANES / 64; wave++)
          for (uint32_t j = 0; j < PER_LANE; j++) {
            uint32_t rows[64], smp[64];
            uint64_t reads[64];
            for (uint32_t lane = 0; lane < 64; lane++) {
              const uint64_t g = g0 + (uint64_t)j * LANES + wave * 64 + lane;
              rows[lane] = NO_ROW; smp[lane] = NO_SAMPLE; reads[lane] = g;
              if (g >= g_end) continue;
              rows[lane] = one_row ? i0 : row_of(ends.data(), SLOTS, G.data(), i0, m, g);
              smp[lane] = sample[rows[lane]] < S ? sample[rows[lane]] : NO_SAMPLE;
            }
            on_wave(rows, smp, reads);
          }
      }
    }
  }
};

}  // namespace

extern "C" {
uint32_t rarefy_host_tile(void) { return TILE; }
uint32_t rarefy_host_slots(void) { return SLOTS; }
uint32_t rarefy_host_bins(void) { return BINS; }
uint32_t rarefy_host_grid(void) { return GRID; }
uint32_t rarefy_host_levels(void) { return LEVELS; }
uint32_t rarefy_host_candidates(void) { return CANDIDATES; }
uint32_t rarefy_host_max_samples(void) { return MAX_SAMPLES; }
uint64_t rarefy_host_fin(uint64_t z) { return fin(z); }
uint64_t rarefy_host_key(uint64_t seed, uint64_t s, uint64_t r) { return key(seed, s, r); }
uint32_t rarefy_host_digit(uint64_t k, uint32_t level) { return digit(k, level); }
uint64_t rarefy_host_prefix(uint64_t k, uint32_t levels) { return prefix_of(k, levels); }
uint32_t rarefy_host_run_kept(uint64_t heads, uint64_t keeps, uint32_t lane) { return run_kept(heads, keeps, lane); }

// dcrx_downsample_device's steps in their plainest serial form, for `grid` blocks: the offsets, the samples, the levels of
// histograms (a block's histogram for the sample of its tiles, everything else straight onto the sample's) and bins, the
// candidates, the thresholds, and the count pass with a wave's runs of lanes in one row.  Every buffer has the kernels' size
// and no more.  levels_out (S entries, may be null): the levels a sample's selection took.  0, or -1 on arguments the launch
// never makes.
int rarefy_host_downsample(uint32_t S, uint32_t m, const uint32_t *sample, const uint64_t *weight, const uint64_t *depth, uint64_t seed,
                           uint32_t grid, uint64_t *kept, uint64_t *reads, uint64_t *depth_used, uint64_t *threshold, uint32_t *levels_out) {
  if (S < 1 || S > MAX_SAMPLES || !grid || grid > GRID || m >= MAX_ROWS) return -1;
  Walk W;
  W.S = S; W.m = m; W.grid = grid; W.sample = sample;
  W.G.assign((size_t)m + 1, 0);
  for (uint32_t i = 0; i < m; i++) W.G[i + 1] = W.G[i] + weight[i];
  const uint64_t sum = W.G[m];
  const bool fits = sum < MAX_READS;
  W.total = fits ? sum : 0;
  W.base.assign((size_t)S + 1, sum);
  W.s_seed.assign(S, 0);
  std::vector<uint64_t> rank(S), prefix(S, 0);
  std::vector<uint32_t> levels(S, 0), active(S, 0), all(S, 0);
  for (uint32_t s = 0; s < S; s++) {
    const uint32_t lo = first_row_of(sample, m, s), hi = first_row_of(sample, m, s + 1);
    const uint64_t b0 = W.G.at(lo), b1 = W.G.at(hi), X = b1 - b0, n = fits ? min_u64(depth[s], X) : 0;
    reads[s] = X; depth_used[s] = n; W.base[s] = b0; W.s_seed[s] = sample_seed(seed, s); rank[s] = n;
    all[s] = fits && n == X;
    active[s] = fits && !all[s];
    threshold[s] = all[s] ? ~0ull : 0;
  }
  for (uint32_t i = 0; i < m; i++) kept[i] = 0;
  if (!m) return 0;
  std::vector<uint64_t> hist((size_t)S * BINS, 0);
  for (uint32_t level = 0; level < LEVELS; level++) {
    if (!std::count(active.begin(), active.end(), 1u)) break;
    std::vector<uint32_t> lh(BINS, 0);
    uint32_t cur = NO_SAMPLE, cur_block = 0;
    auto flush = [&]() {
      for (uint32_t k = 0; k < BINS; k++) {
        if (cur < S) hist.at((size_t)cur * BINS + k) += lh[k];
        lh[k] = 0;
      }
    };
    W.run(
        [&](uint32_t block, uint32_t s0) {
          if (block != cur_block) { flush(); cur = NO_SAMPLE; cur_block = block; }
          if (s0 != cur) { flush(); cur = s0; }
        },
        [&](const uint32_t *rows, const uint32_t *smp, const uint64_t *g) {
          for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t s = smp[lane];
            if (s == NO_SAMPLE || !active[s]) continue;
            const uint64_t k = key_of(W.s_seed[s], g[lane] - W.base[s]);
            if (prefix_of(k, level) != prefix[s]) continue;
            if (s == cur) lh.at(digit(k, level))++;
            else hist.at((size_t)s * BINS + digit(k, level))++;
          }
        });
    flush();
    for (uint32_t s = 0; s < S; s++) {
      if (!active[s]) continue;
      uint64_t *h = &hist[(size_t)s * BINS], below = 0;
      uint32_t b = 0;
      while (b < BINS && rank[s] >= below + h[b]) below += h[b++];
      if (b == BINS) return -1;
      rank[s] -= below;
      prefix[s] = (prefix[s] << BIN_BITS) | b;
      levels[s] = level + 1;
      if (h[b] <= CANDIDATES || level + 1 == LEVELS) active[s] = 0;
      std::fill(h, h + BINS, 0);
    }
  }
  std::vector<uint64_t> cand((size_t)S * CANDIDATES);
  std::vector<uint32_t> cand_n(S, 0);
  W.run([](uint32_t, uint32_t) {},
        [&](const uint32_t *rows, const uint32_t *smp, const uint64_t *g) {
          for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t s = smp[lane];
            if (s == NO_SAMPLE || !levels[s]) continue;
            const uint64_t k = key_of(W.s_seed[s], g[lane] - W.base[s]);
            if (prefix_of(k, levels[s]) == prefix[s]) cand.at((size_t)s * CANDIDATES + cand_n[s]++) = k;
          }
        });
  for (uint32_t s = 0; s < S; s++) {
    if (levels_out) levels_out[s] = levels[s];
    if (!levels[s]) continue;
    const uint64_t *keys = &cand[(size_t)s * CANDIDATES];
    for (uint32_t k = 0; k < cand_n[s]; k++) {
      uint32_t smaller = 0;
      for (uint32_t q = 0; q < cand_n[s]; q++) smaller += keys[q] < keys[k];
      if (smaller == rank[s]) threshold[s] = keys[k];
    }
  }
  W.run([](uint32_t, uint32_t) {},
        [&](const uint32_t *rows, const uint32_t *smp, const uint64_t *g) {
          uint64_t heads = 0, keeps = 0;
          for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t s = smp[lane];
            if (lane == 0 || rows[lane - 1] != rows[lane]) heads |= 1ull << lane;
            if (s != NO_SAMPLE && (all[s] || key_of(W.s_seed[s], g[lane] - W.base[s]) < threshold[s])) keeps |= 1ull << lane;
          }
          for (uint32_t lane = 0; lane < 64; lane++)
            if ((heads >> lane & 1) && rows[lane] != NO_ROW) kept[rows[lane]] += run_kept(heads, keeps, lane);
        });
  return 0;
}
}

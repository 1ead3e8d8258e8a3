// dcrx_umi.hip — the UMI neighbour search of `collapse` (reference src/decombinator/collapse.py:723-751, make_merge_groups:
// pyrepseq.nn.symdel, then the upper triangle in (i, j) order): every pair of UMIs within Levenshtein distance k.
//
// Host side (dcrx_umi_encode): each UMI becomes a record (dcrx_umi_core.h) and the records are sorted by (length,
// composition), so that UMIs that can be close sit in nearby tiles; each tile of DCRX_UMI_TILE records gets a summary (the
// range of its lengths and of each symbol count).
// Device side (umi_pairs_kernel): one block per row tile, one UMI per lane (its symbols, length and composition in
// registers).  The block walks the column tiles from its own to the last; a column tile whose summary is out of reach
// (length ranges more than k apart, or composition ranges more than 2k apart in L1) is skipped whole, otherwise its records
// are staged in LDS and every lane takes each of them in turn: two lower bounds first (length, one v_sad_u8 per four
// symbol counts), the exact Myers check only for what survives.  Hits leave by a ballot: one vector atomic per wave and
// partner, the lanes' slots by mbcnt.  Pairs come out as (min index << 32 | max index) keys of the caller's indices.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_hip.h"
#include "dcrx_umi_core.h"

using namespace dcrx;
using namespace dcrx_umi;

namespace {

constexpr int TILE = DCRX_UMI_TILE;
constexpr int RW = DCRX_UMI_REC_WORDS;
static_assert(RW == 16, "a record is four 16-byte loads");
static_assert(UMI_MAX_LEN == DCRX_UMI_MAX_LEN, "clamp_k clamps to the longest UMI");

__global__ __launch_bounds__(TILE) void umi_pairs_kernel(const uint32_t *__restrict__ recs, const uint32_t *__restrict__ tiles,
                                                         uint32_t n_tiles, int32_t k, unsigned long long *__restrict__ pairs,
                                                         unsigned long long cap, unsigned long long *__restrict__ total) {
  __shared__ uint4 lds[TILE * RW / 4];
  const uint32_t rt = blockIdx.x;
  const uint32_t lane_rec = rt * TILE + threadIdx.x;
  const uint32_t row_count = tiles[rt * DCRX_UMI_TILE_WORDS + 6];
  const bool active = threadIdx.x < row_count;
  const uint4 own_codes = reinterpret_cast<const uint4 *>(recs + (size_t)lane_rec * RW)[2];     // words 8..11
  const uint4 own_rest = reinterpret_cast<const uint4 *>(recs + (size_t)lane_rec * RW)[3];      // words 12..15
  const uint32_t own_len = own_codes.w, own_c0 = own_rest.x, own_c1 = own_rest.y, own_idx = own_rest.z;
  const uint32_t *rtile = tiles + rt * DCRX_UMI_TILE_WORDS;
  const uint32_t lane = __lane_id();

  for (uint32_t ct = rt; ct < n_tiles; ct++) {
    const uint32_t *ctile = tiles + ct * DCRX_UMI_TILE_WORDS;
    if (!tiles_may_match(rtile, ctile, k)) continue;                          // uniform across the block
    const uint32_t col_count = ctile[6];
    __syncthreads();                                                          // the previous tile is no longer read
    const uint4 *src = reinterpret_cast<const uint4 *>(recs + (size_t)ct * TILE * RW);
#pragma unroll
    for (int q = 0; q < RW / 4; q++) lds[q * TILE + threadIdx.x] = src[q * TILE + threadIdx.x];
    __syncthreads();
    const uint32_t *l32 = reinterpret_cast<const uint32_t *>(lds);
    const uint32_t first = ct == rt ? threadIdx.x + 1 : 0;                   // upper triangle: partners after this lane
    // every lane runs the same partner sequence (the ballot needs the whole wave): start at the wave's smallest `first`
    const uint32_t wave_first = ct == rt ? (threadIdx.x & ~63u) + 1 : 0;
    for (uint32_t p = wave_first; p < col_count; p++) {
      const uint32_t *b = l32 + p * RW;                                        // LDS record of partner p (same for all lanes)
      bool hit = false;
      uint32_t b_idx = 0;
      if (active && p >= first && may_match(own_len, own_c0, own_c1, b[W_LEN], b[W_COMP], b[W_COMP + 1], k)) {
        hit = myers(b + W_PEQ, b[W_LEN], own_codes.x, own_codes.y, own_codes.z, own_len, k) <= k;
        b_idx = b[W_INDEX];
      }
      const unsigned long long m = __ballot(hit);
      if (m) {
        const uint32_t leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(total, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (hit) {
          const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
          const unsigned long long slot = base + below;
          if (slot < cap) {
            const uint32_t lo = min(own_idx, b_idx), hi = max(own_idx, b_idx);
            pairs[slot] = ((unsigned long long)lo << 32) | hi;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int64_t dcrx_umi_encode(const char *ascii, const uint64_t *offsets, uint64_t n, uint32_t *recs, uint32_t *tiles) {
  if (n && (!ascii || !offsets)) return set_err(DCRX_E_INVALID, "dcrx_umi_encode: null argument");
  if (n > 0xffffffffull - TILE) return set_err(DCRX_E_UNSUPPORTED, "dcrx_umi_encode: more than 2^32 - 257 UMIs");
  const uint64_t n_tiles = (n + TILE - 1) / TILE;
  int16_t code_of[256];
  for (int c = 0; c < 256; c++) code_of[c] = -1;
  int n_sym = 0;
  // limits and symbols first: an unsupported list is refused before anything is written
  for (uint64_t u = 0; u < n; u++) {
    if (offsets[u + 1] < offsets[u]) return set_err(DCRX_E_INVALID, "dcrx_umi_encode: offsets go backwards");
    const uint64_t len = offsets[u + 1] - offsets[u];
    if (len > DCRX_UMI_MAX_LEN) {
      const std::string m = "UMI " + std::to_string(u) + " is " + std::to_string(len) + " bytes long: the UMI neighbour search takes at most " +
                            std::to_string(DCRX_UMI_MAX_LEN);
      return set_err(DCRX_E_UNSUPPORTED, m.c_str());
    }
    for (uint64_t p = offsets[u]; p < offsets[u + 1]; p++) {
      const uint8_t c = (uint8_t)ascii[p];
      if (code_of[c] < 0) {
        if (n_sym == DCRX_UMI_MAX_SYMBOLS) {
          const std::string m = "the UMIs hold more than " + std::to_string(DCRX_UMI_MAX_SYMBOLS) +
                                " distinct byte values (the UMI neighbour search takes at most that many in one call)";
          return set_err(DCRX_E_UNSUPPORTED, m.c_str());
        }
        code_of[c] = (int16_t)n_sym++;
      }
    }
  }
  if (!recs) return (int64_t)n_tiles;
  if (!tiles) return set_err(DCRX_E_INVALID, "dcrx_umi_encode: tiles is null");
  try {
    std::vector<uint32_t> rec((size_t)n * RW, 0u);
    std::vector<std::pair<uint64_t, uint32_t>> order((size_t)n);
    for (uint64_t u = 0; u < n; u++) {
      uint32_t *r = rec.data() + u * RW;
      uint8_t comp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      const uint32_t len = (uint32_t)(offsets[u + 1] - offsets[u]);
      for (uint32_t p = 0; p < len; p++) {
        const uint32_t s = (uint32_t)code_of[(uint8_t)ascii[offsets[u] + p]];
        r[W_PEQ + s] |= 1u << p;
        r[W_CODES + p / 8] |= s << ((p % 8) * 4);
        comp[s]++;
      }
      r[W_LEN] = len;
      std::memcpy(r + W_COMP, comp, 8);
      r[W_INDEX] = (uint32_t)u;
      uint64_t key = (uint64_t)len << 40;                                       // length, then the counts (5 bits each)
      for (int s = 0; s < 8; s++) key |= (uint64_t)comp[s] << (35 - 5 * s);
      order[u] = {key, (uint32_t)u};
    }
    std::sort(order.begin(), order.end());
    std::memset(recs, 0, (size_t)n_tiles * TILE * RW * sizeof(uint32_t));
    for (uint64_t t = 0; t < n_tiles; t++) {
      uint32_t *ts = tiles + t * DCRX_UMI_TILE_WORDS;
      uint8_t mn[9], mx[9];
      std::memset(mn, 255, sizeof mn);
      std::memset(mx, 0, sizeof mx);
      const uint64_t lo = t * TILE, hi = std::min<uint64_t>(n, lo + TILE);
      for (uint64_t s = lo; s < hi; s++) {
        const uint32_t *r = rec.data() + (size_t)order[s].second * RW;
        std::memcpy(recs + s * RW, r, RW * sizeof(uint32_t));
        uint8_t c[9];
        std::memcpy(c, r + W_COMP, 8);
        c[8] = (uint8_t)r[W_LEN];
        for (int q = 0; q < 9; q++) { mn[q] = std::min(mn[q], c[q]); mx[q] = std::max(mx[q], c[q]); }
      }
      ts[0] = mn[8]; ts[1] = mx[8];
      std::memcpy(ts + 2, mn, 8);
      std::memcpy(ts + 4, mx, 8);
      ts[6] = (uint32_t)(hi - lo);
      ts[7] = 0;
    }
  } catch (const std::bad_alloc &) {
    return set_err(DCRX_E_NOMEM, "out of memory in dcrx_umi_encode");
  }
  return (int64_t)n_tiles;
}

extern "C" int dcrx_umi_neighbours_device(const uint32_t *d_recs, const uint32_t *d_tiles, uint64_t n_tiles, int32_t k,
                                          uint64_t *d_pairs, uint64_t pair_cap, uint64_t *d_total, void *hip_stream) {
  if (k < 0) return set_err(DCRX_E_INVALID, "dcrx_umi_neighbours_device: k < 0");
  k = clamp_k(k);                                                             // the same pairs, and 2 * k stays an int32
  if (!d_total || (n_tiles && (!d_recs || !d_tiles)) || (pair_cap && !d_pairs))
    return set_err(DCRX_E_INVALID, "dcrx_umi_neighbours_device: null argument");
  if (n_tiles > 0xffffffffull / TILE) return set_err(DCRX_E_UNSUPPORTED, "dcrx_umi_neighbours_device: too many tiles");
  hipStream_t s = (hipStream_t)hip_stream;
  hipError_t e = hipMemsetAsync(d_total, 0, sizeof(uint64_t), s);
  if (e == hipSuccess && n_tiles) {
    hipLaunchKernelGGL(umi_pairs_kernel, dim3((uint32_t)n_tiles), dim3(TILE), 0, s, d_recs, d_tiles, (uint32_t)n_tiles, k,
                       (unsigned long long *)d_pairs, (unsigned long long)pair_cap, (unsigned long long *)d_total);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return hip_fail(e, "dcrx_umi_neighbours_device");
  return DCRX_OK;
}

extern "C" int64_t dcrx_umi_neighbours(const char *ascii, const uint64_t *offsets, uint64_t n, int32_t k, uint64_t *pairs,
                                       uint64_t pair_cap) {
  if (k < 0) return set_err(DCRX_E_INVALID, "dcrx_umi_neighbours: k < 0");
  k = clamp_k(k);
  if (pair_cap && !pairs) return set_err(DCRX_E_INVALID, "dcrx_umi_neighbours: pairs is null");
  const int64_t n_tiles = dcrx_umi_encode(ascii, offsets, n, nullptr, nullptr);
  if (n_tiles < 0) return n_tiles;
  if (n < 2) return 0;
  std::vector<uint32_t> recs, tiles;
  try {
    recs.resize((size_t)n_tiles * TILE * RW);
    tiles.resize((size_t)n_tiles * DCRX_UMI_TILE_WORDS);
  } catch (const std::bad_alloc &) {
    return set_err(DCRX_E_NOMEM, "out of memory in dcrx_umi_neighbours");
  }
  const int64_t rc = dcrx_umi_encode(ascii, offsets, n, recs.data(), tiles.data());
  if (rc < 0) return rc;
  DevBuf<uint32_t> d_recs, d_tiles;
  DevBuf<uint64_t> d_pairs, d_total;
  uint64_t total = 0;
  int ret;
  if ((ret = d_recs.alloc(recs.size())) || (ret = d_tiles.alloc(tiles.size())) || (ret = d_total.alloc(1)) ||
      (pair_cap && (ret = d_pairs.alloc(pair_cap)))) return ret;
  HIP_TRY(hipMemcpy(d_recs, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_tiles, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice));
  ret = dcrx_umi_neighbours_device(d_recs, d_tiles, (uint64_t)n_tiles, k, d_pairs, pair_cap, d_total, nullptr);
  if (ret != DCRX_OK) return ret;
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(&total, d_total, 8, hipMemcpyDeviceToHost));
  if (total <= pair_cap && total) HIP_TRY(hipMemcpy(pairs, d_pairs, total * 8, hipMemcpyDeviceToHost));
  if (total <= pair_cap) std::sort(pairs, pairs + total);
  return (int64_t)total;
}

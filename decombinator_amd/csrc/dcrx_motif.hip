// dcrx_motif.hip — the motif step (`motifs`): which 2-, 3- and 4-mers of the middle of a sample's CDR3s occur in more of them
// than in as many CDR3s drawn from a background; include/dcrx.h "motifs" holds the contract, dcrx_motif_core.h the per-unit
// code, the selection's digits and the chunk rule.
//
// The primitive (dcrx_cdr3_motifs_device), on the caller's stream, nothing copied back:
//   pack       motif_pack_kernel, a lane per unit: the packed string, its length (0: it takes no part), the statistics
//   tables     motif_table_kernel, a lane per unit: one onto cs[motif] (cb[motif]) per motif of the unit, in a table over all
//              MOTIFS motifs — the motif's number is its place in motif order, so no sort is needed
//   report     flags (cs >= min_count), dcrx_group.h's ordered compaction: the reported rows and every motif's row + 1
//   per chunk of resamples:
//     select   motif_select_kernel, a block per resample: histogram selection of the (n' + 1)-th smallest key over 8-bit
//              digits, the bin's keys written out, the threshold; then the indices of the n' kept units into the resample's list
//     count    motif_count_kernel, a lane per kept unit of the chunk: one per motif of the unit onto plane[resample][row]
//     fold     motif_fold_kernel, a lane per reported row: ge, sum, max over the chunk's resamples
//   finish     need and the statistics
// A resample's work is n' units, not the background's m': the kept units are listed first and only they are looked at.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/dcrx.h"
#include "dcrx_group.h"
#include "dcrx_motif_core.h"

using dcrx::set_err;
using namespace dcrx_group;
using namespace dcrx_motif;

static_assert(dcrx_motif::BLOCK == (uint32_t)dcrx_group::BLOCK, "a block is dcrx_group.h's");

namespace {

constexpr uint32_t TB = dcrx_motif::BLOCK;

struct Control {
  uint32_t take[2], out_of_reach[2], not_letters[2];      // per side (0: the sample, 1: the background)
  uint32_t reported, distinct;
};

struct Settings {
  uint32_t k_mask, ntrim, ctrim, min_count, resamples;
  uint64_t seed;
};

// what of a call lies in the work space
struct Work {
  uint32_t *words[2];      // per side: WORDS dwords per unit
  uint8_t *len[2];         // per side: a unit's length, 0 where it takes no part
  uint32_t *cs, *cb;       // MOTIFS counts each
  uint32_t *flag, *slot;   // MOTIFS: reported or not, then row + 1 (0: not reported); the exclusive sum
  uint32_t *list;          // chunk x n: a resample's kept units
  uint32_t *plane;         // chunk x reported: c_r(row)
  Control *ctl;
  Scratch cub;
  uint32_t chunk;
  uint64_t plane_words;
  int carve(Pool &P, uint64_t n, uint64_t m, uint32_t resamples) {
    size_t b = 0;
    const int rc = exclusive_sum_bytes<uint32_t>(MOTIFS, &b);
    if (rc) return rc;
    chunk = std::min<uint32_t>(chunk_of(n), std::max<uint32_t>(resamples, 1));
    plane_words = (uint64_t)chunk * max_reported(n);
    P.get(&words[0], n * WORDS); P.get(&len[0], n); P.get(&words[1], m * WORDS); P.get(&len[1], m);
    P.get(&cs, MOTIFS); P.get(&cb, MOTIFS); P.get(&flag, MOTIFS); P.get(&slot, MOTIFS);
    P.get(&list, (uint64_t)chunk * n); P.get(&plane, plane_words); P.get(&ctl, 1); P.get(&cub, b);
    return DCRX_OK;
  }
};

// ---- pack: a lane per unit
__global__ __launch_bounds__(TB) void motif_pack_kernel(const uint64_t *__restrict__ off, const uint8_t *__restrict__ text, uint32_t n,
                                                        uint32_t side, uint32_t *__restrict__ words, uint8_t *__restrict__ len,
                                                        Control *__restrict__ ctl) {
  const uint32_t i = blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint64_t at = off[i], L = off[i + 1] - at;
  const bool reach = dcrx_cdr3net::in_reach(L);
  uint32_t w[WORDS];
  dcrx_cdr3net::pack(text + (reach ? at : 0), L, w);
  const bool ok = takes_part(w, L);
#pragma unroll
  for (uint32_t k = 0; k < WORDS; k++) words[(uint64_t)i * WORDS + k] = w[k];
  len[i] = ok ? (uint8_t)L : (uint8_t)0;
  // one add per wave and counter (the lanes of a wave that are here hold consecutive units: its first lane is among them)
  const uint64_t oks = __ballot(ok), far = __ballot(!reach), odd = __ballot(reach && !ok);
  if ((threadIdx.x & 63u) == 0) {
    if (oks) atomicAdd(&ctl->take[side], (uint32_t)__popcll(oks));
    if (far) atomicAdd(&ctl->out_of_reach[side], (uint32_t)__popcll(far));
    if (odd) atomicAdd(&ctl->not_letters[side], (uint32_t)__popcll(odd));
  }
}

// a lane's unit into its column of the block's LDS, and f(motif number) per motif of the unit (no barrier: a lane reads its own column)
template <class F>
__device__ __forceinline__ void lane_motifs(const uint32_t *__restrict__ words, uint32_t unit, uint32_t L, const Settings &S,
                                            uint32_t (*str)[TB], uint32_t (*codes)[TB], F f) {
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < WORDS; k++) str[k][t] = words[(uint64_t)unit * WORDS + k];
  for (uint32_t k = K_MIN; k <= K_MAX; k++)
    if (S.k_mask >> k & 1u) unit_motifs(&str[0][t], TB, L, S.ntrim, S.ctrim, k, &codes[0][t], TB, f);
}

// ---- tables: one onto table[motif] per motif of a unit that takes part
__global__ __launch_bounds__(TB) void motif_table_kernel(const uint32_t *__restrict__ words, const uint8_t *__restrict__ len, uint32_t n,
                                                         Settings S, uint32_t *__restrict__ table) {
  __shared__ uint32_t str[WORDS][TB];
  __shared__ uint32_t codes[MAX_WINDOWS][TB];
  const uint32_t i = blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t L = len[i];
  if (!L) return;
  lane_motifs(words, i, L, S, str, codes, [&](uint32_t id) { atomicAdd(&table[id], 1u); });
}

// ---- report
__global__ __launch_bounds__(TB) void motif_flags_kernel(const uint32_t *__restrict__ cs, uint32_t min_count, uint32_t *__restrict__ flag,
                                                         Control *__restrict__ ctl) {
  const uint32_t id = blockIdx.x * TB + threadIdx.x;
  if (id >= MOTIFS) return;
  const uint32_t c = cs[id];
  flag[id] = c >= min_count ? 1u : 0u;
  const uint64_t some = __ballot(c > 0);
  if ((threadIdx.x & 63u) == 0 && some) atomicAdd(&ctl->distinct, (uint32_t)__popcll(some));
}

struct PutRow {      // a reported motif's row, where the caller's arrays have room for it
  const uint32_t *cs, *cb;
  uint32_t *k, *code, *o_cs, *o_cb, *ge, *max;
  uint64_t *sum;
  uint64_t cap;
  __device__ void operator()(uint32_t row, uint32_t id) const {
    if (row >= cap) return;
    k[row] = id_k(id); code[row] = id_code(id); o_cs[row] = cs[id]; o_cb[row] = cb[id];
    ge[row] = 0; max[row] = 0; sum[row] = 0;
  }
};

// flag[id] becomes row + 1 of a reported motif, 0 of another
__global__ __launch_bounds__(TB) void motif_rows_kernel(uint32_t *__restrict__ flag, const uint32_t *__restrict__ slot) {
  const uint32_t id = blockIdx.x * TB + threadIdx.x;
  if (id < MOTIFS) flag[id] = flag[id] ? slot[id] + 1u : 0u;
}

// whether the resamples run at all: something is reported, something is drawn, and the background holds enough (the same for every lane)
__device__ __forceinline__ bool resampling(const Control *ctl) { return ctl->reported && ctl->take[0] && ctl->take[0] <= ctl->take[1]; }

// ---- select: a block per resample of the chunk
__global__ __launch_bounds__(TB) void motif_select_kernel(const uint8_t *__restrict__ len, uint32_t m, uint64_t seed, uint32_t r0,
                                                          const Control *__restrict__ ctl, uint32_t *__restrict__ list, uint32_t n) {
  __shared__ uint32_t hist[BINS];
  __shared__ uint64_t cand[CANDIDATES];
  __shared__ uint64_t s_threshold;
  __shared__ uint32_t s_count;
  if (!resampling(ctl)) return;
  const uint32_t t = threadIdx.x, n_take = ctl->take[0], m_take = ctl->take[1];
  const uint64_t r_seed = dcrx_rar::sample_seed(seed, (uint64_t)r0 + blockIdx.x);
  const bool all = n_take == m_take;
  uint64_t threshold = ~0ull;
  if (!all) {
    // every lane walks the same histogram and holds the same prefix, rank and levels
    uint64_t prefix = 0;
    uint32_t rank = n_take, levels = 0;
    for (uint32_t level = 0; level < LEVELS; level++) {
      hist[t] = 0;
      __syncthreads();
      for (uint32_t b = t; b < m; b += TB) {
        if (!len[b]) continue;
        const uint64_t k = dcrx_rar::key_of(r_seed, b);
        if (prefix_of(k, level) == prefix) atomicAdd(&hist[digit(k, level)], 1u);
      }
      __syncthreads();
      uint32_t bin = 0, below = 0;
      while (bin + 1 < BINS && rank >= below + hist[bin]) below += hist[bin++];      // (the bin of the wanted rank: rank < the keys under the prefix)
      const uint32_t held = hist[bin];
      rank -= below;
      prefix = (prefix << BIN_BITS) | bin;
      levels = level + 1;
      __syncthreads();      // the histogram is read before the next level clears it
      if (held <= CANDIDATES) break;
    }
    if (t == 0) { s_count = 0; s_threshold = ~0ull; }
    __syncthreads();
    for (uint32_t b = t; b < m; b += TB) {
      if (!len[b]) continue;
      const uint64_t k = dcrx_rar::key_of(r_seed, b);
      if (prefix_of(k, levels) == prefix) {
        const uint32_t at = atomicAdd(&s_count, 1u);
        if (at < CANDIDATES) cand[at] = k;
      }
    }
    __syncthreads();
    const uint32_t held = min(s_count, CANDIDATES);
    for (uint32_t i = t; i < held; i += TB) {
      const uint64_t mine = cand[i];
      uint32_t smaller = 0;
      for (uint32_t q = 0; q < held; q++) smaller += cand[q] < mine ? 1u : 0u;
      if (smaller == rank) s_threshold = mine;      // (keys are distinct: one lane)
    }
    __syncthreads();
    threshold = s_threshold;
  }
  if (t == 0) s_count = 0;
  __syncthreads();
  uint32_t *mine = list + (uint64_t)blockIdx.x * n;
  for (uint32_t b = t; b < m; b += TB) {
    if (!len[b] || !(all || dcrx_rar::key_of(r_seed, b) < threshold)) continue;
    const uint32_t at = atomicAdd(&s_count, 1u);      // (the list's order is of no consequence: only counts are taken from it)
    if (at < n) mine[at] = b;
  }
}

// ---- count: a lane per kept unit of the chunk
__global__ __launch_bounds__(TB) void motif_count_kernel(const uint32_t *__restrict__ words, const uint8_t *__restrict__ len, uint32_t m,
                                                         const uint32_t *__restrict__ list, uint32_t n, uint32_t chunk, Settings S,
                                                         const Control *__restrict__ ctl, const uint32_t *__restrict__ row_of,
                                                         uint32_t *__restrict__ plane) {
  __shared__ uint32_t str[WORDS][TB];
  __shared__ uint32_t codes[MAX_WINDOWS][TB];
  if (!resampling(ctl)) return;
  const uint32_t n_take = min(ctl->take[0], n), reported = ctl->reported;
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= (uint64_t)chunk * n_take) return;
  const uint32_t r = (uint32_t)(e / n_take), b = list[(uint64_t)r * n + (uint32_t)(e % n_take)];
  if (b >= m) return;      // (never: the list holds background units)
  uint32_t *row = plane + (uint64_t)r * reported;
  lane_motifs(words, b, len[b], S, str, codes, [&](uint32_t id) {
    const uint32_t at = row_of[id];
    if (at) atomicAdd(&row[at - 1], 1u);
  });
}

// ---- fold: a lane per reported row the caller has room for
__global__ __launch_bounds__(TB) void motif_fold_kernel(const uint32_t *__restrict__ plane, uint32_t chunk, const Control *__restrict__ ctl,
                                                        uint64_t cap, const uint32_t *__restrict__ cs, uint32_t *__restrict__ ge,
                                                        uint64_t *__restrict__ sum, uint32_t *__restrict__ max_c) {
  if (!resampling(ctl)) return;
  const uint32_t row = blockIdx.x * TB + threadIdx.x, reported = ctl->reported;
  if (row >= reported || row >= cap) return;
  const uint32_t want = cs[row];
  uint32_t g = 0, mx = 0;
  uint64_t s = 0;
  for (uint32_t r = 0; r < chunk; r++) {
    const uint32_t c = plane[(uint64_t)r * reported + row];
    g += c >= want ? 1u : 0u;
    s += c;
    mx = c > mx ? c : mx;
  }
  ge[row] += g;
  sum[row] += s;
  max_c[row] = mx > max_c[row] ? mx : max_c[row];
}

__global__ void motif_finish_kernel(const Control *__restrict__ ctl, uint64_t n, uint64_t m, uint64_t *__restrict__ need,
                                    dcrx_cdr3_motif_stats_t *__restrict__ st) {
  if (blockIdx.x || threadIdx.x) return;
  *need = ctl->reported;
  st->sample_units = n; st->sample_take_part = ctl->take[0]; st->sample_out_of_reach = ctl->out_of_reach[0];
  st->sample_not_letters = ctl->not_letters[0];
  st->background_units = m; st->background_take_part = ctl->take[1]; st->background_out_of_reach = ctl->out_of_reach[1];
  st->background_not_letters = ctl->not_letters[1];
  st->motifs = ctl->distinct; st->reported = ctl->reported;
}

struct Outputs {
  uint32_t *k, *code, *cs, *cb, *ge, *max;
  uint64_t *sum;
  uint64_t *need;
  dcrx_cdr3_motif_stats_t *stats;
};

int run_motifs(uint64_t n, const uint64_t *d_s_off, const char *d_s_text, uint64_t m, const uint64_t *d_b_off, const char *d_b_text,
               const Settings &S, uint64_t cap, const Outputs &O, const Work &W, hipStream_t s) {
  const uint32_t n32 = (uint32_t)n, m32 = (uint32_t)m;
  int rc;
  HIP_TRY(hipMemsetAsync(W.ctl, 0, sizeof(Control), s));
  HIP_TRY(hipMemsetAsync(W.cs, 0, MOTIFS * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(W.cb, 0, MOTIFS * sizeof(uint32_t), s));
  const uint64_t *off[2] = {d_s_off, d_b_off};
  const char *text[2] = {d_s_text, d_b_text};
  const uint32_t units[2] = {n32, m32};
  uint32_t *const table[2] = {W.cs, W.cb};
  for (uint32_t side = 0; side < 2; side++) {
    if (!units[side]) continue;
    motif_pack_kernel<<<grid_for(units[side]), TB, 0, s>>>(off[side], reinterpret_cast<const uint8_t *>(text[side]), units[side], side,
                                                           W.words[side], W.len[side], W.ctl);
    HIP_TRY(hipGetLastError());
    motif_table_kernel<<<grid_for(units[side]), TB, 0, s>>>(W.words[side], W.len[side], units[side], S, table[side]);
    HIP_TRY(hipGetLastError());
  }
  motif_flags_kernel<<<grid_for(MOTIFS), TB, 0, s>>>(W.cs, S.min_count, W.flag, W.ctl);
  HIP_TRY(hipGetLastError());
  if ((rc = compact(W.cub, W.flag, W.slot, MOTIFS, PutRow{W.cs, W.cb, O.k, O.code, O.cs, O.cb, O.ge, O.max, O.sum, cap}, &W.ctl->reported, s)))
    return rc;
  motif_rows_kernel<<<grid_for(MOTIFS), TB, 0, s>>>(W.flag, W.slot);
  HIP_TRY(hipGetLastError());
  if (n32 && m32 && cap) {
    const uint64_t rows = std::min<uint64_t>(max_reported(n), cap);
    for (uint32_t r0 = 0; r0 < S.resamples; r0 += W.chunk) {
      const uint32_t chunk = std::min(W.chunk, S.resamples - r0);
      HIP_TRY(hipMemsetAsync(W.plane, 0, (uint64_t)chunk * max_reported(n) * sizeof(uint32_t), s));
      motif_select_kernel<<<chunk, TB, 0, s>>>(W.len[1], m32, S.seed, r0, W.ctl, W.list, n32);
      HIP_TRY(hipGetLastError());
      motif_count_kernel<<<grid_for((uint64_t)chunk * n), TB, 0, s>>>(W.words[1], W.len[1], m32, W.list, n32, chunk, S, W.ctl, W.flag, W.plane);
      HIP_TRY(hipGetLastError());
      motif_fold_kernel<<<grid_for(rows), TB, 0, s>>>(W.plane, chunk, W.ctl, cap, O.cs, O.ge, O.sum, O.max);
      HIP_TRY(hipGetLastError());
    }
  }
  motif_finish_kernel<<<1, 64, 0, s>>>(W.ctl, n, m, O.need, O.stats);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

int check_args(const char *who, uint64_t n, uint64_t m, const Settings &S) {
  static thread_local char msg[200];
  const char *why = nullptr;
  if (!S.k_mask || (S.k_mask & ~K_MASK_ALL)) why = "k_mask holds bits 2, 3 and 4 alone, and one at least";
  else if (S.ntrim > MAX_TRIM || S.ctrim > MAX_TRIM) why = "a trim is 0 .. DCRX_CDR3_MOTIF_MAX_TRIM (16)";
  else if (S.min_count < 1) why = "min_count is 1 or more";
  else if (S.resamples > MAX_RESAMPLES) why = "0 .. DCRX_CDR3_MOTIF_MAX_RESAMPLES (65535) resamples";
  if (why) {
    std::snprintf(msg, sizeof msg, "%s: %s", who, why);
    return set_err(DCRX_E_INVALID, msg);
  }
  if (n >= MAX_UNITS || m >= MAX_UNITS) {
    std::snprintf(msg, sizeof msg, "%s: 2^30 or more units", who);
    return set_err(DCRX_E_UNSUPPORTED, msg);
  }
  return DCRX_OK;
}

// a side's units that take part, or -1 for offsets that go down
int64_t host_take_part(uint64_t count, const uint64_t *off, const char *text) {
  int64_t take = 0;
  for (uint64_t i = 0; i < count; i++) {
    if (off[i + 1] < off[i]) return -1;
    const uint64_t L = off[i + 1] - off[i];
    if (!dcrx_cdr3net::in_reach(L)) continue;
    uint32_t w[WORDS];
    dcrx_cdr3net::pack(reinterpret_cast<const uint8_t *>(text) + off[i], L, w);
    take += takes_part(w, L) ? 1 : 0;
  }
  return take;
}

}  // namespace

extern "C" {

uint64_t dcrx_cdr3_motifs_work_bytes(uint64_t n, uint64_t m, uint32_t resamples) {
  Pool P;
  Work W;
  if (n >= MAX_UNITS || m >= MAX_UNITS || resamples > MAX_RESAMPLES || W.carve(P, n, m, resamples) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_motifs_device(uint64_t n, const uint64_t *d_s_off, const char *d_s_text, uint64_t m, const uint64_t *d_b_off,
                            const char *d_b_text, uint32_t k_mask, uint32_t ntrim, uint32_t ctrim, uint32_t min_count,
                            uint32_t resamples, uint64_t seed, uint64_t cap, uint32_t *d_k, uint32_t *d_code, uint32_t *d_cs,
                            uint32_t *d_cb, uint32_t *d_ge, uint64_t *d_sum, uint32_t *d_max, uint64_t *d_need,
                            dcrx_cdr3_motif_stats_t *d_stats, void *d_work, uint64_t work_bytes, void *hip_stream) {
  const Settings S{k_mask, ntrim, ctrim, min_count, resamples, seed};
  int rc;
  if ((rc = check_args("dcrx_cdr3_motifs_device", n, m, S))) return rc;
  if (!d_s_off || !d_b_off || !d_need || !d_stats || !d_work || (n && !d_s_text) || (m && !d_b_text) ||
      (cap && (!d_k || !d_code || !d_cs || !d_cb || !d_ge || !d_sum || !d_max)))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motifs_device: null argument");
  if (reinterpret_cast<uintptr_t>(d_work) % ALIGN) return set_err(DCRX_E_INVALID, "dcrx_cdr3_motifs_device: the work space is not 256-byte aligned");
  Pool P(d_work);
  Work W;
  if ((rc = W.carve(P, n, m, resamples))) return rc;
  if (work_bytes < P.bytes())
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motifs_device: the work space is smaller than dcrx_cdr3_motifs_work_bytes(n, m, resamples)");
  return run_motifs(n, d_s_off, d_s_text, m, d_b_off, d_b_text, S, cap, Outputs{d_k, d_code, d_cs, d_cb, d_ge, d_max, d_sum, d_need, d_stats},
                    W, (hipStream_t)hip_stream);
}

int dcrx_cdr3_motifs(uint64_t n, const uint64_t *s_off, const char *s_text, uint64_t m, const uint64_t *b_off, const char *b_text,
                     uint32_t k_mask, uint32_t ntrim, uint32_t ctrim, uint32_t min_count, uint32_t resamples, uint64_t seed,
                     uint64_t cap, uint32_t *k_out, uint32_t *code_out, uint32_t *cs_out, uint32_t *cb_out, uint32_t *ge_out,
                     uint64_t *sum_out, uint32_t *max_out, uint64_t *need_out, dcrx_cdr3_motif_stats_t *stats_out) {
  const Settings S{k_mask, ntrim, ctrim, min_count, resamples, seed};
  int rc;
  if ((rc = check_args("dcrx_cdr3_motifs", n, m, S))) return rc;
  if (!s_off || !b_off || !need_out || !stats_out || (cap && (!k_out || !code_out || !cs_out || !cb_out || !ge_out || !sum_out || !max_out)))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motifs: null argument");
  if ((n && s_off[n] > s_off[0] && !s_text) || (m && b_off[m] > b_off[0] && !b_text))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motifs: null argument");
  const int64_t n_take = host_take_part(n, s_off, s_text), m_take = host_take_part(m, b_off, b_text);
  if (n_take < 0 || m_take < 0) return set_err(DCRX_E_INVALID, "dcrx_cdr3_motifs: the offsets go down");
  if (resamples && n_take > m_take) {
    static thread_local char msg[200];
    std::snprintf(msg, sizeof msg, "dcrx_cdr3_motifs: %lld sample units take part and only %lld background units: a resample cannot be drawn",
                  (long long)n_take, (long long)m_take);
    return set_err(DCRX_E_INVALID, msg);
  }
  const uint64_t s_bytes = s_off[n] - s_off[0], b_bytes = b_off[m] - b_off[0];
  Pool P;
  Work W;
  uint64_t *d_s_off, *d_b_off, *d_sum, *d_need;
  uint8_t *d_s_text, *d_b_text;
  uint32_t *d_k, *d_code, *d_cs, *d_cb, *d_ge, *d_max;
  dcrx_cdr3_motif_stats_t *d_stats;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_s_off, n + 1); P.get(&d_b_off, m + 1); P.get(&d_s_text, s_bytes); P.get(&d_b_text, b_bytes);
    P.get(&d_k, cap); P.get(&d_code, cap); P.get(&d_cs, cap); P.get(&d_cb, cap); P.get(&d_ge, cap); P.get(&d_max, cap); P.get(&d_sum, cap);
    P.get(&d_need, 1); P.get(&d_stats, 1);
    if ((rc = W.carve(P, n, m, resamples)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_spans(n, s_off, s_text, d_s_off, d_s_text)) || (rc = upload_spans(m, b_off, b_text, d_b_off, d_b_text)) ||
      (rc = run_motifs(n, d_s_off, reinterpret_cast<const char *>(d_s_text), m, d_b_off, reinterpret_cast<const char *>(d_b_text), S, cap,
                       Outputs{d_k, d_code, d_cs, d_cb, d_ge, d_max, d_sum, d_need, d_stats}, W, nullptr)) ||
      (rc = to_host(need_out, d_need, 1)) || (rc = to_host(stats_out, d_stats, 1))) return rc;
  const uint64_t rows = std::min<uint64_t>(*need_out, cap);
  if ((rc = to_host(k_out, d_k, rows)) || (rc = to_host(code_out, d_code, rows)) || (rc = to_host(cs_out, d_cs, rows)) ||
      (rc = to_host(cb_out, d_cb, rows)) || (rc = to_host(ge_out, d_ge, rows)) || (rc = to_host(max_out, d_max, rows))) return rc;
  return to_host(sum_out, d_sum, rows);
}

}  // extern "C"

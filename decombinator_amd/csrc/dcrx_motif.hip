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
#include "dcrx_components.h"
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


// ======== motif groups (include/dcrx.h "motif groups"): the members of the selected motifs, the groups, the host entry ========
// members   members_rows_kernel, a lane per selected motif: row_of[motif] = row + 1 in a table over all MOTIFS motifs
//           motif_pack_kernel, as above; members_walk_kernel<COUNT>, a lane per unit: its selected motifs counted (n_motifs) and
//           one onto each of their rows' counts; an exclusive sum over the rows: mem_off, need
//           with room for members: members_walk_kernel<KEEP>: a unit's postings in the rows that begin below cap; an exclusive sum
//           over the units; members_walk_kernel<WRITE>: (row, unit) pairs at the unit's place — so the pairs lie in unit order —;
//           a stable sort by row; members_put_kernel: the units of the first min(need, cap) pairs
//           The rows that begin below cap end below cap + n (a row holds n units at most): that many pairs are sorted, the unused
//           slots behind every row.
// groups    dcrx_components.h's rounds with the member rows as ROWS, its totals
// host      the two members calls around the members' allocation, the neighbour primitive around the adjacency's, the groups,
//           the census of the groups (group_marks_kernel, group_row_marks_kernel, group_census_kernel)

enum MembersPass { COUNT = 0, KEEP = 1, WRITE = 2 };

struct MembersWork {
  uint32_t *words;
  uint8_t *len;
  uint32_t *row_of;                  // MOTIFS: row + 1 of a selected motif, 0 of another
  unsigned long long *row_cnt;       // MOTIFS + 1: a row's members (the entry behind the last row stays 0)
  uint32_t *kept, *pos;              // n: a unit's postings that are written, and where they begin
  uint64_t *key[2];                  // cap + n: a posting's row
  uint32_t *val[2];                  // ... and its unit
  Control *ctl;
  Scratch cub;
  uint64_t slots;
  int carve(Pool &P, uint64_t n, uint64_t cap) {
    size_t b = 0;
    int rc;
    slots = cap ? cap + n : 0;
    if ((rc = exclusive_sum_bytes<uint64_t>(MOTIFS + 1, &b)) || (rc = exclusive_sum_bytes<uint32_t>(std::max<uint64_t>(n, 1), &b)) ||
        (slots && (rc = sort_pairs_bytes<uint32_t>(slots, MEMBER_ROW_BITS, &b)))) return rc;
    P.get(&words, n * WORDS); P.get(&len, n); P.get(&row_of, MOTIFS); P.get(&row_cnt, MOTIFS + 1); P.get(&kept, n); P.get(&pos, n);
    P.get(&key[0], slots); P.get(&key[1], slots); P.get(&val[0], slots); P.get(&val[1], slots); P.get(&ctl, 1); P.get(&cub, b);
    return DCRX_OK;
  }
};

__global__ __launch_bounds__(TB) void members_rows_kernel(const uint32_t *__restrict__ sel_k, const uint32_t *__restrict__ sel_code, uint32_t S,
                                                          uint32_t k_mask, uint32_t *__restrict__ row_of) {
  const uint32_t s = blockIdx.x * TB + threadIdx.x;
  if (s >= S) return;
  const uint32_t k = sel_k[s], code = sel_code[s];
  if (is_motif(k_mask, k, code)) row_of[motif_id(k, code)] = s + 1;      // (what is no motif of K has no row: no unit holds it)
}

// a lane per unit, over its selected motifs.  COUNT: n_motifs and the rows' counts.  KEEP: its postings in the rows that begin
// below cap.  WRITE: those postings, from pos[unit] on.
template <int PASS>
__global__ __launch_bounds__(TB) void members_walk_kernel(const uint32_t *__restrict__ words, const uint8_t *__restrict__ len, uint32_t n,
                                                          Settings S, const uint32_t *__restrict__ row_of,
                                                          unsigned long long *__restrict__ row_cnt, const uint64_t *__restrict__ mem_off,
                                                          uint64_t cap, uint32_t *__restrict__ count_out, const uint32_t *__restrict__ pos,
                                                          uint64_t *__restrict__ key, uint32_t *__restrict__ val, uint64_t slots) {
  __shared__ uint32_t str[WORDS][TB];
  __shared__ uint32_t codes[MAX_WINDOWS][TB];
  const uint32_t i = blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t L = len[i];
  uint32_t c = 0;
  uint64_t at = PASS == WRITE ? pos[i] : 0;
  if (L)
    lane_motifs(words, i, L, S, str, codes, [&](uint32_t id) {
      const uint32_t r1 = row_of[id];
      if (!r1) return;
      const uint32_t row = r1 - 1;
      if (PASS == COUNT) {
        atomicAdd(&row_cnt[row], 1ull);
        c++;
      } else if (mem_off[row] < cap) {
        if (PASS == WRITE && at < slots) { key[at] = row; val[at] = i; }
        at++;
        c++;
      }
    });
  if (PASS != WRITE) count_out[i] = c;
}

__global__ void members_need_kernel(const uint64_t *__restrict__ mem_off, uint32_t S, uint64_t *__restrict__ need) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *need = mem_off[S];
}

__global__ __launch_bounds__(TB) void members_put_kernel(const uint32_t *__restrict__ val, const uint64_t *__restrict__ mem_off, uint32_t S,
                                                         uint64_t cap, uint64_t slots, uint32_t *__restrict__ mem) {
  const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (p < cap && p < slots && p < mem_off[S]) mem[p] = val[p];
}

int run_members(uint64_t n, const uint64_t *d_off, const char *d_text, const Settings &S, uint64_t sel, const uint32_t *d_sel_k,
                const uint32_t *d_sel_code, uint64_t cap, uint32_t *d_n_motifs, uint64_t *d_mem_off, uint32_t *d_mem, uint64_t *d_need,
                const MembersWork &W, hipStream_t s) {
  const uint32_t n32 = (uint32_t)n, S32 = (uint32_t)sel;
  int rc;
  HIP_TRY(hipMemsetAsync(W.ctl, 0, sizeof(Control), s));
  HIP_TRY(hipMemsetAsync(W.row_of, 0, MOTIFS * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(W.row_cnt, 0, (MOTIFS + 1) * sizeof(unsigned long long), s));
  if (S32) {
    members_rows_kernel<<<grid_for(S32), TB, 0, s>>>(d_sel_k, d_sel_code, S32, S.k_mask, W.row_of);
    HIP_TRY(hipGetLastError());
  }
  if (n32) {
    motif_pack_kernel<<<grid_for(n32), TB, 0, s>>>(d_off, reinterpret_cast<const uint8_t *>(d_text), n32, 0, W.words, W.len, W.ctl);
    HIP_TRY(hipGetLastError());
    members_walk_kernel<COUNT><<<grid_for(n32), TB, 0, s>>>(W.words, W.len, n32, S, W.row_of, W.row_cnt, nullptr, 0, d_n_motifs, nullptr, nullptr,
                                                            nullptr, 0);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = exclusive_sum(W.cub, reinterpret_cast<const uint64_t *>(W.row_cnt), d_mem_off, (uint64_t)S32 + 1, s))) return rc;
  members_need_kernel<<<1, 64, 0, s>>>(d_mem_off, S32, d_need);
  HIP_TRY(hipGetLastError());
  if (!cap || !n32 || !S32) return DCRX_OK;
  members_walk_kernel<KEEP><<<grid_for(n32), TB, 0, s>>>(W.words, W.len, n32, S, W.row_of, nullptr, d_mem_off, cap, W.kept, nullptr, nullptr, nullptr, 0);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_sum(W.cub, W.kept, W.pos, n32, s))) return rc;
  HIP_TRY(hipMemsetAsync(W.key[0], 0xFF, W.slots * sizeof(uint64_t), s));      // (NO_MEMBER_ROW in every slot)
  members_walk_kernel<WRITE><<<grid_for(n32), TB, 0, s>>>(W.words, W.len, n32, S, W.row_of, nullptr, d_mem_off, cap, nullptr, W.pos, W.key[0],
                                                          W.val[0], W.slots);
  HIP_TRY(hipGetLastError());
  if ((rc = sort_pairs(W.cub, W.key[0], W.key[1], W.val[0], W.val[1], W.slots, MEMBER_ROW_BITS, s))) return rc;
  members_put_kernel<<<grid_for(std::min(cap, W.slots)), TB, 0, s>>>(W.val[1], d_mem_off, S32, cap, W.slots, d_mem);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

int check_members(const char *who, uint64_t n, const Settings &S, uint64_t sel, uint64_t cap) {
  int rc;
  if ((rc = check_args(who, n, 0, S))) return rc;
  static thread_local char msg[200];
  if (sel > MOTIFS) {
    std::snprintf(msg, sizeof msg, "%s: more than 475 228 selected motifs", who);
    return set_err(DCRX_E_INVALID, msg);
  }
  if (cap + n >= MAX_MEMBER_KEYS) {
    std::snprintf(msg, sizeof msg, "%s: cap + n is 2^31 or more", who);
    return set_err(DCRX_E_UNSUPPORTED, msg);
  }
  return DCRX_OK;
}

// ---- groups
struct GroupsWork {
  uint32_t *label[2], *changed, *row_label;
  dcrx_components::TotalsWork T;
  int carve(Pool &P, uint64_t n, uint64_t sel) {
    P.get(&label[0], n); P.get(&label[1], n); P.get(&changed, 1); P.get(&row_label, sel);
    return T.carve(P, n);
  }
};

__global__ void groups_count_kernel(const uint32_t *__restrict__ kept, uint32_t *__restrict__ groups) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *groups = *kept;
}

int run_groups(uint64_t n, const uint64_t *d_weight, const uint64_t *d_adj_off, const uint32_t *d_adj, uint64_t adj_entries, uint64_t sel,
               const uint64_t *d_mem_off, const uint32_t *d_mem, uint64_t mem_entries, uint32_t *d_group_of, uint32_t *d_head,
               uint32_t *d_units, uint64_t *d_weight_out, uint32_t *d_groups, uint32_t *rounds_out, const GroupsWork &W, hipStream_t s) {
  const uint32_t n32 = (uint32_t)n;
  const dcrx_components::Rows R{d_mem_off, d_mem, (uint32_t)sel, mem_entries, W.row_label};
  int rc;
  if ((rc = dcrx_components::components(n32, d_adj_off, d_adj, adj_entries != 0, &R, W.label, W.changed, rounds_out, s)) ||
      (rc = dcrx_components::totals(n32, W.label[0], d_weight, W.T, d_group_of, d_head, d_units, d_weight_out, s))) return rc;
  groups_count_kernel<<<1, 64, 0, s>>>(W.T.kept, d_groups);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// ---- the host entry's census: which groups hold a global edge, which a member row of two or more, and the counts
struct Census {
  uint32_t singletons, largest, mixed;
};

__global__ __launch_bounds__(TB) void group_marks_kernel(const uint32_t *__restrict__ degree, const uint32_t *__restrict__ group_of, uint32_t n,
                                                         uint32_t *__restrict__ has_edge) {
  const uint32_t i = blockIdx.x * TB + threadIdx.x;
  if (i < n && degree[i]) has_edge[group_of[i]] = 1u;      // (every writer writes the same word)
}

__global__ __launch_bounds__(TB) void group_row_marks_kernel(const uint64_t *__restrict__ mem_off, const uint32_t *__restrict__ mem, uint32_t S,
                                                             const uint32_t *__restrict__ group_of, uint32_t n, uint32_t *__restrict__ has_row) {
  const uint32_t r = blockIdx.x * TB + threadIdx.x;
  if (r >= S || mem_off[r + 1] - mem_off[r] < 2) return;
  const uint32_t u = mem[mem_off[r]];
  if (u < n) has_row[group_of[u]] = 1u;
}

__global__ __launch_bounds__(TB) void group_census_kernel(const uint32_t *__restrict__ units, const uint32_t *__restrict__ has_edge,
                                                          const uint32_t *__restrict__ has_row, const uint32_t *__restrict__ groups,
                                                          Census *__restrict__ out) {
  const uint32_t g = blockIdx.x * TB + threadIdx.x;
  const bool here = g < *groups;
  const uint32_t u = here ? units[g] : 0u;
  const uint64_t single = __ballot(here && u == 1), mixed = __ballot(here && has_edge[g] && has_row[g]);
  if (u) atomicMax(&out->largest, u);
  if ((threadIdx.x & 63u) == 0) {
    if (single) atomicAdd(&out->singletons, (uint32_t)__popcll(single));
    if (mixed) atomicAdd(&out->mixed, (uint32_t)__popcll(mixed));
  }
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

// ---- the motif groups' entries (include/dcrx.h "motif groups")

uint64_t dcrx_cdr3_motif_members_work_bytes(uint64_t n, uint64_t cap) {
  Pool P;
  MembersWork W;
  if (n >= MAX_UNITS || cap + n >= MAX_MEMBER_KEYS || W.carve(P, n, cap) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_motif_members_device(uint64_t n, const uint64_t *d_off, const char *d_text, uint32_t k_mask, uint32_t ntrim, uint32_t ctrim,
                                   uint64_t S, const uint32_t *d_sel_k, const uint32_t *d_sel_code, uint64_t cap, uint32_t *d_n_motifs,
                                   uint64_t *d_mem_off, uint32_t *d_mem, uint64_t *d_need, void *d_work, uint64_t work_bytes,
                                   void *hip_stream) {
  static const char who[] = "dcrx_cdr3_motif_members_device";
  const Settings St{k_mask, ntrim, ctrim, 1, 0, 0};
  int rc;
  if ((rc = check_members(who, n, St, S, cap))) return rc;
  if (!d_off || !d_mem_off || !d_need || !d_work || (n && (!d_text || !d_n_motifs)) || (S && (!d_sel_k || !d_sel_code)) || (cap && !d_mem))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_members_device: null argument");
  if (reinterpret_cast<uintptr_t>(d_work) % ALIGN)
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_members_device: the work space is not 256-byte aligned");
  Pool P(d_work);
  MembersWork W;
  if ((rc = W.carve(P, n, cap))) return rc;
  if (work_bytes < P.bytes())
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_members_device: the work space is smaller than dcrx_cdr3_motif_members_work_bytes(n, cap)");
  return run_members(n, d_off, d_text, St, S, d_sel_k, d_sel_code, cap, d_n_motifs, d_mem_off, d_mem, d_need, W, (hipStream_t)hip_stream);
}

uint64_t dcrx_cdr3_groups_work_bytes(uint64_t n, uint64_t S) {
  Pool P;
  GroupsWork W;
  if (n >= MAX_UNITS || S > MOTIFS || W.carve(P, n, S) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_groups_device(uint64_t n, const uint64_t *d_weight, const uint64_t *d_adj_off, const uint32_t *d_adj, uint64_t adj_entries,
                            uint64_t S, const uint64_t *d_mem_off, const uint32_t *d_mem, uint64_t mem_entries, uint32_t *d_group_of,
                            uint32_t *d_head, uint32_t *d_units, uint64_t *d_weight_out, uint32_t *d_groups, uint32_t *rounds_out,
                            void *d_work, uint64_t work_bytes, void *hip_stream) {
  if (n >= MAX_UNITS) return set_err(DCRX_E_UNSUPPORTED, "dcrx_cdr3_groups_device: 2^30 or more units");
  if (S > MOTIFS) return set_err(DCRX_E_INVALID, "dcrx_cdr3_groups_device: more than 475 228 member rows");
  if (!d_groups || !d_work || (n && (!d_weight || !d_adj_off || !d_group_of || !d_head || !d_units || !d_weight_out)) ||
      (adj_entries && !d_adj) || (S && !d_mem_off) || (mem_entries && (!d_mem || !S)))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_groups_device: null argument");
  if (reinterpret_cast<uintptr_t>(d_work) % ALIGN) return set_err(DCRX_E_INVALID, "dcrx_cdr3_groups_device: the work space is not 256-byte aligned");
  Pool P(d_work);
  GroupsWork W;
  int rc;
  if ((rc = W.carve(P, n, S))) return rc;
  if (work_bytes < P.bytes())
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_groups_device: the work space is smaller than dcrx_cdr3_groups_work_bytes(n, S)");
  return run_groups(n, d_weight, d_adj_off, d_adj, adj_entries, S, d_mem_off, d_mem, mem_entries, d_group_of, d_head, d_units, d_weight_out,
                    d_groups, rounds_out, W, (hipStream_t)hip_stream);
}

int dcrx_cdr3_motif_groups(uint64_t n, const uint64_t *off, const char *text, const uint64_t *weight, uint32_t k_mask, uint32_t ntrim,
                           uint32_t ctrim, uint64_t S, const uint32_t *sel_k, const uint32_t *sel_code, uint32_t distance,
                           uint32_t *group_of_out, uint32_t *n_motifs_out, uint32_t *degree_out, uint32_t *head_out, uint32_t *units_out,
                           uint64_t *weight_out, uint64_t *mem_off_out, uint32_t *mem_out, uint64_t mem_cap, uint64_t *mem_need_out,
                           dcrx_cdr3_motif_group_stats_t *stats_out) {
  static const char who[] = "dcrx_cdr3_motif_groups";
  const Settings St{k_mask, ntrim, ctrim, 1, 0, 0};
  int rc;
  if ((rc = check_members(who, n, St, S, 0))) return rc;
  if (distance > 2) return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_groups: the distance is 0, 1 or 2");
  if (!off || !mem_off_out || !mem_need_out || !stats_out || (S && (!sel_k || !sel_code)) || (mem_cap && !mem_out) ||
      (n && (!weight || !group_of_out || !n_motifs_out || !degree_out || !head_out || !units_out || !weight_out)))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_groups: null argument");
  if (n && off[n] > off[0] && !text) return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_groups: null argument");
  const int64_t take = host_take_part(n, off, text);
  if (take < 0) return set_err(DCRX_E_INVALID, "dcrx_cdr3_motif_groups: the offsets go down");
  const uint64_t fault = first_selected_fault(S, sel_k, sel_code, k_mask);
  if (fault < S) {
    static thread_local char msg[200];
    std::snprintf(msg, sizeof msg, "dcrx_cdr3_motif_groups: selected motif %llu is no motif of K or is not behind the one before it in motif order",
                  (unsigned long long)fault);
    return set_err(DCRX_E_INVALID, msg);
  }
  const uint64_t text_bytes = off[n] - off[0];
  const uint64_t net_bytes = distance && n ? dcrx_cdr3net_work_bytes(n, text_bytes) : 0;
  if (distance && n && !net_bytes) return set_err(DCRX_E_UNSUPPORTED, "dcrx_cdr3_motif_groups: the neighbour primitive takes no such table");

  Pool P;
  MembersWork MW;
  GroupsWork GW;
  uint64_t *d_off, *d_weight, *d_mem_off, *d_need, *d_adj_off, *d_adj_need, *d_wout;
  uint32_t *d_sel_k, *d_sel_code, *d_n_motifs, *d_degree, *d_cls, *d_group_of, *d_head, *d_units, *d_groups, *d_has_edge, *d_has_row;
  uint8_t *d_text, *d_net;
  Census *d_census;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_off, n + 1); P.get(&d_text, text_bytes); P.get(&d_weight, n); P.get(&d_sel_k, S); P.get(&d_sel_code, S);
    P.get(&d_n_motifs, n); P.get(&d_mem_off, S + 1); P.get(&d_need, 1); P.get(&d_degree, n); P.get(&d_cls, n); P.get(&d_adj_off, n + 1);
    P.get(&d_adj_need, 1); P.get(&d_group_of, n); P.get(&d_head, n); P.get(&d_units, n); P.get(&d_wout, n); P.get(&d_groups, 1);
    P.get(&d_has_edge, n); P.get(&d_has_row, n); P.get(&d_census, 1); P.get(&d_net, net_bytes);
    if ((rc = MW.carve(P, n, 0)) || (rc = GW.carve(P, n, S)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_spans(n, off, text, d_off, d_text)) || (rc = to_device(d_weight, weight, n)) || (rc = to_device(d_sel_k, sel_k, S)) ||
      (rc = to_device(d_sel_code, sel_code, S))) return rc;
  const char *d_chars = reinterpret_cast<const char *>(d_text);

  // the members: a counting call, then exactly `need` of them
  uint64_t need = 0;
  if ((rc = run_members(n, d_off, d_chars, St, S, d_sel_k, d_sel_code, 0, d_n_motifs, d_mem_off, nullptr, d_need, MW, nullptr)) ||
      (rc = to_host(&need, d_need, 1))) return rc;
  if (need + n >= MAX_MEMBER_KEYS) return set_err(DCRX_E_UNSUPPORTED, "dcrx_cdr3_motif_groups: 2^31 - n members or more");
  dcrx::DevBuf<uint32_t> d_mem;
  dcrx::DevBuf<uint8_t> d_mwork;
  if (need) {
    const uint64_t bytes = dcrx_cdr3_motif_members_work_bytes(n, need);
    if (!bytes || d_mem.alloc(need) || d_mwork.alloc(bytes)) return set_err(DCRX_E_NOMEM, "dcrx_cdr3_motif_groups: the members do not fit the device's memory");
    if ((rc = dcrx_cdr3_motif_members_device(n, d_off, d_chars, k_mask, ntrim, ctrim, S, d_sel_k, d_sel_code, need, d_n_motifs, d_mem_off,
                                             d_mem.get(), d_need, d_mwork.get(), bytes, nullptr))) return rc;
  }

  // the global edges: the degree pass, an adjacency of exactly the entries it takes, the write pass
  uint64_t adj_need = 0;
  dcrx::DevBuf<uint32_t> d_adj;
  HIP_TRY(hipMemsetAsync(d_degree, 0, std::max<uint64_t>(n, 1) * 4, nullptr));
  HIP_TRY(hipMemsetAsync(d_adj_off, 0, (n + 1) * 8, nullptr));
  if (distance && n) {
    HIP_TRY(hipMemsetAsync(d_cls, 0, n * 4, nullptr));
    if ((rc = dcrx_cdr3_neighbours_device(n, d_cls, d_off, d_chars, text_bytes, distance, d_degree, d_adj_off, nullptr, 0, d_adj_need, d_net,
                                          net_bytes, nullptr)) ||
        (rc = to_host(&adj_need, d_adj_need, 1))) return rc;
    if (adj_need) {
      if (d_adj.alloc(adj_need)) return set_err(DCRX_E_NOMEM, "dcrx_cdr3_motif_groups: the adjacency does not fit the device's memory");
      if ((rc = dcrx_cdr3_neighbours_device(n, d_cls, d_off, d_chars, text_bytes, distance, d_degree, d_adj_off, d_adj.get(), adj_need,
                                            d_adj_need, d_net, net_bytes, nullptr))) return rc;
    }
  }

  // the groups and their census
  uint32_t rounds = 0, groups = 0;
  if ((rc = run_groups(n, d_weight, d_adj_off, d_adj.get(), adj_need, S, d_mem_off, d_mem.get(), need, d_group_of, d_head, d_units, d_wout,
                       d_groups, &rounds, GW, nullptr))) return rc;
  Census census{};
  if (n) {
    const uint32_t n32 = (uint32_t)n;
    HIP_TRY(hipMemsetAsync(d_has_edge, 0, n * 4, nullptr));
    HIP_TRY(hipMemsetAsync(d_has_row, 0, n * 4, nullptr));
    HIP_TRY(hipMemsetAsync(d_census, 0, sizeof(Census), nullptr));
    group_marks_kernel<<<grid_for(n), TB>>>(d_degree, d_group_of, n32, d_has_edge);
    HIP_TRY(hipGetLastError());
    if (S && need) {
      group_row_marks_kernel<<<grid_for(S), TB>>>(d_mem_off, d_mem.get(), (uint32_t)S, d_group_of, n32, d_has_row);
      HIP_TRY(hipGetLastError());
    }
    group_census_kernel<<<grid_for(n), TB>>>(d_units, d_has_edge, d_has_row, d_groups, d_census);
    HIP_TRY(hipGetLastError());
    if ((rc = to_host(&census, d_census, 1))) return rc;
  }
  if ((rc = to_host(&groups, d_groups, 1)) || (rc = to_host(group_of_out, d_group_of, n)) || (rc = to_host(n_motifs_out, d_n_motifs, n)) ||
      (rc = to_host(degree_out, d_degree, n)) || (rc = to_host(head_out, d_head, groups)) || (rc = to_host(units_out, d_units, groups)) ||
      (rc = to_host(weight_out, d_wout, groups)) || (rc = to_host(mem_off_out, d_mem_off, S + 1))) return rc;
  if (need <= mem_cap && (rc = to_host(mem_out, d_mem.get(), need))) return rc;
  *mem_need_out = need;
  *stats_out = dcrx_cdr3_motif_group_stats_t{n, (uint64_t)take, S, need, adj_need / 2, groups, census.singletons, census.largest, census.mixed, rounds};
  return DCRX_OK;
}

}  // extern "C"

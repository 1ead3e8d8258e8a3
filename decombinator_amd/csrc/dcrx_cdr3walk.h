// dcrx_cdr3walk.h — the tile walk over sorted CDR3 tables and the steps that prepare a table for it, written once for the
// CDR3 network (dcrx_cdr3net.hip), `match` and its weighted metric (dcrx_cdr3match.hip).  Private to those two translation
// units (HIP only, internal linkage, as dcrx_group.h: a unit's instances of the kernels are its own).
//
// Prepare: cdr3_keys_kernel (the key of every node), a stable radix sort of (key, rank) in the walk's bucket order
// (sorted_keys), cdr3_gather_kernel (per sorted position the packed string, and on demand the run mark and the presence mask).
// Walk: cdr3_walk_kernel<WRITE, Side, Pair>.  A block of 256 consecutive sorted nodes of Q, one per lane and in registers,
// walks the sorted entries of T from its first node's bucket to its last node's in LDS tiles of 256 (8 KB of strings, 2 KB of
// keys, 1 KB of ranks in the write pass, 1 KB of masks where the pair test reads them); every lane of a wave reads the same
// staged entry (a broadcast), and a wave skips a tile whose buckets miss its own.  A bucket's entries are in rank order, so a
// node's hits come in ascending rank with no atomics: the degree pass (WRITE false) counts them, an exclusive sum in rank order
// gives the offsets (cdr3_need_kernel closes them), and the write pass (WRITE true) walks again and writes every hit at its
// exact place.
// Sink says what a walk leaves: Out (the two passes above) or Profile, a histogram of the hits' distances per node
// (include/dcrx.h "profile, weighted"): a column of `bins` counters per lane in dynamic LDS, one add per hit, read out behind
// the walk.  Tally (include/dcrx.h "tally, weighted") leaves totals per ENTRY: a count and a weight per staged entry in LDS,
// flushed per tile onto accumulators by sorted position.
// Side says which entries a block walks and whether an entry is the lane's own node: Bipartite (two tables) or Within (one
// table against itself).  Pair is the pair test: Hamming, Levenshtein or Weighted.  Both are dcrx_cdr3pair_core.h's, which a
// plain host build shares (tests/host_cdr3walk walks the same tiles with the same structs); what needs the device stands
// here: begin(), which stages the weighted cost table in LDS, Sorted with its uint4, the sinks and the kernels.
// The weighted metric's host side stands here too, once for both units: what every weighted entry refuses of a cost
// (refuse_cost) and the distance the formatters print (host_weighted).
// The per-node and per-pair code is dcrx_cdr3net_core.h's and dcrx_cdr3w_core.h's, the look-ups are dcrx_cdr3match_core.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "dcrx_cdr3pair_core.h"
#include "dcrx_cdr3profile_core.h"
#include "dcrx_group.h"

namespace dcrx_cdr3walk {
namespace {

using namespace dcrx_cdr3pair;
using namespace dcrx_group;

constexpr uint64_t MAX_NODES = 1ull << 30;
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;
static_assert(BLOCK == (int)QUERIES && BLOCK == (int)TILE, "a lane holds one node and stages one entry");

inline bool metric_exists(uint32_t metric) { return metric == METRIC_HAMMING || metric == METRIC_LEVENSHTEIN; }

struct Nodes {
  const uint32_t *cls;
  const uint64_t *off;
  const uint8_t *text;
  uint64_t text_bytes;
};

// one table in one bucket order: the sorted keys, the ranks, the packed strings and (class order) the presence masks
struct Sorted {
  const uint64_t *key;
  const uint32_t *idx;
  const uint4 *sj;
  const uint32_t *pres;
  uint32_t n;
};

// what a walk leaves, by rank of Q: the degree pass degree and deg64 (the same as 64 bits, for the scan), the write pass the
// hits' ranks — and their distances, where the pair test stores one and dist is not null — at off[rank], below cap
struct Out {
  static constexpr bool HIST = false, TALLY = false;
  uint32_t *degree;
  uint64_t *deg64;
  const uint64_t *off;
  uint32_t *hit, *dist;
  uint64_t cap;
};

// what the profile's walk leaves, by rank of Q: row[rank * bins + b] = the hits of the node whose distance falls into bin b
// (dcrx_cdr3profile_core.h: bin_of).  A lane counts in a column of its own in dynamic LDS, hist[b * BLOCK + lane] (bins * 1 KB
// a block; lanes fall into different banks whatever their bins): a register array indexed by a run-time bin would go to
// scratch, and a chain of compares costs `bins` compares a hit where most pairs of a class are hits.  The column is the
// lane's alone, so it needs no barrier: zeroed in front of the walk, read out behind it.  A node that takes no part keeps its
// zeros and writes them; lanes behind the table write nothing.
struct Profile {
  static constexpr bool HIST = true, TALLY = false;
  uint32_t *row;
  uint32_t step, bins;
  __device__ __forceinline__ uint32_t *column() const {
    extern __shared__ uint32_t lds_hist[];
    return lds_hist + threadIdx.x;
  }
  __device__ __forceinline__ void clear(uint32_t *col) const {
    for (uint32_t b = 0; b < bins; b++) col[b * BLOCK] = 0;
  }
  __device__ __forceinline__ void add(uint32_t *col, uint32_t d) const {
    atomicAdd(&col[dcrx_cdr3profile::bin_of(d, step) * BLOCK], 1u);      // (no lane shares it: an add whose result is not read)
  }
  __device__ __forceinline__ void read_out(const uint32_t *col, uint32_t e) const {
    for (uint32_t b = 0; b < bins; b++) row[(size_t)e * bins + b] = col[b * BLOCK];
  }
};

// what the tally's walk leaves: per sorted position p of T, acc_count[p] = the nodes of Q that hit the entry and acc_weight[p]
// the sum of their weights (weight: by rank of Q), ADDED onto what the arrays hold — the caller zeroes them in front of the walk —,
// and by rank of Q degree = the entries the node hits.  A block keeps a count and a weight per staged entry in LDS (lds_c, lds_w
// of the walk: 3 KB); a hit adds to them with LDS atomics whose results are not read.  At the top of the next tile, behind the
// barrier that stands there, and once behind the walk, lane k flushes entry k — where its count is not zero, one global add each
// onto acc_count[t + k] and acc_weight[t + k], results not read — and zeroes its two cells: at most two global atomics per
// (block, staged entry) however many lanes hit, on addresses that ascend with the lane because the accumulators are by sorted
// position (the ranks of a tile are scattered).  A tile that no wave tests adds nothing and so flushes nothing.
struct Tally {
  static constexpr bool HIST = false, TALLY = true;
  const uint64_t *weight;
  uint32_t *acc_count;
  unsigned long long *acc_weight;
  uint32_t *degree;
};

// the length of node e's string; one past the reach for offsets that go backwards or leave the text
__device__ __forceinline__ uint64_t node_len(const Nodes &N, uint32_t e, uint64_t *at) {
  const uint64_t a = N.off[e], b = N.off[e + 1];
  *at = a;
  return (b < a || b > N.text_bytes) ? (uint64_t)MAX_LEN + 1 : b - a;
}

__global__ __launch_bounds__(BLOCK) void cdr3_keys_kernel(Nodes N, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  uint64_t at;
  key[e] = node_key(N.cls[e], node_len(N, e, &at));
  idx[e] = e;
}

// keys of n nodes, then their stable sort over the key's bits from begin_bit (0: by (class, length); LEN_BITS: by class, the
// sorted keys keep the lengths): (key[1], idx[1])
inline int sorted_keys(const Nodes &N, uint64_t n, uint64_t *const key[2], uint32_t *const idx[2], Scratch cub, int begin_bit, bool make_keys,
                       hipStream_t s) {
  if (make_keys) {
    cdr3_keys_kernel<<<grid_for(n), BLOCK, 0, s>>>(N, (uint32_t)n, key[0], idx[0]);
    HIP_TRY(hipGetLastError());
  }
  return sort_pairs(cub, key[0], key[1], idx[0], idx[1], n, KEY_BITS, s, begin_bit);
}

// per sorted position the packed string; MARKS: the run mark of its bucket, whose max scan gives every position its bucket's
// start; PRES: its letter-presence mask goes beside the string; CLS: the table is in class order (the marks are the classes':
// with the masks unless said otherwise — the weighted network's table is in class order and has no masks)
template <bool MARKS, bool PRES, bool CLS = PRES>
__global__ __launch_bounds__(BLOCK) void cdr3_gather_kernel(Nodes N, uint32_t n, const uint64_t *__restrict__ key,
                                                            const uint32_t *__restrict__ idx, uint4 *__restrict__ sj,
                                                            uint32_t *__restrict__ mark, uint32_t *__restrict__ pres) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= n) return;
  uint64_t at;
  const uint64_t len = node_len(N, idx[s], &at);
  uint32_t w[WORDS];
  pack(N.text + (in_reach(len) ? at : 0), len, w);
  sj[2 * (size_t)s] = make_uint4(w[0], w[1], w[2], w[3]);
  sj[2 * (size_t)s + 1] = make_uint4(w[4], w[5], w[6], w[7]);
  if (MARKS) mark[s] = run_mark(s, [&](uint32_t k) { return bucket_of<CLS>(key[k]); });
  if (PRES) pres[s] = presence(w, in_reach(len) ? (uint32_t)len : 0u);
}

// off[n] and the need behind the scan
__global__ void cdr3_need_kernel(const uint64_t *__restrict__ deg64, uint64_t *__restrict__ off, uint32_t n, uint64_t *__restrict__ need) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t total = off[n - 1] + deg64[n - 1];
    off[n] = total;
    if (need) *need = total;
  }
}

// ---- begin() runs once per lane in front of the walk and returns the Pair::Ctx that window() and test() are handed back
// (the sides and the pair tests themselves are dcrx_cdr3pair_core.h's)

template <class Pair> __device__ __forceinline__ typename Pair::Ctx begin(const Pair &) { return {}; }

// the weighted cost with its table in LDS, a dword from every lane
__device__ __forceinline__ Cost begin(const Weighted &pair) {
  __shared__ uint32_t lds_sub[SUB_BYTES / 4];
  lds_sub[threadIdx.x] = pair.cost.sub[threadIdx.x];      // (the walk's first barrier stands before its first read)
  return Cost{reinterpret_cast<const uint8_t *>(lds_sub), pair.cost.gap, pair.cost.ntrim, pair.cost.ctrim};
}
__device__ __forceinline__ Cost begin(const WeightedPer &pair) {      // (an overload of its own: Weighted's stays what it compiled to)
  __shared__ uint32_t lds_sub[SUB_BYTES / 4];
  lds_sub[threadIdx.x] = pair.cost.sub[threadIdx.x];
  return Cost{reinterpret_cast<const uint8_t *>(lds_sub), pair.cost.gap, pair.cost.ntrim, pair.cost.ctrim};
}

// The walk (see the head of the file).  Q: the block's nodes, T: the entries it walks, both sorted in Pair's bucket order.
template <bool WRITE, class Side, class Pair, class Sink = Out>
__global__ __launch_bounds__(BLOCK) void cdr3_walk_kernel(Sorted Q, Sorted T, Side side, Pair pair, Sink O) {
  constexpr bool CLS = Pair::CLS;
  static_assert(!((Sink::HIST || Sink::TALLY) && WRITE), "a profile and a tally are one pass");
  __shared__ uint4 lds_j[TILE * 2];
  __shared__ uint64_t lds_k[TILE];
  __shared__ uint32_t lds_r[WRITE ? TILE : 1];
  __shared__ uint32_t lds_p[Pair::MASKS ? TILE : 1];
  __shared__ uint32_t lds_b[Pair::PER ? TILE : 1];                    // the staged entries' own bounds
  __shared__ uint32_t lds_c[Sink::TALLY ? TILE : 1];                  // the tally: per staged entry the hits ...
  __shared__ unsigned long long lds_w[Sink::TALLY ? TILE : 1];        // ... and their weights
  const typename Pair::Ctx ctx = begin(pair);
  const uint32_t s0 = blockIdx.x * BLOCK;
  const uint32_t s = s0 + threadIdx.x;
  const bool valid = s < Q.n;
  const uint64_t key_own = valid ? Q.key[s] : KEY_OUT_OF_REACH;
  bool reach = key_own != KEY_OUT_OF_REACH;
  const uint64_t k_own = bucket_of<CLS>(key_own);
  const uint32_t len_own = key_length(key_own), pres_own = Pair::MASKS && valid ? Q.pres[s] : 0u;
  uint32_t own[WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t e = 0, count = 0;
  uint64_t at = 0;
  uint32_t *col = nullptr;
  if constexpr (Sink::HIST) {
    col = O.column();
    O.clear(col);
  }
  unsigned long long w_own = 0;
  uint32_t flush_at = 0;      // the tile whose totals stand in lds_c and lds_w
  // lane k flushes entry k of that tile (its own two cells: the barriers around the staging stand between this and the adds)
  auto flush = [&]() __attribute__((always_inline)) {
    if constexpr (Sink::TALLY) {
      const uint32_t c = lds_c[threadIdx.x];
      if (c != 0 && flush_at + threadIdx.x < T.n) {
        atomicAdd(&O.acc_count[flush_at + threadIdx.x], c);
        atomicAdd(&O.acc_weight[flush_at + threadIdx.x], lds_w[threadIdx.x]);
        lds_c[threadIdx.x] = 0;
        lds_w[threadIdx.x] = 0;
      }
    }
  };
  if constexpr (Sink::TALLY) {
    lds_c[threadIdx.x] = 0;
    lds_w[threadIdx.x] = 0;
  }
  if (valid) {
    e = Q.idx[s];
    if constexpr (WRITE) at = O.off[e];
    if constexpr (Sink::TALLY) w_own = O.weight[e];
    if (reach) {
      const uint4 a = Q.sj[2 * (size_t)s], b = Q.sj[2 * (size_t)s + 1];
      own[0] = a.x; own[1] = a.y; own[2] = a.z; own[3] = a.w; own[4] = b.x; own[5] = b.y; own[6] = b.z; own[7] = b.w;
      reach = pair.admits(own, len_own);
    }
  }
  // the wave's buckets (sorted along s; lanes behind the table hold the largest)
  const uint64_t w_lo = __shfl(k_own, 0), w_hi = __shfl(k_own, warpSize - 1);
  const Range R = side.template range<CLS>(Q.key, Q.n, T.key, T.n, s0);
  for (uint32_t t = R.first; t < T.n; t += TILE) {
    if (!goes_on<CLS>(R, T.key[t])) break;
    __syncthreads();                                        // the previous tile is no longer read
    flush();
    flush_at = t;
    const uint32_t tile_n = min((uint32_t)TILE, T.n - t);
    if (threadIdx.x < tile_n) {
      const uint32_t p = t + threadIdx.x;
      const uint4 a = T.sj[2 * (size_t)p], b = T.sj[2 * (size_t)p + 1];
      lds_j[2 * threadIdx.x] = a;
      lds_j[2 * threadIdx.x + 1] = b;
      const uint32_t w[WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      if constexpr (Pair::PER) {
        const uint32_t bound = pair.bound_of(T.idx[p]);      // (a gather by rank: the index stays as it is)
        lds_b[threadIdx.x] = bound;
        lds_k[threadIdx.x] = pair.staged(w, T.key[p], bound);
      } else {
        lds_k[threadIdx.x] = pair.staged(w, T.key[p]);
      }
      if (WRITE) lds_r[threadIdx.x] = T.idx[p];
      if (Pair::MASKS) lds_p[threadIdx.x] = T.pres[p];
    }
    __syncthreads();
    if (wave_skips(bucket_of<CLS>(lds_k[0]), bucket_of<CLS>(lds_k[tile_n - 1]), w_lo, w_hi)) continue;
    const uint32_t *lj = reinterpret_cast<const uint32_t *>(lds_j);
    auto take = [&](uint32_t q, uint32_t len_q) __attribute__((always_inline)) {
      uint32_t d, bound;
      if constexpr (Pair::PER) {
        bound = lds_b[q];      // (a broadcast, as the key)
        d = pair.test(ctx, own, len_own, lj + q * WORDS, len_q, bound);
      } else {
        bound = pair.bound();
        d = pair.test(ctx, own, len_own, lj + q * WORDS, len_q);
      }
      if (d <= bound) {
        if constexpr (Sink::HIST) {
          O.add(col, d);
        } else if constexpr (Sink::TALLY) {
          atomicAdd(&lds_c[q], 1u);      // (results not read)
          atomicAdd(&lds_w[q], w_own);
          count++;
        } else {
          if (WRITE && at + count < O.cap) {
            O.hit[at + count] = lds_r[q];
            if (Pair::DIST && O.dist) O.dist[at + count] = d;
          }
          count++;
        }
      }
    };
    // DEFER: an entry that passes the cheap tests waits in `pending` (one per lane), and the test runs — for every lane that
    // has one waiting, each on its own entry — only once some lane meets its next one, and at the tile's end: the few lanes
    // of a wave that pass at one entry would otherwise run it nearly alone.  A lane still takes its entries in order.
    uint32_t pending = NO_ENTRY;
    auto settle = [&]() __attribute__((always_inline)) {
      if (pending != NO_ENTRY) {      // (per lane: the vote below is the wave's, what waits is the lane's)
        take(pending, key_length(lds_k[pending]));
        pending = NO_ENTRY;
      }
    };
    for (uint32_t q = 0; q < tile_n; q++) {
      const uint64_t key_q = lds_k[q], kq = bucket_of<CLS>(key_q);
      if (kq < w_lo) continue;
      if (kq > w_hi) break;
      const uint32_t len_q = key_length(key_q);
      bool passes;
      if constexpr (Pair::PER) passes = reach && kq == k_own && !side.self(t + q, s) && pair.window(ctx, len_own, pres_own, len_q, 0u, lds_b[q]);
      else passes = reach && kq == k_own && !side.self(t + q, s) && pair.window(ctx, len_own, pres_own, len_q, Pair::MASKS ? lds_p[q] : 0u);
      if (Pair::DEFER) {
        if (__any(passes && pending != NO_ENTRY)) settle();      // (the same for every lane of the wave)
        if (passes) pending = q;
      } else if (passes) {
        take(q, len_q);
      }
    }
    if (Pair::DEFER) settle();      // (the next tile overwrites the staged entries)
  }
  if constexpr (Sink::HIST) {
    if (valid) O.read_out(col, e);
  } else if constexpr (Sink::TALLY) {
    __syncthreads();      // (the walk's end is the same for every lane of the block: the last tile's adds are done)
    flush();
    if (valid) O.degree[e] = count;
  } else if (valid && !WRITE) {
    O.degree[e] = count;
    O.deg64[e] = count;
  }
}

// ---- the weighted metric on the host: what every weighted entry refuses, and the distance the formatters print

// what every weighted entry refuses of (cost, radius), on the host; the cost as the walk's launch argument
inline int refuse_cost(const char *who, const dcrx_cdr3_cost_t *cost, uint32_t radius, CostArg *arg) {
  auto fail = [&](const char *what) { return dcrx::set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  if (!cost) return fail("null cost");
  if (radius > MAX_RADIUS) return fail("the radius is 0 .. 65535");
  if (cost->gap < 1 || cost->gap > MAX_GAP) return fail("the gap cost is 1 .. 255");
  if (cost->ntrim > MAX_TRIM || cost->ctrim > MAX_TRIM) return fail("a trim is 0 .. 16");
  for (uint32_t x = 1; x <= 26; x++) {
    if (cost->sub[x][x]) return fail("the substitution table is not zero on its diagonal");
    for (uint32_t y = 1; y < x; y++)
      if (cost->sub[x][y] != cost->sub[y][x]) return fail("the substitution table is not symmetric");
  }
  if (arg) {
    static_assert(sizeof cost->sub == sizeof arg->sub, "one table");
    std::memcpy(arg->sub, cost->sub, sizeof arg->sub);
    arg->gap = cost->gap; arg->ntrim = cost->ntrim; arg->ctrim = cost->ctrim;
  }
  return DCRX_OK;
}

inline bool host_letters(const char *a, uint64_t la) {
  for (uint64_t i = 0; i < la; i++)
    if (a[i] < 'A' || a[i] > 'Z') return false;
  return true;
}

// the weighted distance of two strings of letters (the files' distance column): the contract read out, the literal minimum
// over every gap position p in 0 .. la of the sum over the counted positions
inline uint64_t host_weighted(const char *a, uint64_t la, const char *b, uint64_t lb, const dcrx_cdr3_cost_t &cost) {
  if (la > lb) { std::swap(a, b); std::swap(la, lb); }
  const uint64_t d = lb - la;
  uint64_t best = UINT64_MAX;
  for (uint64_t p = 0; p <= (d ? la : 0); p++) {
    uint64_t sum = 0;
    for (uint64_t i = 0; i < la; i++) {
      if (i < cost.ntrim || i + cost.ctrim >= la) continue;
      sum += cost.sub[a[i] & 31][b[i < p ? i : i + d] & 31];
    }
    best = std::min(best, sum);
  }
  return d * cost.gap + best;
}

// one pass under the Hamming metric, or (lev) the Levenshtein metric at a distance above 0
template <bool WRITE, class Side> int walk(const Sorted &Q, const Sorted &T, Side side, uint32_t limit, bool lev, const Out &O, hipStream_t s) {
  if (lev) cdr3_walk_kernel<WRITE><<<grid_for(Q.n), BLOCK, 0, s>>>(Q, T, side, Levenshtein{limit}, O);
  else cdr3_walk_kernel<WRITE><<<grid_for(Q.n), BLOCK, 0, s>>>(Q, T, side, Hamming{limit}, O);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

}  // namespace
}  // namespace dcrx_cdr3walk

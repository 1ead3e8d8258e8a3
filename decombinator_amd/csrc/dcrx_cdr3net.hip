// dcrx_cdr3net.hip — the CDR3 network (`--clonotypes --cdr3-network`): which nodes (clonotypes) of one class and one string
// length lie within D substitutions of each other, and the connected components of that graph; include/dcrx.h holds the
// contract, dcrx_cdr3net_core.h the per-node and per-pair code.
//
// The primitive (dcrx_cdr3_neighbours_device), all on the caller's stream and in the caller's work space:
//   keys     cdr3net_keys_kernel, one lane per node: the bucket key (class, length), out of reach behind every bucket
//   sort     a stable radix sort of (key, rank): a bucket stays in rank order
//   gather   cdr3net_gather_kernel, one lane per sorted position: the 32-byte packed string, and the run marks whose max scan
//            gives every position its bucket's start
//   degrees  cdr3net_walk_kernel<false>: a block of 256 consecutive sorted nodes walks the sorted entries from its first
//            node's bucket start to its last node's bucket end in LDS tiles of 256 (8 KB of strings, 2 KB of keys, 1 KB of
//            ranks); every lane of a wave reads the same staged entry (a broadcast), and a wave skips a tile whose key range
//            misses its own.  Every node counts its OWN neighbours over its whole bucket: twice the comparisons of a
//            triangular walk, but no atomics, and the neighbours come in ascending rank
//   scan     an exclusive sum of the degrees in rank order: adj_off, whose end is the need
//   write    cdr3net_walk_kernel<true>: the same walk writes every neighbour's rank at its exact offset
// The host entry (dcrx_cdr3_network) runs those two halves around the adjacency's allocation, then the components (rounds of
// "the smallest label among my neighbours and me" and pointer jumping, double buffered, until a round changes nothing) and
// the totals (integer atomics onto the heads, results unused; the heads compacted in rank order).
// The sorts, scans, run heads and compaction are dcrx_group.h's.
//
// Under the Levenshtein metric (the *_metric entries, DCRX_CDR3NET_LEVENSHTEIN) the bucket is the class alone: the same keys
// are sorted over their class bits and the out-of-reach bit only — stable, so a class stays in rank order and the sorted keys
// keep every node's length —, the gather also leaves a letter-presence mask per node, and the walk (the LEV forms of the same
// kernels) tests a pair by class, length difference, presence masks and then lev_within (on the entry a lane has waiting,
// once some lane of the wave meets its next one).  A node still walks its whole bucket, now its class: the extra pairs fall
// at one length compare, and the neighbours still come in ascending rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_cdr3net_core.h"
#include "dcrx_group.h"
#include "dcrx_text.h"

using dcrx::set_err;
using namespace dcrx_cdr3net;
using namespace dcrx_group;

namespace {

constexpr uint64_t MAX_NODES = 1ull << 30;
constexpr int TILE = 256;        // staged entries per step
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;

struct Nodes {
  const uint32_t *cls;
  const uint64_t *off;
  const uint8_t *text;
  uint64_t text_bytes;
};

// the length of node e's string; one past the reach for offsets that go backwards or leave the text
__device__ __forceinline__ uint64_t node_len(const Nodes &N, uint32_t e, uint64_t *at) {
  const uint64_t a = N.off[e], b = N.off[e + 1];
  *at = a;
  return (b < a || b > N.text_bytes) ? (uint64_t)MAX_LEN + 1 : b - a;
}

__global__ __launch_bounds__(BLOCK) void cdr3net_keys_kernel(Nodes N, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  uint64_t at;
  key[e] = node_key(N.cls[e], node_len(N, e, &at));
  idx[e] = e;
}

// the key a bucket is made of: the whole key, or under the Levenshtein metric its class (and out-of-reach) bits
template <bool LEV> __device__ __forceinline__ uint64_t bucket_of(uint64_t key) { return LEV ? key_class(key) : key; }

// LEV: the run marks are the classes', and every node's letter-presence mask goes beside its string
template <bool LEV>
__global__ __launch_bounds__(BLOCK) void cdr3net_gather_kernel(Nodes N, uint32_t n, const uint64_t *__restrict__ key,
                                                               const uint32_t *__restrict__ idx, uint4 *__restrict__ sj,
                                                               uint32_t *__restrict__ mark, uint32_t *__restrict__ pres) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= n) return;
  const uint32_t e = idx[s];
  uint64_t at;
  const uint64_t len = node_len(N, e, &at);
  uint32_t w[WORDS];
  pack(N.text + (in_reach(len) ? at : 0), len, w);
  sj[2 * (size_t)s] = make_uint4(w[0], w[1], w[2], w[3]);
  sj[2 * (size_t)s + 1] = make_uint4(w[4], w[5], w[6], w[7]);
  mark[s] = run_mark(s, [&](uint32_t k) { return bucket_of<LEV>(key[k]); });
  if (LEV) pres[s] = presence(w, in_reach(len) ? (uint32_t)len : 0u);
}

// The walk.  WRITE false: degree[rank] (and the same as 64 bits, for the scan); true: the neighbours' ranks at adj_off[rank].
// LEV: the buckets are the classes (the staged keys still hold the lengths), the presence masks are staged with the strings,
// and a pair is tested by length difference, presence masks and lev_within instead of the Hamming distance.
template <bool WRITE, bool LEV>
__global__ __launch_bounds__(BLOCK) void cdr3net_walk_kernel(const uint4 *__restrict__ sj, const uint64_t *__restrict__ key,
                                                             const uint32_t *__restrict__ idx, const uint32_t *__restrict__ bstart,
                                                             uint32_t n, uint32_t limit, uint32_t *__restrict__ degree,
                                                             uint64_t *__restrict__ deg64, const uint64_t *__restrict__ adj_off,
                                                             uint32_t *__restrict__ adj, uint64_t adj_cap,
                                                             const uint32_t *__restrict__ pres) {
  __shared__ uint4 lds_j[TILE * 2];
  __shared__ uint64_t lds_k[TILE];
  __shared__ uint32_t lds_r[TILE];
  __shared__ uint32_t lds_p[LEV ? TILE : 1];
  const uint32_t s0 = blockIdx.x * BLOCK;
  const uint32_t s = s0 + threadIdx.x;
  const bool valid = s < n;
  const uint64_t key_own = valid ? key[s] : KEY_OUT_OF_REACH;
  const bool reach = key_own != KEY_OUT_OF_REACH;
  const uint64_t k_own = bucket_of<LEV>(key_own);
  const uint32_t len_own = key_length(key_own), pres_own = LEV && valid ? pres[s] : 0u;
  uint32_t own[WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t e = 0, count = 0;
  uint64_t at = 0;
  if (valid) {
    e = idx[s];
    if (WRITE) at = adj_off[e];
    if (reach) {
      const uint4 a = sj[2 * (size_t)s], b = sj[2 * (size_t)s + 1];
      own[0] = a.x; own[1] = a.y; own[2] = a.z; own[3] = a.w; own[4] = b.x; own[5] = b.y; own[6] = b.z; own[7] = b.w;
    }
  }
  // the wave's keys (sorted along s; lanes behind the table hold the largest key)
  const uint64_t w_lo = __shfl(k_own, 0), w_hi = __shfl(k_own, warpSize - 1);
  // the block's entries: from its first node's bucket start to its last node's bucket end, nodes out of reach left out
  const uint64_t k_max = min(bucket_of<LEV>(key[min(n, s0 + (uint32_t)BLOCK) - 1]), bucket_of<LEV>(KEY_OUT_OF_REACH) - 1);
  for (uint32_t t = bstart[s0]; t < n; t += TILE) {
    if (bucket_of<LEV>(key[t]) > k_max) break;              // (the same for every lane of the block)
    __syncthreads();                                        // the previous tile is no longer read
    const uint32_t tile_n = min((uint32_t)TILE, n - t);
    if (threadIdx.x < tile_n) {
      const uint32_t p = t + threadIdx.x;
      lds_j[2 * threadIdx.x] = sj[2 * (size_t)p];
      lds_j[2 * threadIdx.x + 1] = sj[2 * (size_t)p + 1];
      lds_k[threadIdx.x] = key[p];
      if (WRITE) lds_r[threadIdx.x] = idx[p];
      if (LEV) lds_p[threadIdx.x] = pres[p];
    }
    __syncthreads();
    if (bucket_of<LEV>(lds_k[tile_n - 1]) < w_lo || bucket_of<LEV>(lds_k[0]) > w_hi) continue;      // the tile holds nothing of this wave's buckets
    const uint32_t *lj = reinterpret_cast<const uint32_t *>(lds_j);
    if (!LEV) {
      for (uint32_t q = 0; q < tile_n; q++) {
        const uint64_t kq = lds_k[q];
        if (kq < w_lo) continue;
        if (kq > w_hi) break;
        if (reach && kq == k_own && t + q != s && distance(own, lj + q * WORDS, limit) <= limit) {
          if (WRITE && at + count < adj_cap) adj[at + count] = lds_r[q];
          count++;
        }
      }
      continue;
    }
    // LEV: an entry that passes the cheap tests waits in `pending` (one per lane), and lev_within runs — for every lane that
    // has one waiting, each on its own entry — only once some lane meets its next one, and at the tile's end: the few lanes
    // of a wave that pass at one entry would otherwise run it nearly alone.  A lane still takes its entries in order.
    uint32_t pending = NO_ENTRY;
    auto settle = [&]() {
      if (pending != NO_ENTRY) {
        if (lev_within(own, len_own, lj + pending * WORDS, key_length(lds_k[pending]), limit) <= limit) {
          if (WRITE && at + count < adj_cap) adj[at + count] = lds_r[pending];
          count++;
        }
        pending = NO_ENTRY;
      }
    };
    for (uint32_t q = 0; q < tile_n; q++) {
      const uint64_t key_q = lds_k[q], kq = key_class(key_q);
      if (kq < w_lo) continue;
      if (kq > w_hi) break;
      const uint32_t len_q = key_length(key_q);
      const bool passes = reach && kq == k_own && t + q != s && len_q + limit >= len_own && len_own + limit >= len_q &&
                          presence_allows(pres_own, lds_p[q], limit);
      if (__any(passes && pending != NO_ENTRY)) settle();      // (the same for every lane of the wave)
      if (passes) pending = q;
    }
    settle();      // (the next tile overwrites the staged entries)
  }
  if (valid && !WRITE) {
    degree[e] = count;
    deg64[e] = count;
  }
}

// adj_off[m] and the need behind the scan
__global__ void cdr3net_need_kernel(const uint64_t *__restrict__ deg64, uint64_t *__restrict__ adj_off, uint32_t n,
                                    uint64_t *__restrict__ need) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t total = adj_off[n - 1] + deg64[n - 1];
    adj_off[n] = total;
    if (need) *need = total;
  }
}

// ---- the host entry's kernels ----

__global__ __launch_bounds__(BLOCK) void cdr3net_label_init_kernel(uint32_t n, uint32_t *__restrict__ label) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) label[i] = i;
}

// a round's first half: the smallest label among a node's neighbours and itself
__global__ __launch_bounds__(BLOCK) void cdr3net_min_kernel(const uint32_t *__restrict__ in, const uint64_t *__restrict__ adj_off,
                                                            const uint32_t *__restrict__ adj, uint32_t n, uint32_t *__restrict__ out,
                                                            uint32_t *__restrict__ changed) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  bool moved = false;
  if (i < n) {
    const uint32_t mine = in[i];
    uint32_t l = mine;
    for (uint64_t k = adj_off[i], end = adj_off[i + 1]; k < end; k++) l = min(l, in[adj[k]]);
    out[i] = l;
    moved = l != mine;
  }
  if (__ballot(moved) && __lane_id() == 0) *changed = 1u;
}

// ... and its second: every label followed to where it ends (a label is a rank not above its node: the chain falls)
__global__ __launch_bounds__(BLOCK) void cdr3net_jump_kernel(const uint32_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t l = in[i];
  for (uint32_t next = in[l]; next != l; next = in[l]) l = next;
  out[i] = l;
}

__global__ __launch_bounds__(BLOCK) void cdr3net_totals_kernel(const uint32_t *__restrict__ label, const uint64_t *__restrict__ weight,
                                                               uint32_t n, unsigned long long *__restrict__ total,
                                                               uint32_t *__restrict__ members, uint32_t *__restrict__ is_head) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = label[i];
  atomicAdd(&total[h], (unsigned long long)weight[i]);
  atomicAdd(&members[h], 1u);
  is_head[i] = h == i ? 1u : 0u;
}

__global__ __launch_bounds__(BLOCK) void cdr3net_rows_kernel(const uint32_t *__restrict__ heads, uint32_t c,
                                                             const unsigned long long *__restrict__ total,
                                                             const uint32_t *__restrict__ members, uint32_t *__restrict__ nn_out,
                                                             uint64_t *__restrict__ w_out) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= c) return;
  const uint32_t h = heads[r];
  nn_out[r] = members[h];
  w_out[r] = total[h];
}

__global__ __launch_bounds__(BLOCK) void cdr3net_cluster_of_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ slot,
                                                                   uint32_t n, uint32_t *__restrict__ cluster_of) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) cluster_of[i] = slot[label[i]];
}

bool metric_exists(uint32_t metric) { return metric == METRIC_HAMMING || metric == METRIC_LEVENSHTEIN; }

// ---- work space of the primitive: the degree pass leaves the sorted keys and ranks (key[1], idx[1]), the bucket starts, the
// packed strings and the presence masks there for the write pass
struct Work {
  uint64_t *key[2];
  uint32_t *idx[2], *mark, *bstart;
  uint4 *sj;
  uint64_t *deg64;
  Scratch cub;
  uint32_t *pres;      // (the Levenshtein walk's; null under Hamming, whose work space is what it was: the masks come behind it)
  int carve(Pool &P, uint64_t n, uint32_t metric) {
    size_t cub_bytes = 0;
    const uint64_t k = std::max<uint64_t>(n, 1);
    int rc;
    if ((rc = sort_pairs_bytes<uint32_t>(k, KEY_BITS, &cub_bytes)) || (rc = run_heads_bytes(k, &cub_bytes)) ||
        (rc = exclusive_sum_bytes<uint64_t>(k, &cub_bytes))) return rc;
    P.get(&key[0], n); P.get(&key[1], n); P.get(&idx[0], n); P.get(&idx[1], n); P.get(&mark, n); P.get(&bstart, n);
    P.get(&sj, 2 * n); P.get(&deg64, n); P.get(&cub, cub_bytes);
    pres = nullptr;
    if (metric == METRIC_LEVENSHTEIN) P.get(&pres, n);
    return DCRX_OK;
  }
};

// keys, sort, gather, the degree pass, the scan and the need
int run_degrees(const Nodes &N, uint64_t n, uint32_t limit, uint32_t metric, uint32_t *d_degree, uint64_t *d_adj_off, uint64_t *d_need,
                const Work &W, hipStream_t s) {
  const bool lev = metric == METRIC_LEVENSHTEIN;
  const uint32_t n32 = (uint32_t)n;
  int rc;
  cdr3net_keys_kernel<<<grid_for(n), BLOCK, 0, s>>>(N, n32, W.key[0], W.idx[0]);
  HIP_TRY(hipGetLastError());
  if ((rc = sort_pairs(W.cub, W.key[0], W.key[1], W.idx[0], W.idx[1], n, KEY_BITS, s, lev ? (int)LEN_BITS : 0))) return rc;
  if (lev) cdr3net_gather_kernel<true><<<grid_for(n), BLOCK, 0, s>>>(N, n32, W.key[1], W.idx[1], W.sj, W.mark, W.pres);
  else cdr3net_gather_kernel<false><<<grid_for(n), BLOCK, 0, s>>>(N, n32, W.key[1], W.idx[1], W.sj, W.mark, nullptr);
  HIP_TRY(hipGetLastError());
  if ((rc = run_heads(W.cub, W.mark, W.bstart, n, s))) return rc;
  if (lev)
    cdr3net_walk_kernel<false, true><<<grid_for(n), BLOCK, 0, s>>>(W.sj, W.key[1], W.idx[1], W.bstart, n32, limit, d_degree, W.deg64, nullptr,
                                                                   nullptr, 0, W.pres);
  else
    cdr3net_walk_kernel<false, false><<<grid_for(n), BLOCK, 0, s>>>(W.sj, W.key[1], W.idx[1], W.bstart, n32, limit, d_degree, W.deg64, nullptr,
                                                                    nullptr, 0, nullptr);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_sum(W.cub, W.deg64, d_adj_off, n, s))) return rc;
  cdr3net_need_kernel<<<1, 64, 0, s>>>(W.deg64, d_adj_off, n32, d_need);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

int run_write(uint64_t n, uint32_t limit, uint32_t metric, const uint64_t *d_adj_off, uint32_t *d_adj, uint64_t adj_cap, const Work &W,
              hipStream_t s) {
  if (metric == METRIC_LEVENSHTEIN)
    cdr3net_walk_kernel<true, true><<<grid_for(n), BLOCK, 0, s>>>(W.sj, W.key[1], W.idx[1], W.bstart, (uint32_t)n, limit, nullptr, nullptr,
                                                                  d_adj_off, d_adj, adj_cap, W.pres);
  else
    cdr3net_walk_kernel<true, false><<<grid_for(n), BLOCK, 0, s>>>(W.sj, W.key[1], W.idx[1], W.bstart, (uint32_t)n, limit, nullptr, nullptr,
                                                                   d_adj_off, d_adj, adj_cap, nullptr);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// an error of the entry `who` (the plain entries and their *_metric forms share one body and name themselves)
int fail(int code, const char *who, const char *what) { return set_err(code, (std::string(who) + ": " + what).c_str()); }

int neighbours_device(const char *who, uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                      uint32_t distance, uint32_t metric, uint32_t *d_degree, uint64_t *d_adj_off, uint32_t *d_adj, uint64_t adj_cap,
                      uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream) try {
  if (m >= MAX_NODES) return fail(DCRX_E_UNSUPPORTED, who, "2^30 or more nodes");
  if (distance != 1 && distance != 2) return fail(DCRX_E_INVALID, who, "the distance is 1 or 2");
  if (!metric_exists(metric)) return fail(DCRX_E_INVALID, who, "the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN");
  hipStream_t s = (hipStream_t)hip_stream;
  if (!m) {
    if (d_adj_need) HIP_TRY(hipMemsetAsync(d_adj_need, 0, sizeof(uint64_t), s));
    if (d_adj_off) HIP_TRY(hipMemsetAsync(d_adj_off, 0, sizeof(uint64_t), s));
    return DCRX_OK;
  }
  if (!d_class || !d_off || !d_degree || !d_adj_off || !d_work || (text_bytes && !d_text) || (adj_cap && !d_adj))
    return fail(DCRX_E_INVALID, who, "null argument");
  if ((uintptr_t)d_work % ALIGN) return fail(DCRX_E_INVALID, who, "the work space is not 256-byte aligned");
  Pool P(d_work);
  Work W;
  int rc = W.carve(P, m, metric);
  if (rc) return rc;
  if (work_bytes < P.bytes())
    return fail(DCRX_E_INVALID, who, metric == METRIC_HAMMING ? "the work space is smaller than dcrx_cdr3net_work_bytes(m, text_bytes)"
                                                              : "the work space is smaller than dcrx_cdr3net_metric_work_bytes(m, text_bytes, metric)");
  const Nodes N{d_class, d_off, reinterpret_cast<const uint8_t *>(d_text), text_bytes};
  if ((rc = run_degrees(N, m, distance, metric, d_degree, d_adj_off, d_adj_need, W, s))) return rc;
  if (!d_adj || !adj_cap) return DCRX_OK;
  return run_write(m, distance, metric, d_adj_off, d_adj, adj_cap, W, s);
} catch (const std::exception &e) {      // (a message that could not be built)
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t network(const char *who, uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                uint32_t distance, uint32_t metric, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out,
                uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint64_t adj_cap,
                uint64_t *adj_need_out, dcrx_cdr3_network_stats_t *stats_out) try {
  if (m >= MAX_NODES) return fail(DCRX_E_UNSUPPORTED, who, "2^30 or more nodes");
  if (distance != 1 && distance != 2) return fail(DCRX_E_INVALID, who, "the distance is 1 or 2");
  if (!metric_exists(metric)) return fail(DCRX_E_INVALID, who, "the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN");
  if (stats_out) { *stats_out = dcrx_cdr3_network_stats_t{}; stats_out->nodes_in = m; }
  if (adj_need_out) *adj_need_out = 0;
  if (adj_off_out) adj_off_out[0] = 0;
  if (!m) return 0;
  if (!cls || !off || !weight || !degree_out || !cluster_of_out || !head_out || !n_nodes_out || !weight_out || (adj_cap && !adj_out))
    return fail(DCRX_E_INVALID, who, "null argument");
  uint64_t out_of_reach = 0;
  for (uint64_t k = 0; k < m; k++) {
    if (off[k + 1] < off[k]) return fail(DCRX_E_INVALID, who, "offsets go backwards");
    if (!in_reach(off[k + 1] - off[k])) out_of_reach++;
  }
  const uint64_t text_bytes = off[m] - off[0];
  if (text_bytes && !text) return fail(DCRX_E_INVALID, who, "text is null");
  const uint32_t m32 = (uint32_t)m;
  int rc;
  size_t cub_bytes = 0;
  if ((rc = exclusive_sum_bytes<uint32_t>(m, &cub_bytes))) return rc;

  Pool P;
  Work W;
  uint32_t *d_cls, *d_degree, *d_label[2], *d_changed, *d_members, *d_ishead, *d_slot, *d_heads, *d_kept, *d_nn, *d_of;
  uint64_t *d_off, *d_weight, *d_adj_off, *d_need, *d_wout;
  unsigned long long *d_total;
  uint8_t *d_text, *d_cub;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_cls, m); P.get(&d_off, m + 1); P.get(&d_text, text_bytes); P.get(&d_weight, m); P.get(&d_degree, m);
    P.get(&d_adj_off, m + 1); P.get(&d_need, 1); P.get(&d_cub, cub_bytes); P.get(&d_label[0], m);
    P.get(&d_label[1], m); P.get(&d_changed, 1); P.get(&d_total, m); P.get(&d_members, m); P.get(&d_ishead, m); P.get(&d_slot, m);
    P.get(&d_heads, m); P.get(&d_kept, 1); P.get(&d_nn, m); P.get(&d_wout, m); P.get(&d_of, m);
    if ((rc = W.carve(P, m, metric)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_spans(m, off, text, d_off, d_text)) || (rc = to_device(d_cls, cls, m)) || (rc = to_device(d_weight, weight, m))) return rc;
  const Nodes N{d_cls, d_off, d_text, text_bytes};

  // the degree pass, then an adjacency of exactly the entries it takes
  if ((rc = run_degrees(N, m, distance, metric, d_degree, d_adj_off, d_need, W, nullptr))) return rc;
  uint64_t need = 0;
  if ((rc = to_host(&need, d_need, 1))) return rc;
  if (adj_need_out) *adj_need_out = need;
  dcrx::DevBuf<uint32_t> d_adj;
  if (d_adj.alloc(std::max<uint64_t>(need, 1))) return fail(DCRX_E_NOMEM, who, "the adjacency does not fit the device's memory");
  if (need && (rc = run_write(m, distance, metric, d_adj_off, d_adj.get(), need, W, nullptr))) return rc;

  // components: rounds of the neighbourhood's smallest label, then the labels followed to their ends
  cdr3net_label_init_kernel<<<grid_for(m), BLOCK>>>(m32, d_label[0]);
  HIP_TRY(hipGetLastError());
  for (uint32_t changed = need ? 1u : 0u; changed;) {
    HIP_TRY(hipMemsetAsync(d_changed, 0, 4, nullptr));
    cdr3net_min_kernel<<<grid_for(m), BLOCK>>>(d_label[0], d_adj_off, d_adj, m32, d_label[1], d_changed);
    HIP_TRY(hipGetLastError());
    cdr3net_jump_kernel<<<grid_for(m), BLOCK>>>(d_label[1], m32, d_label[0]);
    HIP_TRY(hipGetLastError());
    if ((rc = to_host(&changed, d_changed, 1))) return rc;      // (the round's one synchronisation)
  }

  // totals onto the heads; the heads in rank order are the rows
  const Scratch cub{d_cub, cub_bytes};
  HIP_TRY(hipMemsetAsync(d_total, 0, m * 8, nullptr));
  HIP_TRY(hipMemsetAsync(d_members, 0, m * 4, nullptr));
  cdr3net_totals_kernel<<<grid_for(m), BLOCK>>>(d_label[0], d_weight, m32, d_total, d_members, d_ishead);
  HIP_TRY(hipGetLastError());
  if ((rc = compact(cub, d_ishead, d_slot, m32, PutIndex{d_heads}, d_kept, nullptr))) return rc;
  uint32_t c = 0;
  if ((rc = to_host(&c, d_kept, 1))) return rc;
  cdr3net_rows_kernel<<<grid_for(c), BLOCK>>>(d_heads, c, d_total, d_members, d_nn, d_wout);
  HIP_TRY(hipGetLastError());
  cdr3net_cluster_of_kernel<<<grid_for(m), BLOCK>>>(d_label[0], d_slot, m32, d_of);
  HIP_TRY(hipGetLastError());

  if ((rc = to_host(degree_out, d_degree, m)) || (rc = to_host(cluster_of_out, d_of, m)) || (rc = to_host(head_out, d_heads, c)) ||
      (rc = to_host(n_nodes_out, d_nn, c)) || (rc = to_host(weight_out, d_wout, c))) return rc;
  if (adj_off_out) {
    if ((rc = to_host(adj_off_out, d_adj_off, m + 1))) return rc;
    if (adj_out && need <= adj_cap && (rc = to_host(adj_out, d_adj.get(), need))) return rc;
  }
  if (stats_out) {
    stats_out->out_of_reach = out_of_reach;
    stats_out->edges = need / 2;
    stats_out->clusters_out = c;
    for (uint32_t r = 0; r < c; r++) {
      if (n_nodes_out[r] == 1) stats_out->singletons++;
      stats_out->largest_cluster = std::max<uint64_t>(stats_out->largest_cluster, n_nodes_out[r]);
    }
    for (uint64_t k = 0; k < m; k++) stats_out->largest_degree = std::max<uint64_t>(stats_out->largest_degree, degree_out[k]);
  }
  return (int64_t)c;
} catch (const std::exception &e) {      // (a message that could not be built)
  return set_err(DCRX_E_NOMEM, e.what());
}

// the Levenshtein distance of two byte strings of any length (the edge file's column): a plain two-row table
uint64_t host_levenshtein(const char *a, uint64_t la, const char *b, uint64_t lb) {
  std::vector<uint64_t> prev(lb + 1), cur(lb + 1);
  for (uint64_t j = 0; j <= lb; j++) prev[j] = j;
  for (uint64_t i = 1; i <= la; i++) {
    cur[0] = i;
    for (uint64_t j = 1; j <= lb; j++) cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1] ? 1u : 0u)});
    prev.swap(cur);
  }
  return prev[lb];
}

int64_t format_edges(const char *who, uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                     uint32_t metric, char *out, uint64_t out_cap) try {
  static const char header[] = "a\tb\tdistance\n";
  if (!metric_exists(metric)) return fail(DCRX_E_INVALID, who, "the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN");
  if (m && (!adj_off || !off || (adj_off[m] && !adj))) return fail(DCRX_E_INVALID, who, "null argument");
  dcrx::TextOut T{out, out_cap};
  T.put(header, sizeof header - 1);
  for (uint64_t a = 0; a < m; a++) {
    if (adj_off[a + 1] < adj_off[a]) return fail(DCRX_E_INVALID, who, "adjacency offsets go backwards");
    for (uint64_t k = adj_off[a]; k < adj_off[a + 1]; k++) {
      const uint64_t b = adj[k];
      if (b >= m) return fail(DCRX_E_INVALID, who, "a neighbour outside the nodes");
      if (b <= a) continue;
      const uint64_t la = off[a + 1] - off[a], lb = off[b + 1] - off[b];
      unsigned long long d = 0;
      if (metric == METRIC_LEVENSHTEIN) {
        d = host_levenshtein(text + off[a], la, text + off[b], lb);
      } else {
        if (la != lb) return fail(DCRX_E_INVALID, who, "an edge between strings of two lengths");
        for (uint64_t p = 0; p < la; p++) d += text[off[a] + p] != text[off[b] + p];
      }
      T.unum(a); T.put("\t", 1); T.unum(b); T.put("\t", 1); T.unum(d); T.put("\n", 1);
    }
  }
  return (int64_t)T.at;
} catch (const std::exception &e) {      // (host_levenshtein's rows, a message)
  return set_err(DCRX_E_NOMEM, e.what());
}

}  // namespace

extern "C" {

uint64_t dcrx_cdr3net_metric_work_bytes(uint64_t m, uint64_t text_bytes, uint32_t metric) {
  (void)text_bytes;      // (the work space holds per-node keys, ranks and packed strings: the text's bytes do not enter it)
  Pool P;
  Work W;
  if (m >= MAX_NODES || !metric_exists(metric) || W.carve(P, m, metric) != DCRX_OK) return 0;
  return P.bytes();
}

uint64_t dcrx_cdr3net_work_bytes(uint64_t m, uint64_t text_bytes) { return dcrx_cdr3net_metric_work_bytes(m, text_bytes, METRIC_HAMMING); }

int dcrx_cdr3_neighbours_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                                uint32_t distance, uint32_t *d_degree, uint64_t *d_adj_off, uint32_t *d_adj, uint64_t adj_cap,
                                uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream) {
  return neighbours_device("dcrx_cdr3_neighbours_device", m, d_class, d_off, d_text, text_bytes, distance, METRIC_HAMMING, d_degree,
                           d_adj_off, d_adj, adj_cap, d_adj_need, d_work, work_bytes, hip_stream);
}

int dcrx_cdr3_neighbours_metric_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                                       uint32_t distance, uint32_t metric, uint32_t *d_degree, uint64_t *d_adj_off, uint32_t *d_adj,
                                       uint64_t adj_cap, uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream) {
  return neighbours_device("dcrx_cdr3_neighbours_metric_device", m, d_class, d_off, d_text, text_bytes, distance, metric, d_degree,
                           d_adj_off, d_adj, adj_cap, d_adj_need, d_work, work_bytes, hip_stream);
}

int64_t dcrx_cdr3_network(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                          uint32_t distance, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out, uint32_t *n_nodes_out,
                          uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint64_t adj_cap, uint64_t *adj_need_out,
                          dcrx_cdr3_network_stats_t *stats_out) {
  return network("dcrx_cdr3_network", m, cls, off, text, weight, distance, METRIC_HAMMING, degree_out, cluster_of_out, head_out,
                 n_nodes_out, weight_out, adj_off_out, adj_out, adj_cap, adj_need_out, stats_out);
}

int64_t dcrx_cdr3_network_metric(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                                 uint32_t distance, uint32_t metric, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out,
                                 uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint64_t adj_cap,
                                 uint64_t *adj_need_out, dcrx_cdr3_network_stats_t *stats_out) {
  return network("dcrx_cdr3_network_metric", m, cls, off, text, weight, distance, metric, degree_out, cluster_of_out, head_out,
                 n_nodes_out, weight_out, adj_off_out, adj_out, adj_cap, adj_need_out, stats_out);
}

int64_t dcrx_format_cdr3_clusters(uint64_t m, const uint32_t *v_idx, const uint32_t *j_idx, uint32_t n_v, const char *v_calls,
                                  const uint32_t *v_call_off, uint32_t n_j, const char *j_calls, const uint32_t *j_call_off,
                                  const uint64_t *off, const char *text, const uint64_t *weight, const uint32_t *cluster_of,
                                  uint64_t n_clusters, const uint32_t *n_nodes, const uint64_t *cluster_weight, const uint32_t *degree,
                                  char *out, uint64_t out_cap) {
  static const char header[] = "clonotype\tv_call\tj_call\tjunction_aa\tduplicate_count\tcluster\tcluster_size\tcluster_duplicate_count\tdegree\n";
  if (m && (!v_idx || !j_idx || !v_calls || !v_call_off || !j_calls || !j_call_off || !off || !weight || !cluster_of || !n_nodes ||
            !cluster_weight || !degree))
    return set_err(DCRX_E_INVALID, "dcrx_format_cdr3_clusters: null argument");
  dcrx::TextOut T{out, out_cap};
  T.put(header, sizeof header - 1);
  for (uint64_t i = 0; i < m; i++) {
    const uint32_t vi = v_idx[i], ji = j_idx[i], c = cluster_of[i];
    if (vi >= n_v || ji >= n_j) return set_err(DCRX_E_INVALID, "dcrx_format_cdr3_clusters: a gene outside its table");
    if (c >= n_clusters) return set_err(DCRX_E_INVALID, "dcrx_format_cdr3_clusters: a cluster outside the rows");
    if (off[i + 1] < off[i]) return set_err(DCRX_E_INVALID, "dcrx_format_cdr3_clusters: offsets go backwards");
    T.unum(i); T.put("\t", 1);
    T.put_span(v_calls, v_call_off, vi); T.put("\t", 1);
    T.put_span(j_calls, j_call_off, ji); T.put("\t", 1);
    T.put_span(text, off, i); T.put("\t", 1);
    T.unum(weight[i]); T.put("\t", 1);
    T.unum(c); T.put("\t", 1);
    T.unum(n_nodes[c]); T.put("\t", 1);
    T.unum(cluster_weight[c]); T.put("\t", 1);
    T.unum(degree[i]); T.put("\n", 1);
  }
  return (int64_t)T.at;
}

int64_t dcrx_format_cdr3_edges(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                               char *out, uint64_t out_cap) {
  return format_edges("dcrx_format_cdr3_edges", m, adj_off, adj, off, text, METRIC_HAMMING, out, out_cap);
}

int64_t dcrx_format_cdr3_edges_metric(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                                      uint32_t metric, char *out, uint64_t out_cap) {
  return format_edges("dcrx_format_cdr3_edges_metric", m, adj_off, adj, off, text, metric, out, out_cap);
}

}  // extern "C"


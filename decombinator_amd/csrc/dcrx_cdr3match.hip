// dcrx_cdr3match.hip — match (`match`): which queries (a sample's clonotypes) are the same as, or one or two residues from, a
// target (an entry of a database, or of another sample); include/dcrx.h "match" holds the contract, dcrx_cdr3net_core.h the
// per-node and per-pair code (the CDR3 network's), dcrx_cdr3match_core.h the walk's look-ups, dcrx_cdr3walk.h the kernels
// that prepare and walk the tables (the network's too).
//
// The index (dcrx_cdr3_index_create), once per database: keys, then per bucket order — (class, length) for the Hamming walk,
// class alone for the Levenshtein walk — a stable radix sort of (key, rank) and the gather of the packed strings (and, in the
// class order, of the presence masks).  It stays on the device.
// The primitive (dcrx_cdr3_match_device), all on the caller's stream and in the caller's work space:
//   keys, sort, gather   the queries, as the network prepares its nodes (cdr3_keys_kernel, cdr3_gather_kernel<false, PRES>)
//   degrees  cdr3_walk_kernel<false, Bipartite, Pair>: a block of 256 consecutive sorted queries finds the first target at or
//            above its first query's bucket (a binary search over the index's sorted keys, the same for every lane) and walks
//            the targets from there until a tile starts behind its last query's bucket.  A bucket's targets are in rank
//            order: a query's hits come in ascending rank, with no atomics
//   scan     an exclusive sum of the degrees in rank order: hit_off, whose end is the need
//   write    cdr3_walk_kernel<true, Bipartite, Pair>: the same walk writes every hit's rank at its exact offset
// The host entry (dcrx_cdr3_match_run) runs those two halves around the hits' allocation, then the totals: a lane per query
// adds its row's hits onto the targets (integer atomics, results unused).
// The weighted metric (dcrx_cdr3_match_weighted_*; include/dcrx.h "match, weighted") is the same walk over the Levenshtein
// walk's class-order arrays with Weighted (weighted_within, dcrx_cdr3w_core.h) as its pair test; its entries live in this
// file because the index, the work space, the handle and the two halves around the walk are this file's own.
// The profile (dcrx_cdr3_profile_weighted_*; include/dcrx.h "profile, weighted") is the weighted walk once more, at the top of a
// ladder of radii, with a histogram of the hits' distances per query for a sink (Profile, dcrx_cdr3walk.h): one pass, no scan.
// The tally (dcrx_cdr3_tally_weighted_*; include/dcrx.h "tally, weighted") is that walk with a radius per TARGET (WeightedPer) and
// totals per target for a sink (Tally): accumulators by sorted position in the work space, zeroed in front of the walk, and
// cdr3_tally_scatter_kernel behind it, which writes every target's cell by rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_cdr3walk.h"
#include "dcrx_text.h"

using dcrx::set_err;
using namespace dcrx_cdr3walk;

namespace {

// the host entry's: every hit of query i onto its target (the results of the atomics are not read)
__global__ __launch_bounds__(BLOCK) void cdr3match_totals_kernel(const uint64_t *__restrict__ hit_off, const uint32_t *__restrict__ hit,
                                                                 const uint64_t *__restrict__ weight, uint32_t n_q,
                                                                 uint32_t *__restrict__ t_queries, unsigned long long *__restrict__ t_weight) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n_q) return;
  const unsigned long long w = weight[i];
  for (uint64_t k = hit_off[i], end = hit_off[i + 1]; k < end; k++) {
    const uint32_t j = hit[k];
    atomicAdd(&t_queries[j], 1u);
    atomicAdd(&t_weight[j], w);
  }
}

// D = 0 is byte equality: the (class, length) buckets and the Hamming test serve it under either metric
bool walks_lev(uint32_t distance, uint32_t metric) { return metric == METRIC_LEVENSHTEIN && distance > 0; }

// the packed strings in sorted order, and (pres != null) the presence masks
int gather(const Nodes &N, uint64_t n, const uint32_t *idx, uint4 *sj, uint32_t *pres, hipStream_t s) {
  if (pres) cdr3_gather_kernel<false, true><<<grid_for(n), BLOCK, 0, s>>>(N, (uint32_t)n, nullptr, idx, sj, nullptr, pres);
  else cdr3_gather_kernel<false, false><<<grid_for(n), BLOCK, 0, s>>>(N, (uint32_t)n, nullptr, idx, sj, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// ---- work space of the primitive: the degree pass leaves the sorted queries there for the write pass
struct Work {
  uint64_t *key[2];
  uint32_t *idx[2];
  uint4 *sj;
  uint64_t *deg64;
  Scratch cub;
  uint32_t *pres;      // (the Levenshtein walk's; null under Hamming)
  int carve(Pool &P, uint64_t n, uint32_t metric) {
    size_t cub_bytes = 0;
    const uint64_t k = std::max<uint64_t>(n, 1);
    int rc;
    if ((rc = sort_pairs_bytes<uint32_t>(k, KEY_BITS, &cub_bytes)) || (rc = exclusive_sum_bytes<uint64_t>(k, &cub_bytes))) return rc;
    P.get(&key[0], n); P.get(&key[1], n); P.get(&idx[0], n); P.get(&idx[1], n); P.get(&sj, 2 * n); P.get(&deg64, n); P.get(&cub, cub_bytes);
    pres = nullptr;
    if (metric == METRIC_LEVENSHTEIN) P.get(&pres, n);
    return DCRX_OK;
  }
  Sorted queries(uint64_t n, bool lev) const { return Sorted{key[1], idx[1], sj, lev ? pres : nullptr, (uint32_t)n}; }
};

}  // namespace

// the targets in both bucket orders, in one allocation
struct dcrx_cdr3_index {
  uint64_t m = 0, out_of_reach = 0, bytes = 0;
  int device = -1;
  Pool mem;
  uint64_t *key[2] = {nullptr, nullptr};      // [0]: by (class, length); [1]: by class
  uint32_t *idx[2] = {nullptr, nullptr};
  uint4 *sj[2] = {nullptr, nullptr};
  uint32_t *pres = nullptr;                   // of the class order
  void carve() {
    for (int o = 0; o < 2; o++) { mem.get(&key[o], m); mem.get(&idx[o], m); mem.get(&sj[o], 2 * m); }
    mem.get(&pres, m);
  }
  Sorted targets(bool lev) const { return Sorted{key[lev], idx[lev], sj[lev], lev ? pres : nullptr, (uint32_t)m}; }
};

struct dcrx_cdr3_match {
  dcrx_cdr3_match_stats_t stats{};
  std::vector<uint32_t> degree, hit, t_queries;
  std::vector<uint64_t> hit_off, t_weight;
  bool weighted = false;
  std::vector<uint32_t> hit_dist;      // (a weighted handle's)
};

namespace {

int build_index(dcrx_cdr3_index &I, const uint32_t *cls, const uint64_t *off, const char *text) {
  const uint64_t m = I.m, text_bytes = off[m] - off[0];
  int rc;
  I.carve();
  I.bytes = I.mem.bytes();
  if ((rc = I.mem.allocate())) return rc;
  I.carve();
  // what only the build needs: the nodes, the unsorted keys and ranks, hipCUB's scratch
  Pool P;
  uint32_t *d_cls, *d_idx;
  uint64_t *d_off, *d_key;
  uint8_t *d_text;
  Scratch cub;
  size_t cub_bytes = 0;
  if ((rc = sort_pairs_bytes<uint32_t>(m, KEY_BITS, &cub_bytes))) return rc;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_cls, m); P.get(&d_off, m + 1); P.get(&d_text, text_bytes); P.get(&d_key, m); P.get(&d_idx, m); P.get(&cub, cub_bytes);
    if (pass == 0 && (rc = P.allocate())) return rc;
  }
  if ((rc = upload_spans(m, off, text, d_off, d_text)) || (rc = to_device(d_cls, cls, m))) return rc;
  const Nodes N{d_cls, d_off, d_text, text_bytes};
  for (int o = 0; o < 2; o++) {
    uint64_t *const key[2] = {d_key, I.key[o]};
    uint32_t *const idx[2] = {d_idx, I.idx[o]};
    if ((rc = sorted_keys(N, m, key, idx, cub, o ? (int)LEN_BITS : 0, o == 0, nullptr)) ||
        (rc = gather(N, m, I.idx[o], I.sj[o], o ? I.pres : nullptr, nullptr))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(nullptr));      // (the build's buffers go out of scope)
  return DCRX_OK;
}

// one pass of the walk (wc: the weighted walk's cost, and then `limit` is the radius and `lev` is set: the class order, without
// the presence masks)
template <bool WRITE>
int run_walk(const dcrx_cdr3_index &I, uint64_t n, uint32_t limit, bool lev, const CostArg *wc, const Out &O, const Work &W, hipStream_t s) {
  const Sorted Q = W.queries(n, lev), T = I.targets(lev);
  if (!wc) return walk<WRITE>(Q, T, Bipartite{}, limit, lev, O, s);
  cdr3_walk_kernel<WRITE><<<grid_for(n), BLOCK, 0, s>>>(Q, T, Bipartite{}, Weighted{*wc, limit}, O);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// keys, sort, gather of the queries, the degree pass, the scan and the need
int run_degrees(const dcrx_cdr3_index &I, const Nodes &N, uint64_t n, uint32_t limit, bool lev, const CostArg *wc, uint32_t *d_degree,
                uint64_t *d_hit_off, uint64_t *d_need, const Work &W, hipStream_t s) {
  int rc;
  if ((rc = sorted_keys(N, n, W.key, W.idx, W.cub, lev ? (int)LEN_BITS : 0, true, s)) ||
      (rc = gather(N, n, W.idx[1], W.sj, lev ? W.pres : nullptr, s)) ||
      (rc = run_walk<false>(I, n, limit, lev, wc, Out{d_degree, W.deg64, nullptr, nullptr, nullptr, 0}, W, s)) ||
      (rc = exclusive_sum(W.cub, W.deg64, d_hit_off, n, s))) return rc;
  cdr3_need_kernel<<<1, 64, 0, s>>>(W.deg64, d_hit_off, (uint32_t)n, d_need);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

int run_write(const dcrx_cdr3_index &I, uint64_t n, uint32_t limit, bool lev, const CostArg *wc, const uint64_t *d_hit_off, uint32_t *d_hit,
              uint32_t *d_hit_dist, uint64_t hit_cap, const Work &W, hipStream_t s) {
  return run_walk<true>(I, n, limit, lev, wc, Out{nullptr, nullptr, d_hit_off, d_hit, d_hit_dist, hit_cap}, W, s);
}

// the device entry under any metric, behind the entry's own refusals (wc: the weighted walk's cost, `limit` its radius, and
// the carve is the Hamming walk's: no presence masks)
int match_device(const char *who, const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off, const char *d_text,
                 uint64_t text_bytes, uint32_t limit, uint32_t metric, const CostArg *wc, uint32_t *d_degree, uint64_t *d_hit_off,
                 uint32_t *d_hit, uint32_t *d_hit_dist, uint64_t hit_cap, uint64_t *d_hit_need, void *d_work, uint64_t work_bytes,
                 hipStream_t s) {
  auto fail = [&](const char *what) { return set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  if (m_q && (!d_class || !d_off || !d_degree || !d_hit_off || !d_work || (text_bytes && !d_text) || (hit_cap && !d_hit)))
    return fail("null argument");
  dcrx::DeviceGuard on(I->device);      // (the index's device for the launches, the caller's again behind them; no index memory: neither)
  if (!m_q || !I->m) {      // nothing can hit: no launch
    if (d_hit_need) HIP_TRY(hipMemsetAsync(d_hit_need, 0, sizeof(uint64_t), s));
    if (d_hit_off) HIP_TRY(hipMemsetAsync(d_hit_off, 0, (m_q + 1) * sizeof(uint64_t), s));
    if (m_q) HIP_TRY(hipMemsetAsync(d_degree, 0, m_q * sizeof(uint32_t), s));
    return DCRX_OK;
  }
  if ((uintptr_t)d_work % ALIGN) return fail("the work space is not 256-byte aligned");
  Pool P(d_work);
  Work W;
  int rc = W.carve(P, m_q, metric);
  if (rc) return rc;
  if (work_bytes < P.bytes())
    return fail(wc ? "the work space is smaller than dcrx_cdr3_match_weighted_work_bytes(m_q, text_bytes)"
                   : "the work space is smaller than dcrx_cdr3_match_work_bytes(m_q, text_bytes, metric)");
  const Nodes N{d_class, d_off, reinterpret_cast<const uint8_t *>(d_text), text_bytes};
  const bool lev = wc || walks_lev(limit, metric);
  if ((rc = run_degrees(*I, N, m_q, limit, lev, wc, d_degree, d_hit_off, d_hit_need, W, s))) return rc;
  if (!d_hit || !hit_cap) return DCRX_OK;
  return run_write(*I, m_q, limit, lev, wc, d_hit_off, d_hit, d_hit_dist, hit_cap, W, s);
}

// what every entry refuses of (index, m_q, distance, metric)
int refuse(const char *who, const dcrx_cdr3_index_t *I, uint64_t m_q, uint32_t distance, uint32_t metric) {
  auto fail = [&](int code, const char *what) { return set_err(code, (std::string(who) + ": " + what).c_str()); };
  if (!I) return fail(DCRX_E_INVALID, "null index");
  if (m_q >= MAX_NODES) return fail(DCRX_E_UNSUPPORTED, "2^30 or more queries");
  if (distance > 2) return fail(DCRX_E_INVALID, "the distance is 0, 1 or 2");
  if (!metric_exists(metric)) return fail(DCRX_E_INVALID, "the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN");
  return DCRX_OK;
}

int run_match(const dcrx_cdr3_index &I, uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
              uint32_t distance, uint32_t metric, const CostArg *wc, dcrx_cdr3_match &M) {
  const uint64_t text_bytes = off[m] - off[0], mt = I.m;
  const bool lev = wc || walks_lev(distance, metric);
  int rc;
  Pool P;
  Work W;
  uint32_t *d_cls, *d_degree, *d_tq;
  uint64_t *d_off, *d_weight, *d_hit_off, *d_need;
  unsigned long long *d_tw;
  uint8_t *d_text;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_cls, m); P.get(&d_off, m + 1); P.get(&d_text, text_bytes); P.get(&d_weight, m); P.get(&d_degree, m);
    P.get(&d_hit_off, m + 1); P.get(&d_need, 1); P.get(&d_tq, mt); P.get(&d_tw, mt);
    if ((rc = W.carve(P, m, metric)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_spans(m, off, text, d_off, d_text)) || (rc = to_device(d_cls, cls, m)) || (rc = to_device(d_weight, weight, m))) return rc;
  const Nodes N{d_cls, d_off, d_text, text_bytes};

  // the degree pass, then exactly the hits it sized
  if ((rc = run_degrees(I, N, m, distance, lev, wc, d_degree, d_hit_off, d_need, W, nullptr))) return rc;
  uint64_t need = 0;
  if ((rc = to_host(&need, d_need, 1))) return rc;
  dcrx::DevBuf<uint32_t> d_hit, d_dist;
  if (d_hit.alloc(std::max<uint64_t>(need, 1)) || (wc && d_dist.alloc(std::max<uint64_t>(need, 1)))) return set_err(DCRX_E_NOMEM, "dcrx_cdr3_match_run: the hits do not fit the device's memory");
  M.hit.resize(need);
  if (wc) M.hit_dist.resize(need);
  HIP_TRY(hipMemsetAsync(d_tq, 0, mt * sizeof *d_tq, nullptr));
  HIP_TRY(hipMemsetAsync(d_tw, 0, mt * sizeof *d_tw, nullptr));
  if (need) {
    if ((rc = run_write(I, m, distance, lev, wc, d_hit_off, d_hit.get(), wc ? d_dist.get() : nullptr, need, W, nullptr))) return rc;
    cdr3match_totals_kernel<<<grid_for(m), BLOCK>>>(d_hit_off, d_hit.get(), d_weight, (uint32_t)m, d_tq, d_tw);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = to_host(M.degree.data(), d_degree, m)) || (rc = to_host(M.hit_off.data(), d_hit_off, m + 1)) ||
      (rc = to_host(M.hit.data(), d_hit.get(), need)) || (rc = to_host(M.t_queries.data(), d_tq, mt)) ||
      (rc = to_host(M.t_weight.data(), reinterpret_cast<const uint64_t *>(d_tw), mt))) return rc;
  if (wc && (rc = to_host(M.hit_dist.data(), d_dist.get(), need))) return rc;
  return DCRX_OK;
}

// the host entry under any metric, behind the entry's own refusals (wc: the weighted walk's cost, `distance` its radius)
int run_entry(const char *who, const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *cls, const uint64_t *off, const char *text,
              const uint64_t *weight, uint32_t distance, uint32_t metric, const CostArg *wc, dcrx_cdr3_match_t **match_out) {
  auto fail = [&](int code, const char *what) { return set_err(code, (std::string(who) + ": " + what).c_str()); };
  int rc;
  if (m_q && (!cls || !off || !weight)) return fail(DCRX_E_INVALID, "null argument");
  uint64_t out_of_reach = 0, total = 0;
  for (uint64_t k = 0; k < m_q; k++) {
    if (off[k + 1] < off[k]) return fail(DCRX_E_INVALID, "offsets go backwards");
    if (!in_reach(off[k + 1] - off[k])) out_of_reach++;
    if (__builtin_add_overflow(total, weight[k], &total))
      return fail(DCRX_E_UNSUPPORTED, "the sum of the query weights is 2^64 or more");
  }
  if (m_q && off[m_q] > off[0] && !text) return fail(DCRX_E_INVALID, "text is null");
  dcrx_cdr3_match *M = new dcrx_cdr3_match();
  struct Drop {      // (released on every path that does not hand it over)
    dcrx_cdr3_match *p;
    ~Drop() { delete p; }
  } drop{M};
  M->weighted = wc != nullptr;
  M->stats.queries = m_q;
  M->stats.targets = I->m;
  M->stats.queries_out_of_reach = out_of_reach;
  M->stats.targets_out_of_reach = I->out_of_reach;
  M->degree.assign(m_q, 0);
  M->hit_off.assign(m_q + 1, 0);
  M->t_queries.assign(I->m, 0);
  M->t_weight.assign(I->m, 0);
  if (m_q && I->m) {
    dcrx::DeviceGuard on(I->device);
    if ((rc = run_match(*I, m_q, cls, off, text, weight, distance, metric, wc, *M))) return rc;
  }
  M->stats.hits = M->hit.size();
  for (uint64_t k = 0; k < m_q; k++) {
    if (!M->degree[k]) continue;
    M->stats.queries_hit++;
    M->stats.queries_hit_weight += weight[k];
    M->stats.largest_degree = std::max<uint64_t>(M->stats.largest_degree, M->degree[k]);
  }
  for (uint32_t q : M->t_queries) M->stats.targets_hit += q != 0;
  drop.p = nullptr;
  *match_out = M;
  return DCRX_OK;
}

// ---- the profile (include/dcrx.h "profile, weighted"): the weighted walk at radius step * (bins - 1) with the Profile sink

// what both profile entries refuse of (index, m_q, cost, step, bins); the cost as the launch argument and the ladder's top
int refuse_profile(const char *who, const dcrx_cdr3_index_t *I, uint64_t m_q, const dcrx_cdr3_cost_t *cost, uint32_t step, uint32_t bins,
                   CostArg *wc, uint32_t *radius) {
  int rc = refuse(who, I, m_q, 0, METRIC_HAMMING);
  if (rc) return rc;
  if (const char *what = dcrx_cdr3profile::refuse_ladder(step, bins)) return set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str());
  *radius = step * (bins - 1);
  return refuse_cost(who, cost, *radius, wc);
}

// the profile's work space: the sorted queries and the sort's scratch (no degrees, no scan, no masks)
struct ProfileWork {
  uint64_t *key[2];
  uint32_t *idx[2];
  uint4 *sj;
  Scratch cub;
  int carve(Pool &P, uint64_t n) {
    size_t cub_bytes = 0;
    int rc;
    if ((rc = sort_pairs_bytes<uint32_t>(std::max<uint64_t>(n, 1), KEY_BITS, &cub_bytes))) return rc;
    P.get(&key[0], n); P.get(&key[1], n); P.get(&idx[0], n); P.get(&idx[1], n); P.get(&sj, 2 * n); P.get(&cub, cub_bytes);
    return DCRX_OK;
  }
  Sorted queries(uint64_t n) const { return Sorted{key[1], idx[1], sj, nullptr, (uint32_t)n}; }
};

// keys, sort and gather of the queries as the weighted match prepares them, then the one walk; every cell of d_profile is
// written (m_q > 0 and targets > 0 here)
int run_profile(const dcrx_cdr3_index &I, const Nodes &N, uint64_t n, const CostArg &wc, uint32_t radius, uint32_t step, uint32_t bins,
                uint32_t *d_profile, const ProfileWork &W, hipStream_t s) {
  int rc;
  if ((rc = sorted_keys(N, n, W.key, W.idx, W.cub, (int)LEN_BITS, true, s)) || (rc = gather(N, n, W.idx[1], W.sj, nullptr, s))) return rc;
  const size_t hist_bytes = (size_t)bins * BLOCK * sizeof(uint32_t);
  cdr3_walk_kernel<false><<<grid_for(n), BLOCK, hist_bytes, s>>>(W.queries(n), I.targets(true), Bipartite{}, Weighted{wc, radius},
                                                                 Profile{d_profile, step, bins});
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// ---- the tally (include/dcrx.h "tally, weighted"): the weighted walk with a bound per target and the Tally sink

// the accumulators by sorted position onto the outputs by rank: every cell of the two is written
__global__ __launch_bounds__(BLOCK) void cdr3_tally_scatter_kernel(const uint32_t *__restrict__ idx, uint32_t n, const uint32_t *__restrict__ acc_count,
                                                                   const unsigned long long *__restrict__ acc_weight,
                                                                   uint32_t *__restrict__ t_count, uint64_t *__restrict__ t_weight) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  const uint32_t j = idx[p];
  t_count[j] = acc_count[p];
  t_weight[j] = acc_weight[p];
}

// the tally's work space: the profile's, and the two accumulators per target
struct TallyWork {
  ProfileWork q;
  uint32_t *acc_count;
  unsigned long long *acc_weight;
  int carve(Pool &P, uint64_t n, uint64_t m_t) {
    const int rc = q.carve(P, n);
    if (rc) return rc;
    P.get(&acc_count, m_t); P.get(&acc_weight, m_t);
    return DCRX_OK;
  }
};

// what both tally entries refuse of (index, m_q, cost) and of their outputs; the cost as the launch argument
int refuse_tally(const char *who, const dcrx_cdr3_index_t *I, uint64_t m_q, const dcrx_cdr3_cost_t *cost, const void *t_count, const void *t_weight,
                 const void *q_degree, CostArg *wc) {
  int rc = refuse(who, I, m_q, 0, METRIC_HAMMING);
  if (rc || (rc = refuse_cost(who, cost, 0, wc))) return rc;
  if ((I->m && (!t_count || !t_weight)) || (m_q && !q_degree)) return set_err(DCRX_E_INVALID, (std::string(who) + ": null output").c_str());
  return DCRX_OK;
}

// keys, sort and gather of the queries as the weighted match prepares them, the accumulators zeroed, the one walk and the
// scatter; every cell of the three outputs is written (m_q > 0 and targets > 0 here)
int run_tally(const dcrx_cdr3_index &I, const Nodes &N, uint64_t n, const uint64_t *d_weight, const CostArg &wc, const uint32_t *d_radius,
              uint32_t *d_t_count, uint64_t *d_t_weight, uint32_t *d_q_degree, const TallyWork &W, hipStream_t s) {
  int rc;
  if ((rc = sorted_keys(N, n, W.q.key, W.q.idx, W.q.cub, (int)LEN_BITS, true, s)) || (rc = gather(N, n, W.q.idx[1], W.q.sj, nullptr, s))) return rc;
  HIP_TRY(hipMemsetAsync(W.acc_count, 0, I.m * sizeof *W.acc_count, s));
  HIP_TRY(hipMemsetAsync(W.acc_weight, 0, I.m * sizeof *W.acc_weight, s));
  const Sorted T = I.targets(true);
  cdr3_walk_kernel<false><<<grid_for(n), BLOCK, 0, s>>>(W.q.queries(n), T, Bipartite{}, WeightedPer{wc, d_radius},
                                                        Tally{d_weight, W.acc_count, W.acc_weight, d_q_degree});
  HIP_TRY(hipGetLastError());
  cdr3_tally_scatter_kernel<<<grid_for(I.m), BLOCK, 0, s>>>(T.idx, T.n, W.acc_count, W.acc_weight, d_t_count, d_t_weight);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// the matches text under any metric (cost: the weighted metric's, null otherwise)
int64_t format_matches(const char *who, uint64_t m_q, const uint64_t *hit_off, const uint32_t *hit, const uint32_t *v_idx, const uint32_t *j_idx,
                                 uint32_t n_v, const char *v_calls, const uint32_t *v_call_off, uint32_t n_j, const char *j_calls,
                                 const uint32_t *j_call_off, const uint64_t *q_off, const char *q_text, const uint64_t *weight, uint64_t m_t,
                                 const uint64_t *t_off, const char *t_text, const char *db_header, uint64_t db_header_bytes,
                                 const uint64_t *db_line_off, const char *db_lines, uint32_t metric, const dcrx_cdr3_cost_t *cost, char *out, uint64_t out_cap) {
  auto fail = [&](const char *what) { return set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  static const char header[] = "clonotype\tv_call\tj_call\tjunction_aa\tduplicate_count\ttarget\tdistance\t";
  if ((db_header_bytes && !db_header) ||
      (m_q && (!hit_off || !v_idx || !j_idx || !v_calls || !v_call_off || !j_calls || !j_call_off || !q_off || !weight)) ||
      (m_q && hit_off[m_q] && (!hit || !t_off || !db_line_off || !q_text || !t_text || !db_lines)))
    return fail("null argument");
  dcrx::TextOut T{out, out_cap};
  T.put(header, sizeof header - 1);
  T.put(db_header, db_header_bytes);
  T.put("\n", 1);
  for (uint64_t i = 0; i < m_q; i++) {
    if (hit_off[i + 1] < hit_off[i]) return fail("hit offsets go backwards");
    if (hit_off[i + 1] == hit_off[i]) continue;
    const uint32_t vi = v_idx[i], ji = j_idx[i];
    if (vi >= n_v || ji >= n_j) return fail("a gene outside its table");
    if (q_off[i + 1] < q_off[i]) return fail("offsets go backwards");
    const uint64_t lq = q_off[i + 1] - q_off[i];
    for (uint64_t k = hit_off[i]; k < hit_off[i + 1]; k++) {
      const uint64_t j = hit[k];
      if (j >= m_t) return fail("a hit outside the targets");
      if (t_off[j + 1] < t_off[j] || db_line_off[j + 1] < db_line_off[j])
        return fail("offsets go backwards");
      const uint64_t lt = t_off[j + 1] - t_off[j];
      unsigned long long d = 0;
      if (cost) {
        if (!in_reach(lq) || !in_reach(lt) || !host_letters(q_text + q_off[i], lq) || !host_letters(t_text + t_off[j], lt))
          return fail("a hit between strings out of the weighted metric's reach");
        d = host_weighted(q_text + q_off[i], lq, t_text + t_off[j], lt, *cost);
      } else if (metric == METRIC_LEVENSHTEIN) {
        d = dcrx::host_levenshtein(q_text + q_off[i], lq, t_text + t_off[j], lt);
      } else {
        if (lq != lt) return fail("a hit between strings of two lengths");
        for (uint64_t p = 0; p < lq; p++) d += q_text[q_off[i] + p] != t_text[t_off[j] + p];
      }
      T.unum(i); T.put("\t", 1);
      T.put_span(v_calls, v_call_off, vi); T.put("\t", 1);
      T.put_span(j_calls, j_call_off, ji); T.put("\t", 1);
      T.put_span(q_text, q_off, i); T.put("\t", 1);
      T.unum(weight[i]); T.put("\t", 1);
      T.unum(j); T.put("\t", 1);
      T.unum(d); T.put("\t", 1);
      T.put_span(db_lines, db_line_off, j); T.put("\n", 1);
    }
  }
  return (int64_t)T.at;
}

}  // namespace

extern "C" {

int dcrx_cdr3_index_create(uint64_t m_t, const uint32_t *cls, const uint64_t *off, const char *text, dcrx_cdr3_index_t **index_out) try {
  if (!index_out) return set_err(DCRX_E_INVALID, "dcrx_cdr3_index_create: null argument");
  *index_out = nullptr;
  if (m_t >= MAX_NODES) return set_err(DCRX_E_UNSUPPORTED, "dcrx_cdr3_index_create: 2^30 or more targets");
  if (m_t && (!cls || !off)) return set_err(DCRX_E_INVALID, "dcrx_cdr3_index_create: null argument");
  uint64_t out_of_reach = 0;
  for (uint64_t k = 0; k < m_t; k++) {
    if (off[k + 1] < off[k]) return set_err(DCRX_E_INVALID, "dcrx_cdr3_index_create: offsets go backwards");
    if (!in_reach(off[k + 1] - off[k])) out_of_reach++;
  }
  if (m_t && off[m_t] > off[0] && !text) return set_err(DCRX_E_INVALID, "dcrx_cdr3_index_create: text is null");
  dcrx_cdr3_index *I = new dcrx_cdr3_index();
  I->m = m_t;
  I->out_of_reach = out_of_reach;
  if (m_t) {
    int rc = DCRX_OK;
    if (hipGetDevice(&I->device) != hipSuccess) rc = set_err(DCRX_E_NOGPU, "dcrx_cdr3_index_create: no current device");
    if (!rc) rc = build_index(*I, cls, off, text);
    if (rc) { delete I; return rc; }
  }
  *index_out = I;
  return DCRX_OK;
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

void dcrx_cdr3_index_destroy(dcrx_cdr3_index_t *I) {
  if (!I) return;
  dcrx::DeviceGuard on(I->device);      // (what belongs to a device is released with that device current)
  delete I;
}

int dcrx_cdr3_index_info(const dcrx_cdr3_index_t *I, uint64_t *targets, uint64_t *out_of_reach, uint64_t *device_bytes) {
  if (!I) return set_err(DCRX_E_INVALID, "dcrx_cdr3_index_info: null handle");
  if (targets) *targets = I->m;
  if (out_of_reach) *out_of_reach = I->out_of_reach;
  if (device_bytes) *device_bytes = I->m ? I->bytes : 0;
  return DCRX_OK;
}

uint64_t dcrx_cdr3_match_work_bytes(uint64_t m_q, uint64_t text_bytes, uint32_t metric) {
  (void)text_bytes;      // (the work space holds per-query keys, ranks and packed strings: the text's bytes do not enter it)
  Pool P;
  Work W;
  if (m_q >= MAX_NODES || !metric_exists(metric) || W.carve(P, m_q, metric) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_match_device(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off, const char *d_text,
                           uint64_t text_bytes, uint32_t distance, uint32_t metric, uint32_t *d_degree, uint64_t *d_hit_off, uint32_t *d_hit,
                           uint64_t hit_cap, uint64_t *d_hit_need, void *d_work, uint64_t work_bytes, void *hip_stream) try {
  static const char who[] = "dcrx_cdr3_match_device";
  int rc = refuse(who, I, m_q, distance, metric);
  if (rc) return rc;
  return match_device(who, I, m_q, d_class, d_off, d_text, text_bytes, distance, metric, nullptr, d_degree, d_hit_off, d_hit, nullptr, hit_cap,
                      d_hit_need, d_work, work_bytes, (hipStream_t)hip_stream);
} catch (const std::exception &e) {      // (a message that could not be built)
  return set_err(DCRX_E_NOMEM, e.what());
}

int dcrx_cdr3_match_run(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *cls, const uint64_t *off, const char *text,
                        const uint64_t *weight, uint32_t distance, uint32_t metric, dcrx_cdr3_match_t **match_out) try {
  static const char who[] = "dcrx_cdr3_match_run";
  if (!match_out) return set_err(DCRX_E_INVALID, "dcrx_cdr3_match_run: null argument");
  *match_out = nullptr;
  int rc = refuse(who, I, m_q, distance, metric);
  if (rc) return rc;
  return run_entry(who, I, m_q, cls, off, text, weight, distance, metric, nullptr, match_out);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

void dcrx_cdr3_match_destroy(dcrx_cdr3_match_t *M) { delete M; }

int dcrx_cdr3_match_info(const dcrx_cdr3_match_t *M, uint64_t *queries, uint64_t *targets, uint64_t *hits, dcrx_cdr3_match_stats_t *stats) {
  if (!M) return set_err(DCRX_E_INVALID, "dcrx_cdr3_match_info: null handle");
  if (queries) *queries = M->degree.size();
  if (targets) *targets = M->t_queries.size();
  if (hits) *hits = M->hit.size();
  if (stats) *stats = M->stats;
  return DCRX_OK;
}

int dcrx_cdr3_match_export(const dcrx_cdr3_match_t *M, uint32_t *degree, uint64_t *hit_off, uint32_t *hit, uint32_t *t_queries,
                           uint64_t *t_weight) {
  if (!M) return set_err(DCRX_E_INVALID, "dcrx_cdr3_match_export: null handle");
  auto copy = [](auto *dst, const auto &src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0]));
  };
  copy(degree, M->degree); copy(hit_off, M->hit_off); copy(hit, M->hit); copy(t_queries, M->t_queries); copy(t_weight, M->t_weight);
  return DCRX_OK;
}

int64_t dcrx_format_cdr3_matches(uint64_t m_q, const uint64_t *hit_off, const uint32_t *hit, const uint32_t *v_idx, const uint32_t *j_idx,
                                 uint32_t n_v, const char *v_calls, const uint32_t *v_call_off, uint32_t n_j, const char *j_calls,
                                 const uint32_t *j_call_off, const uint64_t *q_off, const char *q_text, const uint64_t *weight, uint64_t m_t,
                                 const uint64_t *t_off, const char *t_text, const char *db_header, uint64_t db_header_bytes,
                                 const uint64_t *db_line_off, const char *db_lines, uint32_t metric, char *out, uint64_t out_cap) try {
  if (!metric_exists(metric))
    return set_err(DCRX_E_INVALID, "dcrx_format_cdr3_matches: the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN");
  return format_matches("dcrx_format_cdr3_matches", m_q, hit_off, hit, v_idx, j_idx, n_v, v_calls, v_call_off, n_j, j_calls, j_call_off, q_off, q_text, weight, m_t, t_off,
                        t_text, db_header, db_header_bytes, db_line_off, db_lines, metric, nullptr, out, out_cap);
} catch (const std::exception &e) {      // (host_levenshtein's rows)
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t dcrx_format_cdr3_matches_weighted(uint64_t m_q, const uint64_t *hit_off, const uint32_t *hit, const uint32_t *v_idx,
                                          const uint32_t *j_idx, uint32_t n_v, const char *v_calls, const uint32_t *v_call_off,
                                          uint32_t n_j, const char *j_calls, const uint32_t *j_call_off, const uint64_t *q_off,
                                          const char *q_text, const uint64_t *weight, uint64_t m_t, const uint64_t *t_off,
                                          const char *t_text, const char *db_header, uint64_t db_header_bytes, const uint64_t *db_line_off,
                                          const char *db_lines, const dcrx_cdr3_cost_t *cost, char *out, uint64_t out_cap) try {
  static const char who[] = "dcrx_format_cdr3_matches_weighted";
  const int rc = refuse_cost(who, cost, 0, nullptr);
  if (rc) return rc;
  return format_matches(who, m_q, hit_off, hit, v_idx, j_idx, n_v, v_calls, v_call_off, n_j, j_calls, j_call_off, q_off, q_text, weight, m_t, t_off,
                        t_text, db_header, db_header_bytes, db_line_off, db_lines, METRIC_WEIGHTED, cost, out, out_cap);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

// ---- the weighted metric's entries (include/dcrx.h "match, weighted")

uint64_t dcrx_cdr3_match_weighted_work_bytes(uint64_t m_q, uint64_t text_bytes) {
  return dcrx_cdr3_match_work_bytes(m_q, text_bytes, METRIC_HAMMING);      // (the same carve: no presence masks)
}

int dcrx_cdr3_match_weighted_device(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off,
                                    const char *d_text, uint64_t text_bytes, const dcrx_cdr3_cost_t *cost, uint32_t radius,
                                    uint32_t *d_degree, uint64_t *d_hit_off, uint32_t *d_hit, uint32_t *d_hit_dist, uint64_t hit_cap,
                                    uint64_t *d_hit_need, void *d_work, uint64_t work_bytes, void *hip_stream) try {
  static const char who[] = "dcrx_cdr3_match_weighted_device";
  CostArg wc;
  int rc = refuse(who, I, m_q, 0, METRIC_HAMMING);
  if (rc || (rc = refuse_cost(who, cost, radius, &wc))) return rc;
  return match_device(who, I, m_q, d_class, d_off, d_text, text_bytes, radius, METRIC_HAMMING, &wc, d_degree, d_hit_off, d_hit, d_hit_dist,
                      hit_cap, d_hit_need, d_work, work_bytes, (hipStream_t)hip_stream);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

int dcrx_cdr3_match_weighted_run(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *cls, const uint64_t *off, const char *text,
                                 const uint64_t *weight, const dcrx_cdr3_cost_t *cost, uint32_t radius, dcrx_cdr3_match_t **match_out) try {
  static const char who[] = "dcrx_cdr3_match_weighted_run";
  if (!match_out) return set_err(DCRX_E_INVALID, "dcrx_cdr3_match_weighted_run: null argument");
  *match_out = nullptr;
  CostArg wc;
  int rc = refuse(who, I, m_q, 0, METRIC_HAMMING);
  if (rc || (rc = refuse_cost(who, cost, radius, &wc))) return rc;
  return run_entry(who, I, m_q, cls, off, text, weight, radius, METRIC_HAMMING, &wc, match_out);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

int dcrx_cdr3_match_export_dist(const dcrx_cdr3_match_t *M, uint32_t *hit_dist) {
  if (!M) return set_err(DCRX_E_INVALID, "dcrx_cdr3_match_export_dist: null handle");
  if (!M->weighted) return set_err(DCRX_E_INVALID, "dcrx_cdr3_match_export_dist: the handle is not of dcrx_cdr3_match_weighted_run");
  if (hit_dist && !M->hit_dist.empty()) std::memcpy(hit_dist, M->hit_dist.data(), M->hit_dist.size() * sizeof(uint32_t));
  return DCRX_OK;
}

// ---- the profile's entries (include/dcrx.h "profile, weighted")

uint64_t dcrx_cdr3_profile_weighted_work_bytes(uint64_t m_q, uint64_t text_bytes, uint32_t bins) {
  (void)text_bytes;      // (per-query keys, ranks and packed strings; the histogram lives in LDS, whatever `bins` is)
  Pool P;
  ProfileWork W;
  if (m_q >= MAX_NODES || bins < 1 || bins > dcrx_cdr3profile::MAX_BINS || W.carve(P, m_q) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_profile_weighted_device(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off,
                                      const char *d_text, uint64_t text_bytes, const dcrx_cdr3_cost_t *cost, uint32_t step, uint32_t bins,
                                      uint32_t *d_profile, void *d_work, uint64_t work_bytes, void *hip_stream) try {
  static const char who[] = "dcrx_cdr3_profile_weighted_device";
  auto fail = [&](const char *what) { return set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  CostArg wc;
  uint32_t radius = 0;
  int rc = refuse_profile(who, I, m_q, cost, step, bins, &wc, &radius);
  if (rc) return rc;
  if (!m_q) return DCRX_OK;      // no cell to write
  if (!d_profile) return fail("null profile");
  if (!d_class || !d_off || !d_work || (text_bytes && !d_text)) return fail("null argument");
  if ((uintptr_t)d_work % ALIGN) return fail("the work space is not 256-byte aligned");
  Pool P(d_work);
  ProfileWork W;
  if ((rc = W.carve(P, m_q))) return rc;
  if (work_bytes < P.bytes()) return fail("the work space is smaller than dcrx_cdr3_profile_weighted_work_bytes(m_q, text_bytes, bins)");
  hipStream_t s = (hipStream_t)hip_stream;
  dcrx::DeviceGuard on(I->device);
  if (!I->m) {      // nothing can hit: every cell is zero, no kernel
    HIP_TRY(hipMemsetAsync(d_profile, 0, m_q * bins * sizeof(uint32_t), s));
    return DCRX_OK;
  }
  const Nodes N{d_class, d_off, reinterpret_cast<const uint8_t *>(d_text), text_bytes};
  return run_profile(*I, N, m_q, wc, radius, step, bins, d_profile, W, s);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

int dcrx_cdr3_profile_weighted(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *cls, const uint64_t *off, const char *text,
                               const dcrx_cdr3_cost_t *cost, uint32_t step, uint32_t bins, uint32_t *profile,
                               dcrx_cdr3_profile_stats_t *stats) try {
  static const char who[] = "dcrx_cdr3_profile_weighted";
  auto fail = [&](const char *what) { return set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  CostArg wc;
  uint32_t radius = 0;
  int rc = refuse_profile(who, I, m_q, cost, step, bins, &wc, &radius);
  if (rc) return rc;
  if (m_q && !profile) return fail("null profile");
  if (m_q && (!cls || !off)) return fail("null argument");
  dcrx_cdr3_profile_stats_t st{};
  st.queries = m_q;
  st.targets = I->m;
  st.targets_out_of_reach = I->out_of_reach;
  for (uint64_t k = 0; k < m_q; k++)
    if (off[k + 1] < off[k]) return fail("offsets go backwards");
  if (m_q && off[m_q] > off[0] && !text) return fail("text is null");
  for (uint64_t k = 0; k < m_q; k++) {
    const uint64_t len = off[k + 1] - off[k];
    if (!in_reach(len)) st.queries_out_of_reach++;
    else if (!host_letters(text + off[k], len)) st.queries_not_letters++;
  }
  const uint64_t cells = m_q * bins;
  if (m_q && I->m) {
    dcrx::DeviceGuard on(I->device);
    const uint64_t text_bytes = off[m_q] - off[0];
    Pool P;
    ProfileWork W;
    uint32_t *d_cls, *d_profile;
    uint64_t *d_off;
    uint8_t *d_text;
    for (int pass = 0; pass < 2; pass++) {
      P.get(&d_cls, m_q); P.get(&d_off, m_q + 1); P.get(&d_text, text_bytes); P.get(&d_profile, cells);
      if ((rc = W.carve(P, m_q)) || (pass == 0 && (rc = P.allocate()))) return rc;
    }
    if ((rc = upload_spans(m_q, off, text, d_off, d_text)) || (rc = to_device(d_cls, cls, m_q))) return rc;
    const Nodes N{d_cls, d_off, d_text, text_bytes};
    if ((rc = run_profile(*I, N, m_q, wc, radius, step, bins, d_profile, W, nullptr)) || (rc = to_host(profile, d_profile, cells))) return rc;
  } else if (cells) {
    std::memset(profile, 0, cells * sizeof(uint32_t));
  }
  for (uint64_t k = 0; k < m_q; k++) {
    uint64_t row = 0;
    for (uint32_t b = 0; b < bins; b++) row += profile[k * bins + b];
    st.cells_sum += row;
    st.queries_nonzero += row != 0;
  }
  if (stats) *stats = st;
  return DCRX_OK;
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

// ---- the tally's entries (include/dcrx.h "tally, weighted")

uint64_t dcrx_cdr3_tally_weighted_work_bytes(uint64_t m_q, uint64_t text_bytes, uint64_t m_t) {
  (void)text_bytes;      // (per-query keys, ranks and packed strings, and two accumulators per target)
  Pool P;
  TallyWork W;
  if (m_q >= MAX_NODES || m_t >= MAX_NODES || W.carve(P, m_q, m_t) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_tally_weighted_device(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off, const char *d_text,
                                    uint64_t text_bytes, const uint64_t *d_weight, const dcrx_cdr3_cost_t *cost, const uint32_t *d_radius,
                                    uint32_t *d_t_count, uint64_t *d_t_weight, uint32_t *d_q_degree, void *d_work, uint64_t work_bytes,
                                    void *hip_stream) try {
  static const char who[] = "dcrx_cdr3_tally_weighted_device";
  auto fail = [&](const char *what) { return set_err(DCRX_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  CostArg wc;
  int rc = refuse_tally(who, I, m_q, cost, d_t_count, d_t_weight, d_q_degree, &wc);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  dcrx::DeviceGuard on(I->device);
  if (!m_q || !I->m) {      // nothing can hit: every cell is zero, no kernel
    if (I->m) {
      HIP_TRY(hipMemsetAsync(d_t_count, 0, I->m * sizeof(uint32_t), s));
      HIP_TRY(hipMemsetAsync(d_t_weight, 0, I->m * sizeof(uint64_t), s));
    }
    if (m_q) HIP_TRY(hipMemsetAsync(d_q_degree, 0, m_q * sizeof(uint32_t), s));
    return DCRX_OK;
  }
  if (!d_class || !d_off || !d_weight || !d_radius || !d_work || (text_bytes && !d_text)) return fail("null argument");
  if ((uintptr_t)d_work % ALIGN) return fail("the work space is not 256-byte aligned");
  Pool P(d_work);
  TallyWork W;
  if ((rc = W.carve(P, m_q, I->m))) return rc;
  if (work_bytes < P.bytes()) return fail("the work space is smaller than dcrx_cdr3_tally_weighted_work_bytes(m_q, text_bytes, targets)");
  const Nodes N{d_class, d_off, reinterpret_cast<const uint8_t *>(d_text), text_bytes};
  return run_tally(*I, N, m_q, d_weight, wc, d_radius, d_t_count, d_t_weight, d_q_degree, W, s);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

int dcrx_cdr3_tally_weighted(const dcrx_cdr3_index_t *I, uint64_t m_q, const uint32_t *cls, const uint64_t *off, const char *text,
                             const uint64_t *weight, const dcrx_cdr3_cost_t *cost, const uint32_t *radius, uint32_t *t_count,
                             uint64_t *t_weight, uint32_t *q_degree, dcrx_cdr3_tally_stats_t *stats) try {
  static const char who[] = "dcrx_cdr3_tally_weighted";
  auto fail = [&](int code, const char *what) { return set_err(code, (std::string(who) + ": " + what).c_str()); };
  CostArg wc;
  int rc = refuse_tally(who, I, m_q, cost, t_count, t_weight, q_degree, &wc);
  if (rc) return rc;
  const uint64_t m_t = I->m;
  if ((m_q && (!cls || !off || !weight)) || (m_t && !radius)) return fail(DCRX_E_INVALID, "null argument");
  if (const char *what = refuse_radii(radius, m_t)) return fail(DCRX_E_INVALID, what);
  dcrx_cdr3_tally_stats_t st{};
  st.queries = m_q;
  st.targets = m_t;
  st.targets_out_of_reach = I->out_of_reach;
  for (uint64_t j = 0; j < m_t; j++) st.targets_without_radius += radius[j] == NO_RADIUS;
  uint64_t total = 0;
  for (uint64_t k = 0; k < m_q; k++) {
    if (off[k + 1] < off[k]) return fail(DCRX_E_INVALID, "offsets go backwards");
    if (__builtin_add_overflow(total, weight[k], &total)) return fail(DCRX_E_UNSUPPORTED, "the sum of the query weights is 2^64 or more");
  }
  if (m_q && off[m_q] > off[0] && !text) return fail(DCRX_E_INVALID, "text is null");
  for (uint64_t k = 0; k < m_q; k++) {
    const uint64_t len = off[k + 1] - off[k];
    if (!in_reach(len)) st.queries_out_of_reach++;
    else if (!host_letters(text + off[k], len)) st.queries_not_letters++;
  }
  if (m_q && m_t) {
    dcrx::DeviceGuard on(I->device);
    const uint64_t text_bytes = off[m_q] - off[0];
    Pool P;
    TallyWork W;
    uint32_t *d_cls, *d_radius, *d_tc, *d_deg;
    uint64_t *d_off, *d_weight, *d_tw;
    uint8_t *d_text;
    for (int pass = 0; pass < 2; pass++) {
      P.get(&d_cls, m_q); P.get(&d_off, m_q + 1); P.get(&d_text, text_bytes); P.get(&d_weight, m_q); P.get(&d_radius, m_t);
      P.get(&d_tc, m_t); P.get(&d_tw, m_t); P.get(&d_deg, m_q);
      if ((rc = W.carve(P, m_q, m_t)) || (pass == 0 && (rc = P.allocate()))) return rc;
    }
    if ((rc = upload_spans(m_q, off, text, d_off, d_text)) || (rc = to_device(d_cls, cls, m_q)) || (rc = to_device(d_weight, weight, m_q)) ||
        (rc = to_device(d_radius, radius, m_t))) return rc;
    const Nodes N{d_cls, d_off, d_text, text_bytes};
    if ((rc = run_tally(*I, N, m_q, d_weight, wc, d_radius, d_tc, d_tw, d_deg, W, nullptr)) || (rc = to_host(t_count, d_tc, m_t)) ||
        (rc = to_host(t_weight, d_tw, m_t)) || (rc = to_host(q_degree, d_deg, m_q))) return rc;
  } else {
    if (m_t) { std::memset(t_count, 0, m_t * sizeof(uint32_t)); std::memset(t_weight, 0, m_t * sizeof(uint64_t)); }
    if (m_q) std::memset(q_degree, 0, m_q * sizeof(uint32_t));
  }
  for (uint64_t k = 0; k < m_q; k++) {
    st.hits += q_degree[k];
    if (q_degree[k]) { st.queries_hit++; st.queries_hit_weight += weight[k]; }
  }
  for (uint64_t j = 0; j < m_t; j++) st.targets_hit += t_count[j] != 0;
  if (stats) *stats = st;
  return DCRX_OK;
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

}  // extern "C"

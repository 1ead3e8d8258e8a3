// dcrx_cdr3net.hip — the CDR3 network (`--clonotypes --cdr3-network`): which nodes (clonotypes) of one class and one string
// length lie within D substitutions of each other, and the connected components of that graph; include/dcrx.h holds the
// contract, dcrx_cdr3net_core.h the per-node and per-pair code, dcrx_cdr3walk.h the kernels that prepare and walk the table.
//
// The primitive (dcrx_cdr3_neighbours_device), all on the caller's stream and in the caller's work space:
//   keys     cdr3_keys_kernel, one lane per node: the bucket key (class, length), out of reach behind every bucket
//   sort     a stable radix sort of (key, rank): a bucket stays in rank order
//   gather   cdr3_gather_kernel<true, LEV>, one lane per sorted position: the 32-byte packed string, and the run marks whose
//            max scan gives every position its bucket's start
//   degrees  cdr3_walk_kernel<false, Within, Pair>: the table walked against itself, a block of 256 consecutive sorted nodes
//            from its first node's bucket start to its last node's bucket end.  Every node counts its OWN neighbours over its
//            whole bucket: twice the comparisons of a triangular walk, but no atomics, and the neighbours come in ascending rank
//   scan     an exclusive sum of the degrees in rank order: adj_off, whose end is the need
//   write    cdr3_walk_kernel<true, Within, Pair>: the same walk writes every neighbour's rank at its exact offset
// The host entry (dcrx_cdr3_network) runs those two halves around the adjacency's allocation, then the components (rounds of
// "the smallest label among my neighbours and me" and pointer jumping, double buffered, until a round changes nothing) and
// the totals (integer atomics onto the heads, results unused; the heads compacted in rank order).
// The sorts, scans, run heads and compaction are dcrx_group.h's.
//
// Under the Levenshtein metric (the *_metric entries, DCRX_CDR3NET_LEVENSHTEIN) the bucket is the class alone: the same keys
// are sorted over their class bits and the out-of-reach bit only — stable, so a class stays in rank order and the sorted keys
// keep every node's length —, the gather also leaves a letter-presence mask per node, and the walk (Pair is Levenshtein, not
// Hamming) tests a pair by class, length difference, presence masks and then lev_within (on the entry a lane has waiting,
// once some lane of the wave meets its next one).  A node still walks its whole bucket, now its class: the extra pairs fall
// at one length compare, and the neighbours still come in ascending rank.
//
// Under the weighted metric (the *_weighted entries; include/dcrx.h "the CDR3 network, weighted") the table is prepared in the
// same class order, without the presence masks (cdr3_gather_kernel<true, false, true>), and the walk's pair test is Weighted
// (dcrx_cdr3walk.h): a node with a non-letter is not admitted and is staged with length 0; the write pass stores every
// neighbour's distance beside its rank.  `wc` below is that walk's cost (null under the other two metrics), `limit` then the
// radius, and the work space is the Hamming walk's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_cdr3walk.h"
#include "dcrx_components.h"
#include "dcrx_text.h"

using dcrx::set_err;
using namespace dcrx_cdr3walk;

namespace {

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
  Sorted nodes(uint64_t n) const { return Sorted{key[1], idx[1], sj, pres, (uint32_t)n}; }
};

// one pass of the walk over the prepared table
template <bool WRITE> int run_walk(uint64_t n, uint32_t limit, uint32_t metric, const CostArg *wc, const Out &O, const Work &W, hipStream_t s) {
  const Sorted X = W.nodes(n);
  if (!wc) return walk<WRITE>(X, X, Within{W.bstart}, limit, metric == METRIC_LEVENSHTEIN, O, s);
  cdr3_walk_kernel<WRITE><<<grid_for(n), BLOCK, 0, s>>>(X, X, Within{W.bstart}, Weighted{*wc, limit}, O);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// keys, sort, gather, the bucket starts, the degree pass, the scan and the need
int run_degrees(const Nodes &N, uint64_t n, uint32_t limit, uint32_t metric, const CostArg *wc, uint32_t *d_degree, uint64_t *d_adj_off,
                uint64_t *d_need, const Work &W, hipStream_t s) {
  const bool lev = metric == METRIC_LEVENSHTEIN;
  const uint32_t n32 = (uint32_t)n;
  int rc;
  if ((rc = sorted_keys(N, n, W.key, W.idx, W.cub, lev || wc ? (int)LEN_BITS : 0, true, s))) return rc;
  if (wc) cdr3_gather_kernel<true, false, true><<<grid_for(n), BLOCK, 0, s>>>(N, n32, W.key[1], W.idx[1], W.sj, W.mark, nullptr);
  else if (lev) cdr3_gather_kernel<true, true><<<grid_for(n), BLOCK, 0, s>>>(N, n32, W.key[1], W.idx[1], W.sj, W.mark, W.pres);
  else cdr3_gather_kernel<true, false><<<grid_for(n), BLOCK, 0, s>>>(N, n32, W.key[1], W.idx[1], W.sj, W.mark, nullptr);
  HIP_TRY(hipGetLastError());
  if ((rc = run_heads(W.cub, W.mark, W.bstart, n, s)) ||
      (rc = run_walk<false>(n, limit, metric, wc, Out{d_degree, W.deg64, nullptr, nullptr, nullptr, 0}, W, s)) ||
      (rc = exclusive_sum(W.cub, W.deg64, d_adj_off, n, s))) return rc;
  cdr3_need_kernel<<<1, 64, 0, s>>>(W.deg64, d_adj_off, n32, d_need);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

int run_write(uint64_t n, uint32_t limit, uint32_t metric, const CostArg *wc, const uint64_t *d_adj_off, uint32_t *d_adj, uint32_t *d_adj_dist,
              uint64_t adj_cap, const Work &W, hipStream_t s) {
  return run_walk<true>(n, limit, metric, wc, Out{nullptr, nullptr, d_adj_off, d_adj, d_adj_dist, adj_cap}, W, s);
}

// an error of the entry `who` (the plain entries and their *_metric forms share one body and name themselves)
int fail(int code, const char *who, const char *what) { return set_err(code, (std::string(who) + ": " + what).c_str()); }

int neighbours_device(const char *who, uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                      uint32_t distance, uint32_t metric, const CostArg *wc, uint32_t *d_degree, uint64_t *d_adj_off, uint32_t *d_adj,
                      uint32_t *d_adj_dist, uint64_t adj_cap, uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream) try {
  if (m >= MAX_NODES) return fail(DCRX_E_UNSUPPORTED, who, "2^30 or more nodes");
  if (!wc && distance != 1 && distance != 2) return fail(DCRX_E_INVALID, who, "the distance is 1 or 2");
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
    return fail(DCRX_E_INVALID, who, wc ? "the work space is smaller than dcrx_cdr3net_weighted_work_bytes(m, text_bytes)"
                                     : metric == METRIC_HAMMING ? "the work space is smaller than dcrx_cdr3net_work_bytes(m, text_bytes)"
                                                                : "the work space is smaller than dcrx_cdr3net_metric_work_bytes(m, text_bytes, metric)");
  const Nodes N{d_class, d_off, reinterpret_cast<const uint8_t *>(d_text), text_bytes};
  if ((rc = run_degrees(N, m, distance, metric, wc, d_degree, d_adj_off, d_adj_need, W, s))) return rc;
  if (!d_adj || !adj_cap) return DCRX_OK;
  return run_write(m, distance, metric, wc, d_adj_off, d_adj, d_adj_dist, adj_cap, W, s);
} catch (const std::exception &e) {      // (a message that could not be built)
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t network(const char *who, uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                uint32_t distance, uint32_t metric, const CostArg *wc, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out,
                uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint32_t *adj_dist_out,
                uint64_t adj_cap, uint64_t *adj_need_out, dcrx_cdr3_network_stats_t *stats_out) try {
  if (m >= MAX_NODES) return fail(DCRX_E_UNSUPPORTED, who, "2^30 or more nodes");
  if (!wc && distance != 1 && distance != 2) return fail(DCRX_E_INVALID, who, "the distance is 1 or 2");
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

  Pool P;
  Work W;
  dcrx_components::TotalsWork T;
  uint32_t *d_cls, *d_degree, *d_label[2], *d_changed, *d_heads, *d_nn, *d_of;
  uint64_t *d_off, *d_weight, *d_adj_off, *d_need, *d_wout;
  uint8_t *d_text;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_cls, m); P.get(&d_off, m + 1); P.get(&d_text, text_bytes); P.get(&d_weight, m); P.get(&d_degree, m);
    P.get(&d_adj_off, m + 1); P.get(&d_need, 1); P.get(&d_label[0], m); P.get(&d_label[1], m); P.get(&d_changed, 1);
    P.get(&d_heads, m); P.get(&d_nn, m); P.get(&d_wout, m); P.get(&d_of, m);
    if ((rc = T.carve(P, m)) || (rc = W.carve(P, m, metric)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_spans(m, off, text, d_off, d_text)) || (rc = to_device(d_cls, cls, m)) || (rc = to_device(d_weight, weight, m))) return rc;
  const Nodes N{d_cls, d_off, d_text, text_bytes};

  // the degree pass, then an adjacency of exactly the entries it takes
  if ((rc = run_degrees(N, m, distance, metric, wc, d_degree, d_adj_off, d_need, W, nullptr))) return rc;
  uint64_t need = 0;
  if ((rc = to_host(&need, d_need, 1))) return rc;
  if (adj_need_out) *adj_need_out = need;
  const bool want_dist = wc && adj_dist_out && adj_out && need <= adj_cap;      // (the distances go where the adjacency goes)
  dcrx::DevBuf<uint32_t> d_adj, d_dist;
  if (d_adj.alloc(std::max<uint64_t>(need, 1)) || (want_dist && d_dist.alloc(std::max<uint64_t>(need, 1))))
    return fail(DCRX_E_NOMEM, who, "the adjacency does not fit the device's memory");
  if (need && (rc = run_write(m, distance, metric, wc, d_adj_off, d_adj.get(), want_dist ? d_dist.get() : nullptr, need, W, nullptr))) return rc;

  // components (dcrx_components.h): rounds of the neighbourhood's smallest label, then the labels followed to their ends;
  // totals onto the heads, and the heads in rank order are the rows
  if ((rc = dcrx_components::components(m32, d_adj_off, d_adj, need != 0, nullptr, d_label, d_changed, nullptr, nullptr)) ||
      (rc = dcrx_components::totals(m32, d_label[0], d_weight, T, d_of, d_heads, d_nn, d_wout, nullptr))) return rc;
  uint32_t c = 0;
  if ((rc = to_host(&c, T.kept, 1))) return rc;

  if ((rc = to_host(degree_out, d_degree, m)) || (rc = to_host(cluster_of_out, d_of, m)) || (rc = to_host(head_out, d_heads, c)) ||
      (rc = to_host(n_nodes_out, d_nn, c)) || (rc = to_host(weight_out, d_wout, c))) return rc;
  if (adj_off_out) {
    if ((rc = to_host(adj_off_out, d_adj_off, m + 1))) return rc;
    if (adj_out && need <= adj_cap && (rc = to_host(adj_out, d_adj.get(), need))) return rc;
    if (want_dist && (rc = to_host(adj_dist_out, d_dist.get(), need))) return rc;
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

int64_t format_edges(const char *who, uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                     uint32_t metric, const dcrx_cdr3_cost_t *cost, char *out, uint64_t out_cap) try {
  static const char header[] = "a\tb\tdistance\n";
  if (!cost && !metric_exists(metric)) return fail(DCRX_E_INVALID, who, "the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN");
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
      if (cost) {
        if (!in_reach(la) || !in_reach(lb) || !host_letters(text + off[a], la) || !host_letters(text + off[b], lb))
          return fail(DCRX_E_INVALID, who, "an edge between strings out of the weighted metric's reach");
        d = host_weighted(text + off[a], la, text + off[b], lb, *cost);
      } else if (metric == METRIC_LEVENSHTEIN) {
        d = dcrx::host_levenshtein(text + off[a], la, text + off[b], lb);
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
  return neighbours_device("dcrx_cdr3_neighbours_device", m, d_class, d_off, d_text, text_bytes, distance, METRIC_HAMMING, nullptr, d_degree,
                           d_adj_off, d_adj, nullptr, adj_cap, d_adj_need, d_work, work_bytes, hip_stream);
}

int dcrx_cdr3_neighbours_metric_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                                       uint32_t distance, uint32_t metric, uint32_t *d_degree, uint64_t *d_adj_off, uint32_t *d_adj,
                                       uint64_t adj_cap, uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream) {
  return neighbours_device("dcrx_cdr3_neighbours_metric_device", m, d_class, d_off, d_text, text_bytes, distance, metric, nullptr, d_degree,
                           d_adj_off, d_adj, nullptr, adj_cap, d_adj_need, d_work, work_bytes, hip_stream);
}

int64_t dcrx_cdr3_network(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                          uint32_t distance, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out, uint32_t *n_nodes_out,
                          uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint64_t adj_cap, uint64_t *adj_need_out,
                          dcrx_cdr3_network_stats_t *stats_out) {
  return network("dcrx_cdr3_network", m, cls, off, text, weight, distance, METRIC_HAMMING, nullptr, degree_out, cluster_of_out, head_out,
                 n_nodes_out, weight_out, adj_off_out, adj_out, nullptr, adj_cap, adj_need_out, stats_out);
}

int64_t dcrx_cdr3_network_metric(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                                 uint32_t distance, uint32_t metric, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out,
                                 uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint64_t adj_cap,
                                 uint64_t *adj_need_out, dcrx_cdr3_network_stats_t *stats_out) {
  return network("dcrx_cdr3_network_metric", m, cls, off, text, weight, distance, metric, nullptr, degree_out, cluster_of_out, head_out,
                 n_nodes_out, weight_out, adj_off_out, adj_out, nullptr, adj_cap, adj_need_out, stats_out);
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
  return format_edges("dcrx_format_cdr3_edges", m, adj_off, adj, off, text, METRIC_HAMMING, nullptr, out, out_cap);
}

int64_t dcrx_format_cdr3_edges_metric(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                                      uint32_t metric, char *out, uint64_t out_cap) {
  return format_edges("dcrx_format_cdr3_edges_metric", m, adj_off, adj, off, text, metric, nullptr, out, out_cap);
}

// ---- the weighted metric's entries (include/dcrx.h "the CDR3 network, weighted")

uint64_t dcrx_cdr3net_weighted_work_bytes(uint64_t m, uint64_t text_bytes) {
  return dcrx_cdr3net_metric_work_bytes(m, text_bytes, METRIC_HAMMING);      // (the same carve: no presence masks)
}

int dcrx_cdr3_neighbours_weighted_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                                         const dcrx_cdr3_cost_t *cost, uint32_t radius, uint32_t *d_degree, uint64_t *d_adj_off,
                                         uint32_t *d_adj, uint32_t *d_adj_dist, uint64_t adj_cap, uint64_t *d_adj_need, void *d_work,
                                         uint64_t work_bytes, void *hip_stream) try {
  static const char who[] = "dcrx_cdr3_neighbours_weighted_device";
  CostArg wc;
  const int rc = refuse_cost(who, cost, radius, &wc);
  if (rc) return rc;
  return neighbours_device(who, m, d_class, d_off, d_text, text_bytes, radius, METRIC_HAMMING, &wc, d_degree, d_adj_off, d_adj, d_adj_dist,
                           adj_cap, d_adj_need, d_work, work_bytes, hip_stream);
} catch (const std::exception &e) {      // (a message that could not be built)
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t dcrx_cdr3_network_weighted(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                                   const dcrx_cdr3_cost_t *cost, uint32_t radius, uint32_t *degree_out, uint32_t *cluster_of_out,
                                   uint32_t *head_out, uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out,
                                   uint32_t *adj_out, uint32_t *adj_dist_out, uint64_t adj_cap, uint64_t *adj_need_out,
                                   dcrx_cdr3_network_stats_t *stats_out) try {
  static const char who[] = "dcrx_cdr3_network_weighted";
  CostArg wc;
  const int rc = refuse_cost(who, cost, radius, &wc);
  if (rc) return rc;
  return network(who, m, cls, off, text, weight, radius, METRIC_HAMMING, &wc, degree_out, cluster_of_out, head_out, n_nodes_out, weight_out,
                 adj_off_out, adj_out, adj_dist_out, adj_cap, adj_need_out, stats_out);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t dcrx_format_cdr3_edges_weighted(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                                        const dcrx_cdr3_cost_t *cost, char *out, uint64_t out_cap) try {
  static const char who[] = "dcrx_format_cdr3_edges_weighted";
  const int rc = refuse_cost(who, cost, 0, nullptr);
  if (rc) return rc;
  return format_edges(who, m, adj_off, adj, off, text, METRIC_WEIGHTED, cost, out, out_cap);
} catch (const std::exception &e) {
  return set_err(DCRX_E_NOMEM, e.what());
}

}  // extern "C"


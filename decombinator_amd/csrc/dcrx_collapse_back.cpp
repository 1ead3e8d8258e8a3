// dcrx_collapse_back.cpp — the host half of `collapse` after the rows' front half (dcrx_collapse.cpp): grouping of the rows
// by barcode (reference src/decombinator/collapse.py:585-683), the protoseq test of the neighbour edges (make_clusters,
// :771-779) and the counting of DCRs per cluster with the `.freq`, -wc and -bd texts (collapsinate :897-977,
// write_clusters :813-843).  The UMI neighbour search between them is dcrx_umi.hip; the connected components (networkx's
// _plain_bfs, whose Python set order decides the cluster names) stay in Python.
//
// Grouping is the reference's loop, row by row in input order: it is cheap next to the rest (one hash lookup per row, a
// Levenshtein test against the protoseq only when a barcode repeats with another seq) and the group order it produces —
// by the row of each group's creation or last re-key — falls out of a sequential pass for free.
// The reference's `ratio < 0.01 and time > 3600 s` break (:526) is a wall-clock quirk and is not reproduced: every row is read.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/dcrx.h"

namespace dcrx { int set_err(int code, const char *msg); }
using dcrx::set_err;

namespace {

// levenshtein(a, b) when it is <= K, else K + 1: the DP restricted to the band |i - j| <= K.
int lev_bounded(const char *a, int n, const char *b, int m, int K, std::vector<int> &prev, std::vector<int> &cur) {
  if (std::abs(n - m) > K) return K + 1;
  if (n == m && std::memcmp(a, b, (size_t)n) == 0) return 0;
  K = std::min(K, std::max(n, m));
  const int INF = K + 1;
  prev.assign((size_t)m + 2, INF);
  cur.assign((size_t)m + 2, INF);
  for (int j = 0; j <= std::min(m, K); j++) prev[(size_t)j] = j;
  for (int i = 1; i <= n; i++) {
    const int lo = std::max(1, i - K), hi = std::min(m, i + K);
    cur[(size_t)lo - 1] = lo == 1 ? std::min(i, INF) : INF;
    int row_min = cur[(size_t)lo - 1];
    for (int j = lo; j <= hi; j++) {
      int v = prev[(size_t)j - 1] + (a[i - 1] != b[j - 1]);
      v = std::min(v, prev[(size_t)j] + 1);
      v = std::min(v, cur[(size_t)j - 1] + 1);
      cur[(size_t)j] = std::min(v, INF);
      row_min = std::min(row_min, cur[(size_t)j]);
    }
    if (hi < m) cur[(size_t)hi + 1] = INF;
    if (row_min > K) return K + 1;
    std::swap(prev, cur);
  }
  return prev[(size_t)m];
}

// are_seqs_equivalent (collapse.py:349-354): levenshtein <= len(shorter) * fraction, the product in double as Python takes it.
bool equivalent(std::string_view a, std::string_view b, double fraction, std::vector<int> &prev, std::vector<int> &cur) {
  const double thr = (double)std::min(a.size(), b.size()) * fraction;
  if (!(thr >= 0.0)) return false;
  const int K = thr >= 1e9 ? 1000000000 : (int)std::floor(thr);
  return lev_bounded(a.data(), (int)a.size(), b.data(), (int)b.size(), K, prev, cur) <= K;
}

struct Seq { std::string_view s; uint64_t count; };

struct Group {
  std::string barcode;
  std::vector<Seq> seqs;         // distinct seqs in first-seen order, with their counts
  uint32_t best = 0;             // index in seqs of the protoseq
  uint64_t order = 0;            // row of creation or last re-key
  std::vector<uint64_t> members; // input rows, in join order
  bool alive = true;
};

struct Row {                     // the fields of a row the later steps need (spans into the text)
  uint32_t dcr = 0;              // interned DCR (fields 0-4)
  std::string_view seq, qual, id, region, tail;
};

}  // namespace

struct dcrx_groups {
  const char *text = nullptr;
  const dcrx_collapse_row_t *rows = nullptr;
  int sampling = 0;
  std::vector<Row> row;                                  // per input row (only the rows that reach grouping are filled)
  std::vector<std::vector<std::string_view>> dcr_fields; // per interned DCR: its five fields
  std::vector<Group> groups;                             // every group ever made, in creation order
  std::vector<uint32_t> order;                           // the live groups, in the reference's dict order
};

namespace {

// Splits a row into its fields; false when it has fewer than `need`.
bool split_fields(const char *p, const char *end, std::string_view sep, std::string_view *f, int need, int max_f, int *nf) {
  int k = 0;
  const char *s = p;
  while (k < max_f) {
    const char *q = (const char *)nullptr;
    for (const char *x = s; x + sep.size() <= end; x++)
      if (std::memcmp(x, sep.data(), sep.size()) == 0) { q = x; break; }
    if (!q) { f[k++] = std::string_view(s, (size_t)(end - s)); break; }
    f[k++] = std::string_view(s, (size_t)(q - s));
    s = q + sep.size();
  }
  *nf = k;
  return k >= need;
}

// The Python repr of one field inside str(list): fields here are ASCII without quotes or backslashes (checked on entry).
void put_repr(std::string &o, std::string_view s) { o += '\''; o.append(s.data(), s.size()); o += '\''; }

void put_dcretc(std::string &o, const dcrx_groups &G, uint64_t r) {
  const Row &w = G.row[r];
  const auto &f = G.dcr_fields[w.dcr];
  o += '[';
  for (int q = 0; q < 5; q++) { if (q) o += ", "; put_repr(o, f[(size_t)q]); }
  o += "]|";
  o.append(w.seq.data(), w.seq.size()); o += '|';
  o.append(w.qual.data(), w.qual.size()); o += '|';
  o.append(w.id.data(), w.id.size());
  if (G.sampling) {
    const dcrx_collapse_row_t &cr = G.rows[r];
    o += '|'; o.append(cr.barcode, cr.barcode_len);
    o += '|'; o.append(cr.barcode_qual, cr.barcode_qual_len);
    o += '|'; o.append(w.region.data(), w.region.size());
    o += '|'; o.append(w.tail.data(), w.tail.size());
  }
}

bool plain_field(std::string_view s) {
  for (char c : s)
    if (c == '\'' || c == '\\' || (unsigned char)c < 32 || (unsigned char)c > 126) return false;
  return true;
}

}  // namespace

extern "C" int dcrx_seqs_equivalent(const char *a, uint32_t na, const char *b, uint32_t nb, double lev_fraction) {
  if ((na && !a) || (nb && !b)) return set_err(DCRX_E_INVALID, "dcrx_seqs_equivalent: null argument");
  std::vector<int> p, c;
  return equivalent(std::string_view(a ? a : "", na), std::string_view(b ? b : "", nb), lev_fraction, p, c) ? 1 : 0;
}

extern "C" int dcrx_collapse_group(const char *text, uint64_t n_bytes, const uint64_t *row_offsets, const dcrx_collapse_row_t *rows,
                                   uint64_t n_rows, const char *field_sep, double lev_fraction, int sampling_analysis,
                                   dcrx_groups_t **out, uint64_t *counters) {
  if (!out || !counters || !field_sep || !field_sep[0] || (n_rows && (!text || !row_offsets || !rows)))
    return set_err(DCRX_E_INVALID, "dcrx_collapse_group: bad argument");
  *out = nullptr;
  dcrx_groups *G = nullptr;
  try {
    G = new dcrx_groups();
    G->text = text;
    G->rows = rows;
    G->sampling = sampling_analysis ? 1 : 0;
    G->row.resize((size_t)n_rows);
    const std::string_view sep(field_sep);
    std::unordered_map<std::string_view, uint32_t> dcr_id;
    std::unordered_map<std::string, int64_t> by_barcode;        // group index, or -1 once the barcode is multi-TCR
    std::vector<uint64_t> dcr_rows;                             // input_dcr_counts (:555-563): per DCR
    std::vector<int> lp, lc;
    uint64_t multi_reads = 0, multi_barcodes = 0;
    for (uint64_t r = 0; r < n_rows; r++) {
      const dcrx_collapse_row_t &cr = rows[r];
      if (cr.status != DCRX_CF_OK && cr.status != DCRX_CF_OVERLONG) continue;
      if (row_offsets[r + 1] > n_bytes || row_offsets[r] > row_offsets[r + 1]) {
        delete G;
        return set_err(DCRX_E_INVALID, "dcrx_collapse_group: row offsets outside the text");
      }
      const char *p = text + row_offsets[r], *end = text + row_offsets[r + 1];
      while (end > p && (end[-1] == '\n' || end[-1] == '\r')) end--;
      std::string_view f[12];
      int nf = 0;
      if (!split_fields(p, end, sep, f, sampling_analysis ? 11 : 10, 12, &nf)) {
        delete G;
        const std::string m = "row " + std::to_string(r) + " has fewer fields than the grouping needs";
        return set_err(DCRX_E_INVALID, m.c_str());
      }
      for (int q = 0; q < 5; q++)
        if (!plain_field(f[q])) {
          delete G;
          const std::string m = "row " + std::to_string(r) + ": a DCR field holds a quote, a backslash or a non-printable byte";
          return set_err(DCRX_E_UNSUPPORTED, m.c_str());
        }
      const std::string_view dcr_text(f[0].data(), (size_t)(f[4].data() + f[4].size() - f[0].data()));
      auto it = dcr_id.find(dcr_text);
      uint32_t d;
      if (it == dcr_id.end()) {
        d = (uint32_t)G->dcr_fields.size();
        dcr_id.emplace(dcr_text, d);
        G->dcr_fields.push_back({f[0], f[1], f[2], f[3], f[4]});
        dcr_rows.push_back(0);
      } else {
        d = it->second;
      }
      dcr_rows[d]++;
      Row &w = G->row[(size_t)r];
      w.dcr = d;
      if (cr.status != DCRX_CF_OK) continue;                  // too long an inter-tag seq: counted above, not grouped
      w.seq = f[6]; w.qual = f[7]; w.id = f[5]; w.region = f[8];
      if (sampling_analysis) w.tail = f[10];
      const std::string barcode(cr.barcode, cr.barcode_len);
      auto bt = by_barcode.find(barcode);
      if (bt == by_barcode.end()) {                           // a new group, index 0 (:671-681)
        by_barcode.emplace(barcode, (int64_t)G->groups.size());
        Group g;
        g.barcode = barcode;
        g.seqs.push_back({w.seq, 1});
        g.order = r;
        g.members.push_back(r);
        G->groups.push_back(std::move(g));
        continue;
      }
      if (bt->second < 0) { multi_reads++; continue; }        // a multi-TCR barcode (:604-607)
      Group &g = G->groups[(size_t)bt->second];
      if (!equivalent(g.seqs[g.best].s, w.seq, lev_fraction, lp, lc)) {   // the barcode turns multi-TCR (:657-669)
        multi_reads++;
        multi_barcodes++;
        g.alive = false;
        g.members.clear(); g.members.shrink_to_fit();
        g.seqs.clear(); g.seqs.shrink_to_fit();
        bt->second = -1;
        continue;
      }
      g.members.push_back(r);
      // Counter(seqs).most_common(1) (:626-631): only this seq's count moved, so the winner is the old one or this one;
      // ties go to the seq seen first in the group
      uint32_t s = 0;
      while (s < g.seqs.size() && g.seqs[s].s != w.seq) s++;
      if (s == g.seqs.size()) g.seqs.push_back({w.seq, 0});
      g.seqs[s].count++;
      if (s != g.best && (g.seqs[s].count > g.seqs[g.best].count || (g.seqs[s].count == g.seqs[g.best].count && s < g.best))) {
        if (g.seqs[s].s != g.seqs[g.best].s) g.order = r;     // a new protoseq re-keys the group: it moves to the dict's end
        g.best = s;
      }
    }
    std::vector<std::pair<uint64_t, uint32_t>> live;
    for (uint32_t k = 0; k < G->groups.size(); k++)
      if (G->groups[k].alive) live.push_back({G->groups[k].order, k});
    std::sort(live.begin(), live.end());
    G->order.reserve(live.size());
    for (auto &x : live) G->order.push_back(x.second);
    counters[DCRX_GRP_C_KEYS] = G->order.size();
    counters[DCRX_GRP_C_INPUT_UNIQUE] = dcr_rows.size();
    uint64_t total = 0;
    for (uint64_t c : dcr_rows) total += c;
    counters[DCRX_GRP_C_INPUT_TOTAL] = total;
    counters[DCRX_GRP_C_MULTI_BARCODES] = multi_barcodes;
    counters[DCRX_GRP_C_MULTI_READS] = multi_reads;
  } catch (const std::bad_alloc &) {
    delete G;
    return set_err(DCRX_E_NOMEM, "out of memory in dcrx_collapse_group");
  }
  *out = G;
  return DCRX_OK;
}

extern "C" void dcrx_groups_destroy(dcrx_groups_t *groups) { delete groups; }

extern "C" int dcrx_groups_info(const dcrx_groups_t *G, uint64_t *n_groups, uint64_t *n_members, uint64_t *umi_bytes,
                                uint64_t *proto_bytes) {
  if (!G) return set_err(DCRX_E_INVALID, "dcrx_groups_info: null handle");
  uint64_t nm = 0, ub = 0, pb = 0;
  for (uint32_t k : G->order) {
    const Group &g = G->groups[k];
    nm += g.members.size();
    ub += g.barcode.size();
    pb += g.seqs[g.best].s.size();
  }
  if (n_groups) *n_groups = G->order.size();
  if (n_members) *n_members = nm;
  if (umi_bytes) *umi_bytes = ub;
  if (proto_bytes) *proto_bytes = pb;
  return DCRX_OK;
}

extern "C" int dcrx_groups_export(const dcrx_groups_t *G, char *umi_text, uint64_t *umi_off, char *proto_text, uint64_t *proto_off,
                                  uint64_t *member_off, uint64_t *member_rows) {
  if (!G) return set_err(DCRX_E_INVALID, "dcrx_groups_export: null handle");
  uint64_t u = 0, p = 0, m = 0;
  for (size_t q = 0; q < G->order.size(); q++) {
    const Group &g = G->groups[G->order[q]];
    const std::string_view proto = g.seqs[g.best].s;
    if (umi_off) umi_off[q] = u;
    if (proto_off) proto_off[q] = p;
    if (member_off) member_off[q] = m;
    if (umi_text) std::memcpy(umi_text + u, g.barcode.data(), g.barcode.size());
    if (proto_text) std::memcpy(proto_text + p, proto.data(), proto.size());
    if (member_rows) std::memcpy(member_rows + m, g.members.data(), g.members.size() * sizeof(uint64_t));
    u += g.barcode.size(); p += proto.size(); m += g.members.size();
  }
  const size_t n = G->order.size();
  if (umi_off) umi_off[n] = u;
  if (proto_off) proto_off[n] = p;
  if (member_off) member_off[n] = m;
  return DCRX_OK;
}

extern "C" int dcrx_groups_equivalent(const dcrx_groups_t *G, const uint64_t *pairs, uint64_t n_pairs, double lev_fraction,
                                      uint8_t *keep, int n_threads) {
  if (!G || (n_pairs && (!pairs || !keep))) return set_err(DCRX_E_INVALID, "dcrx_groups_equivalent: bad argument");
  const uint64_t n = G->order.size();
  for (uint64_t e = 0; e < n_pairs; e++)
    if ((pairs[e] >> 32) >= n || (pairs[e] & 0xffffffffull) >= n)
      return set_err(DCRX_E_INVALID, "dcrx_groups_equivalent: a pair names a group that does not exist");
  auto proto = [&](uint64_t k) { const Group &g = G->groups[G->order[k]]; return g.seqs[g.best].s; };
  auto work = [&](uint64_t lo, uint64_t hi) {
    std::vector<int> a, b;
    for (uint64_t e = lo; e < hi; e++) keep[e] = equivalent(proto(pairs[e] >> 32), proto(pairs[e] & 0xffffffffull), lev_fraction, a, b) ? 1 : 0;
  };
  unsigned nt = n_threads > 0 ? (unsigned)n_threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n_pairs < 4096) nt = 1;
  try {
    std::vector<std::thread> th;
    const uint64_t per = (n_pairs + nt - 1) / nt;
    for (unsigned t = 1; t < nt; t++) {
      const uint64_t lo = std::min(n_pairs, per * t), hi = std::min(n_pairs, per * (t + 1));
      try { th.emplace_back(work, lo, hi); } catch (const std::system_error &) { work(lo, hi); }
    }
    work(0, std::min(n_pairs, per));
    for (auto &x : th) x.join();
  } catch (const std::bad_alloc &) {
    return set_err(DCRX_E_NOMEM, "out of memory in dcrx_groups_equivalent");
  }
  return DCRX_OK;
}

extern "C" int dcrx_collapse_count(const dcrx_groups_t *G, const uint32_t *cluster_groups, const uint64_t *cluster_off,
                                   uint64_t n_clusters, uint64_t *n_dcrs, uint64_t *votes, uint64_t *size_sum, uint64_t *freq_bytes,
                                   char *freq_text, int extra, uint64_t *wc_bytes, char *wc_text, uint64_t *bd_bytes, char *bd_text) {
  if (!G || !n_dcrs || !freq_bytes || (n_clusters && (!cluster_groups || !cluster_off)) || (extra && (!wc_bytes || !bd_bytes)))
    return set_err(DCRX_E_INVALID, "dcrx_collapse_count: bad argument");
  const uint64_t n_groups = G->order.size();
  if (n_clusters && cluster_off[0] != 0) return set_err(DCRX_E_INVALID, "dcrx_collapse_count: cluster_off[0] != 0");
  for (uint64_t c = 0; c < n_clusters; c++) {
    if (cluster_off[c + 1] <= cluster_off[c]) return set_err(DCRX_E_INVALID, "dcrx_collapse_count: an empty cluster");
    for (uint64_t q = cluster_off[c]; q < cluster_off[c + 1]; q++)
      if (cluster_groups[q] >= n_groups) return set_err(DCRX_E_INVALID, "dcrx_collapse_count: a cluster names a group that does not exist");
  }
  try {
    // per cluster: most_common(1) of its members' DCRs in concatenation order (:945-951), ties to the first seen
    std::vector<uint32_t> dcr_order;                             // DCRs in order of their first cluster
    std::vector<int64_t> slot(G->dcr_fields.size(), -1);         // DCR -> position in dcr_order
    std::vector<uint64_t> v, ssum;
    std::vector<uint64_t> cnt(G->dcr_fields.size(), 0);
    std::vector<uint32_t> seen;
    std::string wc, bd;
    for (uint64_t c = 0; c < n_clusters; c++) {
      uint64_t size = 0;
      seen.clear();
      uint32_t best = 0;
      uint64_t best_n = 0;
      const Group &base = G->groups[G->order[cluster_groups[cluster_off[c]]]];
      for (uint64_t q = cluster_off[c]; q < cluster_off[c + 1]; q++) {
        const Group &g = G->groups[G->order[cluster_groups[q]]];
        for (uint64_t r : g.members) {
          const uint32_t d = G->row[(size_t)r].dcr;
          if (cnt[d]++ == 0) seen.push_back(d);
          size++;
          if (extra) {
            wc.append(base.barcode); wc += ":0|";
            put_dcretc(wc, *G, r);
            wc += '\n';
          }
        }
      }
      for (uint32_t d : seen) {                                  // first-seen order: a tie keeps the earlier DCR
        if (cnt[d] > best_n) { best_n = cnt[d]; best = d; }
      }
      for (uint32_t d : seen) cnt[d] = 0;
      if (slot[best] < 0) { slot[best] = (int64_t)dcr_order.size(); dcr_order.push_back(best); v.push_back(0); ssum.push_back(0); }
      v[(size_t)slot[best]]++;
      ssum[(size_t)slot[best]] += size;
      if (extra) { bd.append(base.barcode); bd += "|0,"; bd += std::to_string(size); bd += '\n'; }
    }
    std::string freq;
    for (size_t k = 0; k < dcr_order.size(); k++) {
      const auto &f = G->dcr_fields[dcr_order[k]];
      for (int q = 0; q < 5; q++) { freq.append(f[(size_t)q].data(), f[(size_t)q].size()); freq += ", "; }
      // round(sum / count): the quotient in double, then half to even (:957-960)
      const double mean = (double)ssum[k] / (double)v[k];
      freq += std::to_string(v[k]); freq += ", ";
      freq += std::to_string((long long)std::nearbyint(mean)); freq += '\n';
    }
    *n_dcrs = dcr_order.size();
    *freq_bytes = freq.size();
    if (extra) { *wc_bytes = wc.size(); *bd_bytes = bd.size(); }
    if (freq_text) {
      std::memcpy(freq_text, freq.data(), freq.size());
      if (votes) std::memcpy(votes, v.data(), v.size() * sizeof(uint64_t));
      if (size_sum) std::memcpy(size_sum, ssum.data(), ssum.size() * sizeof(uint64_t));
      if (extra && wc_text) std::memcpy(wc_text, wc.data(), wc.size());
      if (extra && bd_text) std::memcpy(bd_text, bd.data(), bd.size());
    }
  } catch (const std::bad_alloc &) {
    return set_err(DCRX_E_NOMEM, "out of memory in dcrx_collapse_count");
  }
  return DCRX_OK;
}

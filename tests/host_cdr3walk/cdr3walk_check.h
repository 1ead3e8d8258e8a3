// Test-only: what the stand-alone programs that check the host walk (cdr3walk_host.h) share: a table of (class, string) under
// construction, the constructed strings and cost tables, the two reference distances — the plain Levenshtein DP and the
// weighted contract read out (the gapped string built for every p) — and the comparison of the walk's rows with an all-pairs
// count.
#pragma once
#include <cstdio>
#include <string>

#include "cdr3walk_host.h"

namespace cdr3walk_check {

using namespace cdr3walk_host;

struct Table {
  std::vector<uint32_t> cls;
  std::vector<uint64_t> off{0};
  std::string text;
  void add(uint32_t c, const std::string &s) { cls.push_back(c); text += s; off.push_back(text.size()); }
  uint64_t m() const { return cls.size(); }
  const uint8_t *bytes() const { return reinterpret_cast<const uint8_t *>(text.data()); }
  std::vector<std::string> strings() const {
    std::vector<std::string> out;
    for (uint64_t i = 0; i < m(); i++) out.push_back(text.substr(off[i], off[i + 1] - off[i]));
    return out;
  }
};

// string number i: three base-20 digits between fixed ends (two numbers differ in 1 to 3 places); tails: the tail has
// 2 + i % 3 letters of its four
inline std::string code(uint32_t i, bool tails = false) {
  static const char amino[] = "ACDEFGHIKLMNPQRSTVWY";
  std::string s = "CASS";
  const uint32_t n = i;
  for (int d = 0; d < 3; d++, i /= 20) s += amino[i % 20];
  return s + std::string("EQYF").substr(0, tails ? 2 + n % 3 : 4);
}

inline std::vector<uint8_t> table(uint32_t seed) {      // symmetric, zero diagonal, cells 0 .. 255
  std::vector<uint8_t> sub(SUB_BYTES, 0);
  for (uint32_t x = 1; x <= 26; x++)
    for (uint32_t y = 1; y < x; y++) {
      seed = seed * 1664525u + 1013904223u;
      sub[x * SUB_DIM + y] = sub[y * SUB_DIM + x] = (uint8_t)((seed >> 24) % (seed & 4 ? 13 : 256));
    }
  return sub;
}

// in reach and letters alone: what takes part under the weighted metric
inline bool letters(const std::string &s) {
  if (s.empty() || s.size() > MAX_LEN) return false;
  for (char c : s)
    if (c < 'A' || c > 'Z') return false;
  return true;
}

inline uint64_t lev(const std::string &a, const std::string &b) {
  std::vector<uint64_t> prev(b.size() + 1), cur(b.size() + 1);
  std::iota(prev.begin(), prev.end(), 0);
  for (size_t i = 1; i <= a.size(); i++) {
    cur[0] = i;
    for (size_t j = 1; j <= b.size(); j++) cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])});
    prev.swap(cur);
  }
  return prev[b.size()];
}

// whether two strings of one class hit under a plain metric at D, and at which distance
inline bool plain_hit(const std::string &a, const std::string &b, uint32_t D, uint32_t metric, uint64_t *d) {
  if (a.empty() || b.empty() || a.size() > MAX_LEN || b.size() > MAX_LEN) return false;
  if (metric == METRIC_LEVENSHTEIN) return (*d = lev(a, b)) <= D;
  if (a.size() != b.size()) return false;
  *d = 0;
  for (size_t p = 0; p < a.size(); p++) *d += a[p] != b[p];
  return *d <= D;
}

// the contract: a with a gap of d put in behind its first p residues, against b, summed over the counted positions
inline uint64_t dist(std::string a, std::string b, const Cost &C) {
  if (a.size() > b.size()) a.swap(b);
  const size_t la = a.size(), d = b.size() - la;
  uint64_t best = UINT64_MAX;
  for (size_t p = 0; p <= la; p++) {
    const std::string gapped = a.substr(0, p) + std::string(d, '-') + a.substr(p);
    uint64_t sum = 0;
    for (size_t k = 0; k < gapped.size(); k++) {
      if (gapped[k] == '-') continue;
      const size_t i = k < p ? k : k - d;      // the position in a
      if (i < C.ntrim || i + C.ctrim >= la) continue;
      sum += C.sub[(gapped[k] & 31) * SUB_DIM + (b[k] & 31)];
    }
    best = std::min(best, sum);
  }
  return d * C.gap + best;
}

inline Weighted weighted(const Cost &C, uint32_t radius) { return cdr3walk_host::weighted(C.sub, C.gap, C.ntrim, C.ctrim, radius); }

// The walk's rows against the all-pairs count: row i wants, in the order of j, every j < m_t of which hit(i, j, &d) holds,
// with its distance d.  Returns the rows that differ; *total: the hits wanted.
template <class F> int rows_differ(const Hits &got, uint64_t m_q, uint64_t m_t, F hit, uint64_t *total) {
  int bad = 0;
  for (uint64_t i = 0; i < m_q; i++) {
    std::vector<Hit> want;
    for (uint64_t j = 0; j < m_t; j++) {
      uint64_t d = 0;
      if (hit(i, j, &d)) want.push_back(Hit{(uint32_t)j, (uint32_t)d});
    }
    if (!(want == got.rows.at(i))) bad++;
    *total += want.size();
  }
  return bad;
}

// the hits of a table against itself that have no twin of the same distance the other way round
inline int not_symmetric(const Hits &got) {
  int bad = 0;
  for (uint64_t i = 0; i < got.rows.size(); i++)
    for (const Hit &h : got.rows[i]) {
      bool back = false;
      for (const Hit &g : got.rows.at(h.rank)) back |= g.rank == i && g.dist == h.dist;
      if (!back) bad++;
    }
  return bad;
}

}  // namespace cdr3walk_check

// dcrx_text.h — the bounded text writer of the format entries (dcrx_format_clonotypes, dcrx_format_cdr3_clusters,
// dcrx_format_cdr3_edges[_metric], dcrx_format_overlap_public), written once, and the edit distance two of them print.
// Host only; no HIP.
// A format entry is called twice: with no buffer (or one too small) for the size, then with one that fits.  So every
// piece is written only where it fits and always counted: `at` ends as the bytes the whole text takes.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace dcrx {

struct TextOut {
  char *out;
  uint64_t cap, at = 0;
  void put(const char *p, uint64_t bytes) {
    if (out && at + bytes <= cap && bytes) std::memcpy(out + at, p, bytes);
    at += bytes;
  }
  void unum(unsigned long long x) {
    char buf[24];
    put(buf, (uint64_t)snprintf(buf, sizeof buf, "%llu", x));
  }
  void num(long long x) {
    char buf[24];
    put(buf, (uint64_t)snprintf(buf, sizeof buf, "%lld", x));
  }
  // the k-th string of an offsets table: text[off[k] .. off[k + 1])
  template <class O> void put_span(const char *text, const O *off, uint64_t k) { put(text + off[k], off[k + 1] - off[k]); }
};

// the Levenshtein distance of two byte strings of any length (the distance column of the edge file and of the matches file):
// a plain two-row table
inline uint64_t host_levenshtein(const char *a, uint64_t la, const char *b, uint64_t lb) {
  std::vector<uint64_t> prev(lb + 1), cur(lb + 1);
  for (uint64_t j = 0; j <= lb; j++) prev[j] = j;
  for (uint64_t i = 1; i <= la; i++) {
    cur[0] = i;
    for (uint64_t j = 1; j <= lb; j++) cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1] ? 1u : 0u)});
    prev.swap(cur);
  }
  return prev[lb];
}

}  // namespace dcrx

// dcrx_text.h — the bounded text writer of the format entries (dcrx_format_clonotypes, dcrx_format_cdr3_clusters,
// dcrx_format_cdr3_edges[_metric], dcrx_format_overlap_public), written once.  Host only; no HIP.
// A format entry is called twice: with no buffer (or one too small) for the size, then with one that fits.  So every
// piece is written only where it fits and always counted: `at` ends as the bytes the whole text takes.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>

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

}  // namespace dcrx

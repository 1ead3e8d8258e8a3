// Test-only, stand-alone (its own main; `make asan` builds it with -fsanitize=address,undefined): bin_of of
// dcrx_cdr3profile_core.h for every d in 0 .. 65535 under steps at the edges of its range, against the smallest b with
// b * step >= d found by multiplying; the ladders the entries refuse; and the host walk with the histogram sink over tables that
// put a class on the tile and block edges (1, 3 and 6 blocks of queries), mix in nodes that take no part and hold every length
// 0 .. 33, each against an all-pairs count whose distance is the contract read out (the gapped string built for every p).
// Exit status 0: everything agreed (and the sanitizers saw nothing).
#include <cstdio>
#include <string>

#include "cdr3profile_walk.h"

using namespace cdr3profile_host;

namespace {

struct Table {
  std::vector<uint32_t> cls;
  std::vector<uint64_t> off{0};
  std::string text;
  void add(uint32_t c, const std::string &s) { cls.push_back(c); text += s; off.push_back(text.size()); }
  uint64_t m() const { return cls.size(); }
  std::string str(uint64_t i) const { return text.substr(off[i], off[i + 1] - off[i]); }
  const uint8_t *bytes() const { return reinterpret_cast<const uint8_t *>(text.data()); }
};

std::string code(uint32_t i) {      // three base-20 digits between fixed ends, and a tail of 2 .. 4 letters by the number
  static const char amino[] = "ACDEFGHIKLMNPQRSTVWY";
  std::string s = "CASS";
  const uint32_t n = i;
  for (int d = 0; d < 3; d++, i /= 20) s += amino[i % 20];
  return s + std::string("EQYF").substr(0, 2 + n % 3);
}

std::vector<uint8_t> table(uint32_t seed) {      // symmetric, zero diagonal, cells 0 .. 255
  std::vector<uint8_t> sub(SUB_BYTES, 0);
  for (uint32_t x = 1; x <= 26; x++)
    for (uint32_t y = 1; y < x; y++) {
      seed = seed * 1664525u + 1013904223u;
      sub[x * SUB_DIM + y] = sub[y * SUB_DIM + x] = (uint8_t)((seed >> 24) % (seed & 4 ? 13 : 256));
    }
  return sub;
}

bool takes_part(const std::string &s) {
  if (s.empty() || s.size() > MAX_LEN) return false;
  for (char c : s)
    if (c < 'A' || c > 'Z') return false;
  return true;
}

// the contract: a with a gap of d put in behind its first p residues, against b, summed over the counted positions
uint64_t dist(std::string a, std::string b, const Cost &C) {
  if (a.size() > b.size()) a.swap(b);
  const size_t la = a.size(), d = b.size() - la;
  uint64_t best = UINT64_MAX;
  for (size_t p = 0; p <= la; p++) {
    const std::string gapped = a.substr(0, p) + std::string(d, '-') + a.substr(p);
    uint64_t sum = 0;
    for (size_t k = 0; k < gapped.size(); k++) {
      if (gapped[k] == '-') continue;
      const size_t i = k < p ? k : k - d;
      if (i < C.ntrim || i + C.ctrim >= la) continue;
      sum += C.sub[(gapped[k] & 31) * SUB_DIM + (b[k] & 31)];
    }
    best = std::min(best, sum);
  }
  return d * C.gap + best;
}

int check_bins() {
  int bad = 0;
  for (uint32_t step : {1u, 2u, 3u, 5u, 7u, 12u, 255u, 256u, 257u, 4095u, 4096u, 32767u, 32768u, 65534u, 65535u}) {
    uint64_t b = 0;      // the smallest b with b * step >= d: it only grows with d
    for (uint32_t d = 0; d <= 65535; d++) {
      while (b * step < d) b++;
      if (bin_of(d, step) != b) bad++;
    }
  }
  struct { uint32_t step, bins; bool refused; } ladders[] = {{0, 1, true}, {1, 0, true}, {1, 33, true}, {65536, 1, true}, {65535, 2, false},
                                                              {65535, 3, true}, {2115, 32, true}, {2114, 32, false}, {2115, 31, false},
                                                              {1, 32, false}, {1, 1, false}, {65535, 1, false}};
  for (const auto &l : ladders)
    if ((dcrx_cdr3profile::refuse_ladder(l.step, l.bins) != nullptr) != l.refused) bad++;
  std::printf("bin_of and the ladders: %d differ\n", bad);
  return bad;
}

int check(const char *name, const Table &T, const Table &Q, const Cost &C, uint32_t step, uint32_t bins) {
  std::vector<uint32_t> got;
  if (profile(T.m(), T.cls.data(), T.off.data(), T.bytes(), Q.m(), Q.cls.data(), Q.off.data(), Q.bytes(), C, step, bins, got)) return 1;
  int bad = 0;
  uint64_t total = 0;
  for (uint64_t i = 0; i < Q.m(); i++) {
    std::vector<uint32_t> want(bins, 0);
    const std::string q = Q.str(i);
    for (uint64_t j = 0; takes_part(q) && j < T.m(); j++) {
      const std::string t = T.str(j);
      if (Q.cls[i] != T.cls[j] || !takes_part(t)) continue;
      const uint64_t d = dist(q, t, C), b = (d + step - 1) / step;
      if (b < bins) { want[b]++; total++; }
    }
    for (uint32_t b = 0; b < bins; b++) bad += got.at(i * bins + b) != want[b];
  }
  std::printf("%s, step %u bins %u gap %u trim %u,%u: %llu counted, %d cells differ\n", name, step, bins, C.gap, C.ntrim, C.ctrim,
              (unsigned long long)total, bad);
  return bad;
}

int check_all(const char *name, const Table &T, const Table &Q) {
  int bad = 0;
  const std::vector<uint8_t> s1 = table(1), s2 = table(7);
  bad += check(name, T, Q, Cost{s1.data(), 12, 3, 2}, 2, 25);
  bad += check(name, T, Q, Cost{s1.data(), 12, 3, 2}, 48, 2);
  bad += check(name, T, Q, Cost{s2.data(), 5, 0, 0}, 3, 32);
  bad += check(name, T, Q, Cost{s1.data(), 255, 16, 16}, 65535, 2);
  bad += check(name, T, Q, Cost{s2.data(), 1, 1, 4}, 7, 1);
  return bad;
}

}  // namespace

int main() {
  int bad = check_bins();
  for (uint32_t n : {1u, 255u, 256u, 257u, 513u, 1500u}) {
    Table T, Q;
    for (uint32_t i = 0; i < n; i++) T.add(7, code(i));
    for (uint32_t i : {0u, n - 1, n, 7999u}) Q.add(7, code(i));
    Q.add(8, code(0));
    Q.add(7, "");
    Q.add(7, std::string(33, 'A'));
    Q.add(7, "CASSaEQYF");
    Q.add(7, std::string("CAS\0EQYF", 8));
    bad += check_all("targets in one class", T, Q);
    bad += check_all("queries in one class", Q, T);
  }
  {
    Table T, Q;
    const std::string base = "CASSLAPGATNEKLFFGSGTQLSVLEDLKNVFPPE";
    for (size_t l = 0; l <= 33; l++) {
      T.add(0, base.substr(0, l));
      Q.add(0, base.substr(0, l / 2) + base.substr(base.size() - (l - l / 2)));
    }
    bad += check_all("every length", T, Q);
  }
  {
    Table T, Q, none;
    T.add(1, code(1));
    Q.add(1, code(2));
    bad += check_all("no targets", none, Q);
    bad += check_all("no queries", T, none);
  }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

// Test-only, stand-alone (its own main; `make asan` builds it with -fsanitize=address,undefined): bin_of of
// dcrx_cdr3profile_core.h for every d in 0 .. 65535 under steps at the edges of its range, against the smallest b with
// b * step >= d found by multiplying; the ladders the entries refuse; and the host walk with the histogram sink over tables that
// put a class on the tile and block edges (1, 3 and 6 blocks of queries), mix in nodes that take no part and hold every length
// 0 .. 33, each against an all-pairs count whose distance is the contract read out (the gapped string built for every p).
// Exit status 0: everything agreed (and the sanitizers saw nothing).
#include "../host_cdr3walk/cdr3walk_check.h"

using namespace cdr3walk_check;
using dcrx_cdr3profile::bin_of;

namespace {

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
  if (dcrx_cdr3profile::refuse_ladder(step, bins)) return 1;
  const std::vector<uint32_t> got = profile(T.m(), T.cls.data(), T.off.data(), T.bytes(), Q.m(), Q.cls.data(), Q.off.data(), Q.bytes(), weighted(C, 0), step, bins);
  const std::vector<std::string> t = T.strings(), q = Q.strings();
  int bad = 0;
  uint64_t total = 0;
  for (uint64_t i = 0; i < Q.m(); i++) {
    std::vector<uint32_t> want(bins, 0);
    for (uint64_t j = 0; letters(q[i]) && j < T.m(); j++) {
      if (Q.cls[i] != T.cls[j] || !letters(t[j])) continue;
      const uint64_t d = dist(q[i], t[j], C), b = (d + step - 1) / step;
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
    for (uint32_t i = 0; i < n; i++) T.add(7, code(i, true));
    for (uint32_t i : {0u, n - 1, n, 7999u}) Q.add(7, code(i, true));
    Q.add(8, code(0, true));
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
    T.add(1, code(1, true));
    Q.add(1, code(2, true));
    bad += check_all("no targets", none, Q);
    bad += check_all("no queries", T, none);
  }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

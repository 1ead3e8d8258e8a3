// Test-only, stand-alone (its own main; `make asan` builds it with -fsanitize=address,undefined): the tally's walk on the host
// (cdr3tally_walk.h) over tables that put a class on the tile and block edges (1, 3 and 6 blocks of queries), mix in nodes that
// take no part and hold every length 0 .. 33, under three patterns of radii per target — all R, R * (j % 4) / 3, and every third
// target without one —, each against an all-pairs count whose distance is the contract read out (the gapped string built for
// every p); the radii the host entry refuses; and the bound on the flushes.  Exit status 0: everything agreed (and the sanitizers
// saw nothing).
#include "../host_cdr3walk/cdr3walk_check.h"
#include "cdr3tally_walk.h"

using namespace cdr3walk_check;
using namespace cdr3tally_host;

namespace {

std::vector<uint32_t> radii(uint64_t m_t, uint32_t R, int pattern) {
  std::vector<uint32_t> r(m_t);
  for (uint64_t j = 0; j < m_t; j++) r[j] = pattern == 0 ? R : pattern == 1 ? (uint32_t)((uint64_t)R * (j % 4) / 3) : (j % 3 == 2 ? NO_RADIUS : R);
  return r;
}

int check(const char *name, const Table &T, const Table &Q, const Cost &C, uint32_t R) {
  const std::vector<std::string> t = T.strings(), q = Q.strings();
  std::vector<uint64_t> weight(Q.m());
  for (uint64_t i = 0; i < Q.m(); i++) weight[i] = i % 5 == 4 ? (1ull << 40) + i : 1 + (7 * i) % 11;
  int bad = 0;
  uint64_t total = 0;
  for (int pattern = 0; pattern < 3; pattern++) {
    std::vector<uint32_t> r = radii(T.m(), R, pattern);
    if (pattern == 1 && !r.empty()) r[0] = 70000;      // (the device entry's rule: above 65535 is no radius)
    const Totals got = tally(T.m(), T.cls.data(), T.off.data(), T.bytes(), Q.m(), Q.cls.data(), Q.off.data(), Q.bytes(), weight.data(),
                             weighted_per(C.sub, C.gap, C.ntrim, C.ctrim, r.data()));
    std::vector<uint32_t> t_count(T.m(), 0), q_degree(Q.m(), 0);
    std::vector<uint64_t> t_weight(T.m(), 0);
    for (uint64_t i = 0; i < Q.m(); i++)
      for (uint64_t j = 0; letters(q[i]) && j < T.m(); j++) {
        if (Q.cls[i] != T.cls[j] || !letters(t[j]) || r[j] > MAX_RADIUS || dist(q[i], t[j], C) > r[j]) continue;
        t_count[j]++; t_weight[j] += weight[i]; q_degree[i]++; total++;
      }
    bad += got.t_count != t_count;
    bad += got.t_weight != t_weight;
    bad += got.q_degree != q_degree;
    // at most one flush per (block, target that is hit)
    uint64_t hit = 0;
    for (uint32_t c : t_count) hit += c != 0;
    bad += got.flushes > hit * ((Q.m() + QUERIES - 1) / QUERIES);
  }
  std::printf("%s, R %u gap %u trim %u,%u: %llu counted, %d arrays differ\n", name, R, C.gap, C.ntrim, C.ctrim, (unsigned long long)total, bad);
  return bad;
}

int check_all(const char *name, const Table &T, const Table &Q) {
  int bad = 0;
  const std::vector<uint8_t> s1 = table(1), s2 = table(7);
  bad += check(name, T, Q, Cost{s1.data(), 12, 3, 2}, 48);
  bad += check(name, T, Q, Cost{s1.data(), 12, 3, 2}, 0);
  bad += check(name, T, Q, Cost{s2.data(), 5, 0, 0}, 93);
  bad += check(name, T, Q, Cost{s1.data(), 255, 16, 16}, 65535);
  return bad;
}

int check_refusals() {
  int bad = 0;
  const uint32_t ok[] = {0, 65535, NO_RADIUS}, above[] = {0, 65536}, below_none[] = {0xFFFFFFFEu};
  bad += refuse_radii(ok, 3) != nullptr;
  bad += refuse_radii(ok, 0) != nullptr;
  bad += refuse_radii(above, 2) == nullptr;
  bad += refuse_radii(above, 1) != nullptr;
  bad += refuse_radii(below_none, 1) == nullptr;
  std::printf("the radii the host entry refuses: %d differ\n", bad);
  return bad;
}

}  // namespace

int main() {
  int bad = check_refusals();
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
  {      // three classes of 256: the tiles of classes 1 and 9 are skipped by the waves of class 5
    Table T, Q;
    for (uint32_t c : {1u, 5u, 9u})
      for (uint32_t i = 0; i < 256; i++) T.add(c, code(i, true));
    for (uint32_t i = 0; i < 300; i++) Q.add(5, code(i, true));
    bad += check_all("a class between two", T, Q);
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

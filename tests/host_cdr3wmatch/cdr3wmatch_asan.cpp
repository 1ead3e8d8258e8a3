// Test-only, stand-alone (its own main; built with -fsanitize=address,undefined by `make asan`): the host walk of the weighted
// `match` over lists that put buckets on the tile and block edges (grids of 1, 3 and 6 blocks), leave buckets empty on either
// side, mix in nodes with a non-letter, and hold every length 1 .. 33, each checked against an all-pairs count whose distance is
// the contract read out (the gapped string built for every p).  Exit status 0: every list agreed and the sanitizers saw nothing.
#include "../host_cdr3walk/cdr3walk_check.h"

using namespace cdr3walk_check;

namespace {

int check(const char *name, const Table &T, const Table &Q, const Cost &C, uint32_t radius) {
  const Hits hits = match(T.m(), T.cls.data(), T.off.data(), T.bytes(), Q.m(), Q.cls.data(), Q.off.data(), Q.bytes(), weighted(C, radius));
  const std::vector<std::string> t = T.strings(), q = Q.strings();
  uint64_t total = 0;
  const int bad = rows_differ(hits, Q.m(), T.m(), [&](uint64_t i, uint64_t j, uint64_t *d) {
    return Q.cls[i] == T.cls[j] && letters(q[i]) && letters(t[j]) && (*d = dist(q[i], t[j], C)) <= radius;
  }, &total);
  std::printf("%s, radius %u gap %u trim %u,%u: %llu hits, %d rows differ\n", name, radius, C.gap, C.ntrim, C.ctrim,
              (unsigned long long)total, bad);
  return bad;
}

int check_all(const char *name, const Table &T, const Table &Q) {
  int bad = 0;
  const std::vector<uint8_t> s1 = table(1), s2 = table(7);
  bad += check(name, T, Q, Cost{s1.data(), 12, 3, 2}, 24);
  bad += check(name, T, Q, Cost{s2.data(), 5, 0, 0}, 40);
  bad += check(name, T, Q, Cost{s1.data(), 255, 16, 16}, 65535);
  bad += check(name, T, Q, Cost{s2.data(), 1, 1, 4}, 0);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  // one bucket of n targets around the tile size, queries at its ends and beside it; 1, 3 and 6 blocks of queries when swapped
  for (uint32_t n : {1u, 255u, 256u, 257u, 513u, 1500u}) {
    Table T, Q;
    for (uint32_t i = 0; i < n; i++) T.add(7, code(i, true));
    for (uint32_t i : {0u, n - 1, n, 7999u}) Q.add(7, code(i, true));
    Q.add(7, code(0).substr(1));
    Q.add(7, "");
    Q.add(7, std::string(33, 'A'));
    Q.add(7, "CASSaEQYF");
    Q.add(7, std::string("CAS\0EQYF", 8));
    bad += check_all("targets in one bucket", T, Q);
    bad += check_all("queries in one bucket", Q, T);
  }
  // a node with a non-letter at a tile's first and last slot, inside a full bucket
  {
    Table T, Q;
    for (uint32_t i = 0; i < 600; i++) T.add(3, i == 0 || i == 255 || i == 256 || i == 511 || i == 599 ? std::string("CASS*") + code(i).substr(5) : code(i));
    for (uint32_t i = 0; i < 300; i += 7) Q.add(3, code(i));
    Q.add(3, std::string("CASS\x80") + code(5).substr(5));
    bad += check_all("non-letters on the tile edges", T, Q);
    bad += check_all("non-letters on the tile edges, sides swapped", Q, T);
  }
  // buckets that one side lacks, between buckets both have; the first and the last bucket missing on either side
  for (uint32_t lack = 0; lack < 4; lack++) {
    Table T, Q;
    for (uint32_t c = 0; c < 12; c++) {
      const bool in_t = c % 3 != 1 && !(lack == 0 && c == 0) && !(lack == 1 && c == 11);
      const bool in_q = c % 4 != 2 && !(lack == 2 && c == 0) && !(lack == 3 && c == 11);
      for (uint32_t i = 0; in_t && i < 40 + 30 * c; i++) T.add(c, code(i, true));
      for (uint32_t i = 0; in_q && i < 50; i++) Q.add(c, code(i * 7, true));
    }
    bad += check_all("empty buckets", T, Q);
    bad += check_all("empty buckets, sides swapped", Q, T);
  }
  // every length 0 .. 33 against every length
  {
    Table T, Q;
    const std::string base = "CASSLAPGATNEKLFFGSGTQLSVLEDLKNVFPPE";
    for (size_t l = 0; l <= 33; l++) {
      T.add(0, base.substr(0, l));
      Q.add(0, base.substr(0, l / 2) + base.substr(base.size() - (l - l / 2)));
    }
    bad += check_all("every length", T, Q);
  }
  // no targets, no queries
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

// Test-only, stand-alone (its own main; built with -fsanitize=address,undefined by `make asan`): the host walk of `match`
// over lists that put buckets on the tile and block edges and leave buckets empty on either side, each checked against an
// all-pairs count.  Exit status 0: every list agreed and the sanitizers saw nothing.
#include "../host_cdr3walk/cdr3walk_check.h"

using namespace cdr3walk_check;

namespace {

int check(const char *name, const Table &T, const Table &Q) {
  int bad = 0;
  const std::vector<std::string> t = T.strings(), q = Q.strings();
  for (uint32_t metric = 0; metric < 2; metric++)
    for (uint32_t D = 0; D <= 2; D++) {
      const Hits hits = match(T.m(), T.cls.data(), T.off.data(), T.bytes(), Q.m(), Q.cls.data(), Q.off.data(), Q.bytes(), D, metric);
      uint64_t total = 0;
      bad += rows_differ(hits, Q.m(), T.m(), [&](uint64_t i, uint64_t j, uint64_t *d) {
        return Q.cls[i] == T.cls[j] && plain_hit(q[i], t[j], D, metric, d);
      }, &total);
      std::printf("%s metric %u D %u: %llu hits, %d rows differ\n", name, metric, D, (unsigned long long)total, bad);
    }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  // one bucket of n targets around the tile size, queries at its ends and beside it
  for (uint32_t n : {1u, 255u, 256u, 257u, 513u}) {
    Table T, Q;
    for (uint32_t i = 0; i < n; i++) T.add(7, code(i));
    for (uint32_t i : {0u, n - 1, n, 7999u}) Q.add(7, code(i));
    Q.add(7, code(0).substr(1));      // (one deletion: a Levenshtein hit alone)
    Q.add(7, "");
    Q.add(7, std::string(33, 'A'));
    bad += check("targets in one bucket", T, Q);
    bad += check("queries in one bucket", Q, T);
  }
  // buckets that one side lacks, between buckets both have; the first and the last bucket missing on either side
  for (uint32_t lack = 0; lack < 4; lack++) {
    Table T, Q;
    for (uint32_t c = 0; c < 12; c++) {
      const bool in_t = c % 3 != 1 && !(lack == 0 && c == 0) && !(lack == 1 && c == 11);
      const bool in_q = c % 4 != 2 && !(lack == 2 && c == 0) && !(lack == 3 && c == 11);
      for (uint32_t i = 0; in_t && i < 40 + 30 * c; i++) T.add(c, code(i));
      for (uint32_t i = 0; in_q && i < 50; i++) Q.add(c, code(i * 7));
    }
    bad += check("empty buckets", T, Q);
    bad += check("empty buckets, sides swapped", Q, T);
  }
  // no targets, no queries
  {
    Table T, Q, none;
    T.add(1, code(1));
    Q.add(1, code(2));
    bad += check("no targets", none, Q);
    bad += check("no queries", T, none);
  }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

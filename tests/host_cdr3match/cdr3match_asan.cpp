// Test-only, stand-alone (its own main; built with -fsanitize=address,undefined by `make asan`): the host walk of `match`
// over lists that put buckets on the tile and block edges and leave buckets empty on either side, each checked against an
// all-pairs count.  Exit status 0: every list agreed and the sanitizers saw nothing.
#include <cstdio>
#include <string>

#include "cdr3match_walk.h"

using namespace cdr3match_host;

namespace {

struct Table {
  std::vector<uint32_t> cls;
  std::vector<uint64_t> off{0};
  std::string text;
  void add(uint32_t c, const std::string &s) { cls.push_back(c); text += s; off.push_back(text.size()); }
  uint64_t m() const { return cls.size(); }
  std::string str(uint64_t i) const { return text.substr(off[i], off[i + 1] - off[i]); }
};

// string number i of one length: three base-20 digits between fixed ends (two numbers differ in 1 to 3 places)
std::string code(uint32_t i, const std::string &tail = "EQYF") {
  static const char amino[] = "ACDEFGHIKLMNPQRSTVWY";
  std::string s = "CASS";
  for (int d = 0; d < 3; d++, i /= 20) s += amino[i % 20];
  return s + tail;
}

uint64_t lev(const std::string &a, const std::string &b) {
  std::vector<uint64_t> prev(b.size() + 1), cur(b.size() + 1);
  std::iota(prev.begin(), prev.end(), 0);
  for (size_t i = 1; i <= a.size(); i++) {
    cur[0] = i;
    for (size_t j = 1; j <= b.size(); j++) cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])});
    prev.swap(cur);
  }
  return prev[b.size()];
}

bool pair_hits(const std::string &a, const std::string &b, uint32_t D, uint32_t metric) {
  if (a.empty() || b.empty() || a.size() > MAX_LEN || b.size() > MAX_LEN) return false;
  if (metric == METRIC_LEVENSHTEIN) return lev(a, b) <= D;
  if (a.size() != b.size()) return false;
  uint32_t d = 0;
  for (size_t p = 0; p < a.size(); p++) d += a[p] != b[p];
  return d <= D;
}

int check(const char *name, const Table &T, const Table &Q) {
  int bad = 0;
  for (uint32_t metric = 0; metric < 2; metric++)
    for (uint32_t D = 0; D <= 2; D++) {
      const auto hits = match(T.m(), T.cls.data(), T.off.data(), reinterpret_cast<const uint8_t *>(T.text.data()), Q.m(), Q.cls.data(),
                              Q.off.data(), reinterpret_cast<const uint8_t *>(Q.text.data()), D, metric);
      uint64_t total = 0;
      for (uint64_t i = 0; i < Q.m(); i++) {
        std::vector<uint32_t> want;
        for (uint64_t j = 0; j < T.m(); j++)
          if (Q.cls[i] == T.cls[j] && pair_hits(Q.str(i), T.str(j), D, metric)) want.push_back((uint32_t)j);
        if (want != hits[i]) bad++;
        total += want.size();
      }
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

// Test-only, stand-alone (its own main; built with -fsanitize=address,undefined by `make asan`): the host walk of the weighted
// CDR3 network over lists that put a node's own entry on a tile's first and last slot (classes of 255, 256, 257, 513 and 1 500
// nodes of three lengths: 1, 3 and 6 blocks), mix in nodes with a non-letter on those slots, spread classes over block edges
// and hold every length 0 .. 33, each checked against an all-pairs count whose distance is the contract read out (the gapped
// string built for every p) and for symmetry.  Exit status 0: every list agreed and the sanitizers saw nothing.
#include "../host_cdr3walk/cdr3walk_check.h"

using namespace cdr3walk_check;

namespace {

int check(const char *name, const Table &N, const Cost &C, uint32_t radius) {
  const Hits hits = network(N.m(), N.cls.data(), N.off.data(), N.bytes(), weighted(C, radius));
  const std::vector<std::string> str = N.strings();
  uint64_t total = 0;
  int bad = rows_differ(hits, N.m(), N.m(), [&](uint64_t i, uint64_t j, uint64_t *d) {
    return i != j && N.cls[i] == N.cls[j] && letters(str[i]) && letters(str[j]) && (*d = dist(str[i], str[j], C)) <= radius;
  }, &total);
  bad += not_symmetric(hits);
  std::printf("%s, radius %u gap %u trim %u,%u: %llu entries, %d rows differ\n", name, radius, C.gap, C.ntrim, C.ctrim,
              (unsigned long long)total, bad);
  return bad;
}

int check_all(const char *name, const Table &N) {
  int bad = 0;
  const std::vector<uint8_t> s1 = table(1), s2 = table(7);
  bad += check(name, N, Cost{s1.data(), 12, 3, 2}, 24);
  bad += check(name, N, Cost{s2.data(), 5, 0, 0}, 40);
  bad += check(name, N, Cost{s1.data(), 255, 16, 16}, 65535);
  bad += check(name, N, Cost{s2.data(), 1, 1, 4}, 0);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  // one class of n nodes around the tile size (a node's own entry on slot 0 and on slot 255), out-of-reach nodes behind it
  for (uint32_t n : {1u, 2u, 255u, 256u, 257u, 513u, 1500u}) {
    Table N;
    for (uint32_t i = 0; i < n; i++) N.add(7, code(i % 700, true));      // (from 700 on: equal strings, linked at 0)
    N.add(7, "");
    N.add(7, std::string(33, 'A'));
    if (n <= 513) {
      bad += check_all("one class", N);
    } else {      // (six blocks: under the default cost alone, to keep the run short)
      const std::vector<uint8_t> s1 = table(1);
      bad += check("one class, six blocks", N, Cost{s1.data(), 12, 3, 2}, 24);
    }
  }
  // a node with a non-letter at a tile's first and last slot, inside a full class
  {
    Table N;
    for (uint32_t i = 0; i < 600; i++)
      N.add(3, i == 0 || i == 255 || i == 256 || i == 511 || i == 599 ? std::string("CASS") + "*a\x80_\x01"[i % 5] + code(i, true).substr(5) : code(i, true));
    N.add(3, std::string("CAS\0EQYF", 8));
    bad += check_all("non-letters on the tile edges", N);
  }
  // classes of growing size in interleaved rank order: class starts inside tiles, blocks that span several classes
  {
    Table N;
    for (uint32_t i = 0; i < 700; i++) N.add(i % 12 < 3 ? 0x80000000u : i % 12, code(i / 3, true));
    bad += check_all("classes over block edges", N);
  }
  // every length 0 .. 33 against every length
  {
    Table N;
    const std::string base = "CASSLAPGATNEKLFFGSGTQLSVLEDLKNVFPPE";
    for (size_t l = 0; l <= 33; l++) {
      N.add(0, base.substr(0, l));
      N.add(0, base.substr(0, l / 2) + base.substr(base.size() - (l - l / 2)));
    }
    bad += check_all("every length", N);
  }
  // no nodes
  bad += check_all("no nodes", Table{});
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

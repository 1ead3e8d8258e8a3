// Test-only, stand-alone (its own main; built with -fsanitize=address,undefined by `make asan`): the host walk of the CDR3
// network under its two plain metrics (../host_cdr3walk/cdr3walk_host.h: Within with Hamming and with Levenshtein) at D = 1
// and 2, over lists that put a node's own entry on a tile's first and last slot (one class of 1, 2, 254 .. 257 and 513 nodes,
// and of 1 500 — six blocks — under D = 1), hold three lengths in one class and equal strings, put nodes of length 0 and 33 on
// the edge slots behind the class and spread a dozen classes, some empty, over block edges; each checked against an all-pairs
// count and for symmetry.  Exit status 0: every list agreed and the sanitizers saw nothing.
#include "../host_cdr3walk/cdr3walk_check.h"

using namespace cdr3walk_check;

namespace {

int check(const char *name, const Table &N, uint32_t max_d = 2) {
  int bad = 0;
  const std::vector<std::string> str = N.strings();
  for (uint32_t metric : {METRIC_HAMMING, METRIC_LEVENSHTEIN})
    for (uint32_t D = 1; D <= max_d; D++) {
      const Hits hits = network(N.m(), N.cls.data(), N.off.data(), N.bytes(), D, metric);
      uint64_t total = 0;
      bad += rows_differ(hits, N.m(), N.m(), [&](uint64_t i, uint64_t j, uint64_t *d) {
        return i != j && N.cls[i] == N.cls[j] && plain_hit(str[i], str[j], D, metric, d);
      }, &total);
      bad += not_symmetric(hits);
      std::printf("%s metric %u D %u: %llu entries, %d rows differ\n", name, metric, D, (unsigned long long)total, bad);
    }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  // one class of n nodes of three lengths around the tile size (a node's own entry on slot 0 and on slot 255 of a tile), nodes
  // of length 0 and 33 behind it: on a tile's last and first slot at 254, 255 and 256; from 700 on the strings repeat (equal
  // strings, linked at 0)
  for (uint32_t n : {1u, 2u, 254u, 255u, 256u, 257u, 513u, 1500u}) {
    Table N;
    N.add(7, "");
    for (uint32_t i = 0; i < n; i++) N.add(7, code(i % 700, true));
    N.add(7, std::string(33, 'A'));
    if (n <= 513) bad += check("one class", N);
    else bad += check("one class, six blocks", N, 1);
  }
  // a dozen classes of growing size, three of them empty, their ranks interleaved: class starts inside tiles, blocks that span
  // several classes
  {
    Table N, M;
    for (uint32_t c = 0; c < 12; c++)
      for (uint32_t i = 0; c % 4 != 2 && i < 40 + 30 * c; i++) N.add(c, code(i, true));
    const std::vector<std::string> str = N.strings();
    for (uint64_t k = 0; k < 7; k++)
      for (uint64_t i = k; i < N.m(); i += 7) M.add(N.cls[i], str[i]);
    bad += check("classes over block edges", M);
  }
  // no nodes
  bad += check("no nodes", Table{});
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

// Test-only, stand-alone (its own main; built with -fsanitize=address,undefined by `make asan`): the host walk of the weighted
// CDR3 network over lists that put a node's own entry on a tile's first and last slot (classes of 255, 256, 257, 513 and 1 500
// nodes of three lengths: 1, 3 and 6 blocks), mix in nodes with a non-letter on those slots, spread classes over block edges
// and hold every length 0 .. 33, each checked against an all-pairs count whose distance is the contract read out (the gapped
// string built for every p) and for symmetry.  Exit status 0: every list agreed and the sanitizers saw nothing.
#include <cstdio>
#include <string>

#include "cdr3wnet_walk.h"

using namespace cdr3wnet_host;

namespace {

struct Nodes {
  std::vector<uint32_t> cls;
  std::vector<uint64_t> off{0};
  std::string text;
  void add(uint32_t c, const std::string &s) { cls.push_back(c); text += s; off.push_back(text.size()); }
  uint64_t m() const { return cls.size(); }
  std::string str(uint64_t i) const { return text.substr(off[i], off[i + 1] - off[i]); }
};

// string number i: three base-20 digits between fixed ends (two numbers differ in 1 to 3 places), and a tail of 2 + i % 3 letters
std::string code(uint32_t i) {
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
      sub[x * SUB_DIM + y] = sub[y * SUB_DIM + x] = (uint8_t)(seed >> 24) % (seed & 4 ? 13 : 256);
    }
  return sub;
}

bool letters(const std::string &s) {
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
      const size_t i = k < p ? k : k - d;      // the position in a
      if (i < C.ntrim || i + C.ctrim >= la) continue;
      sum += C.sub[(gapped[k] & 31) * SUB_DIM + (b[k] & 31)];
    }
    best = std::min(best, sum);
  }
  return d * C.gap + best;
}

int check(const char *name, const Nodes &N, const Cost &C, uint32_t radius) {
  int bad = 0;
  const auto hits = network(N.m(), N.cls.data(), N.off.data(), reinterpret_cast<const uint8_t *>(N.text.data()), C, radius);
  uint64_t total = 0;
  std::vector<std::string> strings;
  std::vector<bool> in;      // in reach, letters alone
  for (uint64_t i = 0; i < N.m(); i++) {
    strings.push_back(N.str(i));
    in.push_back(!strings[i].empty() && strings[i].size() <= MAX_LEN && letters(strings[i]));
  }
  for (uint64_t i = 0; i < N.m(); i++) {
    std::vector<std::pair<uint32_t, uint32_t>> want, got;
    const std::string &a = strings[i];
    for (uint64_t j = 0; j < N.m(); j++) {
      const std::string &b = strings[j];
      if (i == j || N.cls[i] != N.cls[j] || !in[i] || !in[j]) continue;
      const size_t apart = a.size() > b.size() ? a.size() - b.size() : b.size() - a.size();
      if (apart * C.gap > radius) continue;      // (every cell is >= 0: the gap alone is too much)
      const uint64_t d = dist(a, b, C);
      if (d <= radius) want.push_back({(uint32_t)j, (uint32_t)d});
    }
    for (const Hit &h : hits[i]) got.push_back({h.node, h.dist});
    if (want != got) bad++;
    total += want.size();
    for (const Hit &h : hits[i]) {      // symmetric, with one distance
      bool back = false;
      for (const Hit &g : hits[h.node]) back |= g.node == i && g.dist == h.dist;
      if (!back) bad++;
    }
  }
  std::printf("%s, radius %u gap %u trim %u,%u: %llu entries, %d rows differ\n", name, radius, C.gap, C.ntrim, C.ctrim,
              (unsigned long long)total, bad);
  return bad;
}

int check_all(const char *name, const Nodes &N) {
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
    Nodes N;
    for (uint32_t i = 0; i < n; i++) N.add(7, code(i % 700));      // (from 700 on: equal strings, linked at 0)
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
    Nodes N;
    for (uint32_t i = 0; i < 600; i++)
      N.add(3, i == 0 || i == 255 || i == 256 || i == 511 || i == 599 ? std::string("CASS") + "*a\x80_\x01"[i % 5] + code(i).substr(5) : code(i));
    N.add(3, std::string("CAS\0EQYF", 8));
    bad += check_all("non-letters on the tile edges", N);
  }
  // classes of growing size in interleaved rank order: class starts inside tiles, blocks that span several classes
  {
    Nodes N;
    for (uint32_t i = 0; i < 700; i++) N.add(i % 12 < 3 ? 0x80000000u : i % 12, code(i / 3));
    bad += check_all("classes over block edges", N);
  }
  // every length 0 .. 33 against every length
  {
    Nodes N;
    const std::string base = "CASSLAPGATNEKLFFGSGTQLSVLEDLKNVFPPE";
    for (size_t l = 0; l <= 33; l++) {
      N.add(0, base.substr(0, l));
      N.add(0, base.substr(0, l / 2) + base.substr(base.size() - (l - l / 2)));
    }
    bad += check_all("every length", N);
  }
  // no nodes
  bad += check_all("no nodes", Nodes{});
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

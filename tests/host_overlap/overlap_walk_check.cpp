// Test-only, stand-alone: overlap_host_pairs (overlap_host.cpp: the pair kernel's walk with the look-ups its lanes make) over
// the empty-group and tile-edge lists of tests/overlap_util.py, written again here, against a loop over every group's pairs.
// `make asan` builds it with -fsanitize=address,undefined: the cell arrays and the staged ends are heap blocks of their exact
// size, so a look-up past `ends` or `cell_off` that a GPU survives silently stops this program.  Exit status 0: all lists agree.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

extern "C" int overlap_host_pairs(uint32_t n_groups, const uint32_t *cell_off, const uint32_t *cell_sample, const uint32_t *cell_weight,
                                  uint32_t S, uint32_t smax, uint32_t grid, uint64_t *planes);

namespace {

using Group = std::map<uint32_t, uint32_t>;      // sample -> weight, samples ascending
using Groups = std::vector<Group>;

void append(Groups &to, const Groups &from) { to.insert(to.end(), from.begin(), from.end()); }

Groups tail3() { return {{{1, 4}}, {{0, 2}, {2, 9}}, {}, {{0, 1}, {1, 2}, {2, 3}}, {{2, 8}}}; }

Groups lookup_groups(uint32_t empties, uint32_t front) {
  Groups g;
  for (uint32_t k = 0; k < front; k++) g.push_back({{k % 3, 1 + k % 7}});
  g.push_back({{0, 3}, {2, 5}});
  g.insert(g.end(), empties, Group{});
  g.push_back({{0, 11}, {1, 13}, {2, 17}});
  for (uint32_t k = 0; k < 5; k++) g.push_back({{k % 3, 20 + k}});
  return g;
}

Groups body3() {
  Groups g;
  for (uint32_t k = 0; k < 40; k++) g.push_back({{k % 3, 2 + k % 5}});
  append(g, tail3());
  return g;
}

Group full_group(uint32_t r) {
  Group g;
  for (uint32_t a = 0; a < 64; a++) g[a] = 1 + (7 * a + 3 * r) % 61;
  return g;
}

Groups tile_edge_groups(uint32_t front) {
  Groups g;
  for (uint32_t k = 0; k < front; k++) g.push_back({{k % 64, 1 + k % 9}});
  g.push_back(full_group(front));
  g.push_back({{5, 2}});
  g.push_back({{0, 1}, {63, 4}});
  return g;
}

Groups tile_edge_long_groups() {
  Groups g;
  for (uint32_t r = 1; r <= 160; r++) {
    for (uint32_t k = 0; k < r % 37; k++) g.push_back({{(r + k) % 64, 1 + (r * k) % 11}});
    g.push_back(full_group(r));
  }
  return g;
}

uint32_t smax_for(uint32_t S) { return S <= 8 ? 8 : S <= 16 ? 16 : S <= 32 ? 32 : 64; }

int check(const char *name, const Groups &groups, uint32_t S) {
  std::vector<uint32_t> off{0}, smp, wt;
  std::vector<uint64_t> want((size_t)5 * S * S, 0);
  for (const Group &per : groups) {
    for (const auto &[a, wa] : per) {
      smp.push_back(a); wt.push_back(wa);
      for (const auto &[b, wb] : per) {
        const uint64_t p = (uint64_t)wa * wb;
        const size_t at = (size_t)a * S + b;
        want[at] += 1;
        want[(size_t)S * S + at] += wa;
        want[(size_t)2 * S * S + at] += wa < wb ? wa : wb;
        want[(size_t)3 * S * S + at] += p & 0xFFFFFFFFull;
        want[(size_t)4 * S * S + at] += p >> 32;
      }
    }
    off.push_back((uint32_t)smp.size());
  }
  smp.shrink_to_fit(); wt.shrink_to_fit(); off.shrink_to_fit();
  int bad = 0;
  for (uint32_t smax : {smax_for(S), 64u})
    for (uint32_t grid : {1u, 3u, 2048u}) {
      std::vector<uint64_t> got((size_t)5 * S * S, 0);
      const int rc = overlap_host_pairs((uint32_t)groups.size(), off.data(), smp.data(), wt.data(), S, smax, grid, got.data());
      if (rc || got != want) {
        std::printf("FAIL %s: smax %u grid %u (rc %d)\n", name, smax, grid, rc);
        bad = 1;
      }
    }
  std::printf("%s %s: %zu groups, %zu cells\n", bad ? "FAIL" : "ok  ", name, groups.size(), smp.size());
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  char name[64];
  for (uint32_t front : {0u, 512u})
    for (uint32_t e : {253u, 254u, 255u, 256u}) {
      std::snprintf(name, sizeof name, "lookup front %u empties %u", front, e);
      bad |= check(name, lookup_groups(e, front), 3);
    }
  Groups lead(300, Group{}), trail = body3(), singles;
  append(lead, body3());
  trail.insert(trail.end(), 300, Group{});
  for (uint32_t k = 0; k < 256; k++) singles.push_back({{k % 3, 1 + k % 9}});
  singles.push_back({{0, 7}, {1, 8}, {2, 9}});
  append(singles, tail3());
  bad |= check("leading empties", lead, 3);
  bad |= check("trailing empties", trail, 3);
  bad |= check("a full tile of singles", singles, 3);
  for (uint32_t front : {193u, 224u, 255u}) {
    std::snprintf(name, sizeof name, "tile edge front %u", front);
    bad |= check(name, tile_edge_groups(front), 64);
  }
  bad |= check("tile edge long", tile_edge_long_groups(), 64);
  std::printf(bad ? "overlap_walk_check: FAILED\n" : "overlap_walk_check: all lists agree\n");
  return bad;
}

// Test-only, stand-alone: rarefy_host_downsample (rarefy_host.cpp: the primitive's steps with the look-ups its lanes make) over
// tables at the tile's edges, behind the staged slots and through runs of weight-0 rows, against every key sorted.
// `make asan` builds it with -fsanitize=address,undefined: the offsets, the staged ends, the histograms and the candidates are
// heap blocks of their exact size, so a look-up past one that a GPU survives silently stops this program.  Exit status 0: all
// tables agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
uint32_t rarefy_host_tile(void);
uint32_t rarefy_host_slots(void);
uint32_t rarefy_host_grid(void);
uint64_t rarefy_host_key(uint64_t seed, uint64_t s, uint64_t r);
int rarefy_host_downsample(uint32_t S, uint32_t m, const uint32_t *sample, const uint64_t *weight, const uint64_t *depth, uint64_t seed,
                           uint32_t grid, uint64_t *kept, uint64_t *reads, uint64_t *depth_used, uint64_t *threshold, uint32_t *levels_out);
}

namespace {

struct Table {
  uint32_t S = 1;
  std::vector<uint32_t> sample;
  std::vector<uint64_t> weight, depth;
  void rows(uint32_t s, uint32_t n, uint64_t w) { sample.insert(sample.end(), n, s); weight.insert(weight.end(), n, w); }
};

int check(const char *name, Table T, uint64_t seed) {
  const uint32_t S = T.S, m = (uint32_t)T.sample.size();
  std::vector<uint64_t> want_kept(m, 0), want_reads(S, 0), want_used(S), want_thr(S);
  for (uint32_t s = 0; s < S; s++) {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> owner;
    for (uint32_t i = 0; i < m; i++)
      if (T.sample[i] == s)
        for (uint64_t k = 0; k < T.weight[i]; k++) { keys.push_back(rarefy_host_key(seed, s, keys.size())); owner.push_back(i); }
    const uint64_t X = keys.size(), n = std::min<uint64_t>(T.depth[s], X);
    std::vector<uint64_t> sorted(keys);
    std::sort(sorted.begin(), sorted.end());
    want_reads[s] = X; want_used[s] = n; want_thr[s] = n == X ? ~0ull : sorted[n];
    for (uint64_t r = 0; r < X; r++)
      if (n == X || keys[r] < want_thr[s]) want_kept[owner[r]]++;
  }
  T.sample.shrink_to_fit(); T.weight.shrink_to_fit();
  int bad = 0;
  for (uint32_t grid : {1u, 3u, rarefy_host_grid()}) {
    std::vector<uint64_t> kept(m, 7), reads(S), used(S), thr(S);
    const int rc = rarefy_host_downsample(S, m, T.sample.data(), T.weight.data(), T.depth.data(), seed, grid, kept.data(), reads.data(),
                                          used.data(), thr.data(), nullptr);
    if (rc || kept != want_kept || reads != want_reads || used != want_used || thr != want_thr) {
      std::printf("FAIL %s: grid %u (rc %d)\n", name, grid, rc);
      bad = 1;
    }
  }
  std::printf("%s %s: %u rows\n", bad ? "FAIL" : "ok  ", name, m);
  return bad;
}

}  // namespace

int main() {
  const uint32_t TILE = rarefy_host_tile(), SLOTS = rarefy_host_slots();
  int bad = 0;
  char name[64];
  for (int d = -1; d <= 1; d++) {      // a row, and a sample, ending at TILE - 1, TILE, TILE + 1
    Table T;
    T.S = 2; T.depth = {TILE / 2, 100};
    T.rows(0, 1, TILE + d); T.rows(0, 3, 1); T.rows(1, 5, 40);
    std::snprintf(name, sizeof name, "row end at TILE%+d", d);
    bad |= check(name, T, 3);
    Table U;
    U.S = 3; U.depth = {TILE / 3, 7, 0};
    U.rows(0, 10, 10); U.rows(0, 1, TILE + d - 100); U.rows(2, 50, 3);
    std::snprintf(name, sizeof name, "sample end at TILE%+d", d);
    bad |= check(name, U, 4);
  }
  {
    Table T;
    T.depth = {TILE};
    T.rows(0, 1, 1); T.rows(0, 1, 3 * TILE + 5); T.rows(0, 1, 1);
    bad |= check("a heavy row between two light ones", T, 5);
  }
  for (uint32_t n : {TILE, SLOTS + 1, SLOTS, SLOTS - 1}) {
    Table T;
    T.depth = {n / 2};
    T.rows(0, n, 1);
    std::snprintf(name, sizeof name, "%u rows of weight 1", n);
    bad |= check(name, T, 6);
  }
  for (uint32_t zeros : {SLOTS - 1, SLOTS, SLOTS + 1, 3 * SLOTS}) {
    Table T;
    T.S = 2; T.depth = {9, 30};
    T.rows(0, zeros, 0); T.rows(0, 2, 10); T.rows(0, zeros, 0); T.rows(0, 1, 5); T.rows(1, zeros, 0); T.rows(1, 60, 1); T.rows(1, zeros, 0);
    std::snprintf(name, sizeof name, "runs of %u rows of weight 0", zeros);
    bad |= check(name, T, 7);
  }
  {
    Table T;
    T.S = 4; T.depth = {0, 5, 1000000, 4000};
    T.rows(0, 3, 9); T.rows(2, 20, 11); T.rows(3, 1, 5 * TILE + 3); T.rows(3, 700, 2);
    bad |= check("depth 0, a sample without rows, depth above X, a real depth", T, 8);
  }
  std::printf(bad ? "rarefy_walk_check: FAILED\n" : "rarefy_walk_check: all tables agree\n");
  return bad;
}

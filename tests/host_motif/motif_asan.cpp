// Test-only, a program of its own (`make asan`), never loaded into python: the shared per-unit code over every length, trim
// and k, on units that end flush with their heap blocks, under AddressSanitizer and UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_motif_core.h"

extern "C" int motif_host_unit_motifs(const uint8_t *s, uint64_t len, uint32_t N, uint32_t C, uint32_t k, uint32_t *out);
extern "C" int motif_host_takes_part(const uint8_t *s, uint64_t len);

int main() {
  using namespace dcrx_motif;
  uint64_t calls = 0, motifs = 0;
  for (uint32_t L = 0; L <= MAX_LEN + 1; L++) {
    std::vector<uint8_t> unit(L);      // exactly L bytes: a read past the unit is a read past the block
    for (uint32_t p = 0; p < L; p++) unit[p] = (uint8_t)('A' + (p * 7 + L) % 5);
    const int takes = motif_host_takes_part(unit.data(), L);
    if (takes != (L >= 1 && L <= MAX_LEN)) { std::printf("takes_part wrong at L = %u\n", L); return 1; }
    for (uint32_t N = 0; N <= MAX_TRIM; N++)
      for (uint32_t C = 0; C <= MAX_TRIM; C++)
        for (uint32_t k = K_MIN; k <= K_MAX; k++) {
          std::vector<uint32_t> out(MAX_WINDOWS);
          const int got = motif_host_unit_motifs(unit.data(), L, N, C, k, out.data());
          calls++;
          if (!takes) { if (got != -1) return 1; continue; }
          if (got < 0 || (uint32_t)got > window_count(L, N, C, k)) { std::printf("count wrong at L = %u\n", L); return 1; }
          motifs += (uint64_t)got;
        }
  }
  std::printf("motif_asan: %llu calls, %llu motifs, clean\n", (unsigned long long)calls, (unsigned long long)motifs);
  return 0;
}

// Test-only, a program of its own (`make`, `make asan`), never loaded into python: the motif groups' host code in the shared
// header — which (k, code) are motifs of K, the first fault of a list of selected motifs, and the members' sort constants —
// on lists that end flush with their heap blocks.
//   motif_groups_host                       the self-checks; prints "motif_groups_host: ... ok"
//   motif_groups_host K_MASK k:code ...     prints the index of the list's first fault, or its length where it is in order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_motif_core.h"

using namespace dcrx_motif;

static uint64_t fault_of(uint32_t k_mask, const std::vector<uint32_t> &k, const std::vector<uint32_t> &code) {
  // exactly S entries each: a read past the list is a read past the block
  return first_selected_fault(k.size(), k.data(), code.data(), k_mask);
}

static int fail(const char *what) {
  std::printf("motif_groups_host: %s\n", what);
  return 1;
}

int main(int argc, char **argv) {
  if (argc > 1) {
    const uint32_t k_mask = (uint32_t)std::strtoul(argv[1], nullptr, 0);
    std::vector<uint32_t> k, code;
    for (int a = 2; a < argc; a++) {
      const char *colon = std::strchr(argv[a], ':');
      if (!colon) return fail("a selected motif is k:code");
      k.push_back((uint32_t)std::strtoul(argv[a], nullptr, 10));
      code.push_back((uint32_t)std::strtoul(colon + 1, nullptr, 10));
    }
    std::printf("%llu\n", (unsigned long long)fault_of(k_mask, k, code));
    return 0;
  }
  uint64_t checks = 0;
  // which (k, code) are motifs of K
  for (uint32_t k_mask = 0; k_mask < 64; k_mask++)
    for (uint32_t k = 0; k < 8; k++) {
      const bool in_k = k >= 2 && k <= 4 && (k_mask >> k & 1u);
      uint32_t codes = 1;
      for (uint32_t i = 0; i < k && i < 4; i++) codes *= 26;
      if (k >= 2 && k <= 4 && codes_of(k) != codes) return fail("codes_of");
      if (k < 2 || k > 4) { if (codes_of(k) != 0) return fail("codes_of outside K"); codes = 26; }
      for (uint32_t code : {0u, 1u, codes - 1, codes, codes + 1, 0xFFFFFFFFu}) {
        if (is_motif(k_mask, k, code) != (in_k && code < codes)) return fail("is_motif");
        checks++;
      }
    }
  // the whole list of K = {2, 3, 4} in motif order is in order, and its numbers are 0 .. MOTIFS - 1
  {
    std::vector<uint32_t> k, code;
    for (uint32_t id = 0; id < MOTIFS; id++) { k.push_back(id_k(id)); code.push_back(id_code(id)); }
    if (fault_of(K_MASK_ALL, k, code) != MOTIFS) return fail("every motif in order");
    if (motif_id(k.back(), code.back()) != MOTIFS - 1) return fail("the last motif's number");
    // one pair swapped, one motif twice, a k outside K, a code outside its k: the fault is where it stands
    for (uint64_t at : {(uint64_t)1, (uint64_t)BASE3, (uint64_t)BASE4, (uint64_t)MOTIFS - 1}) {
      std::vector<uint32_t> k2 = k, c2 = code;
      std::swap(k2[at], k2[at - 1]); std::swap(c2[at], c2[at - 1]);
      if (fault_of(K_MASK_ALL, k2, c2) != at) return fail("a swapped pair");
      k2 = k; c2 = code;
      k2[at] = k2[at - 1]; c2[at] = c2[at - 1];
      if (fault_of(K_MASK_ALL, k2, c2) != at) return fail("a motif twice");
      c2 = code; k2 = k;
      c2[at] = codes_of(k2[at]);
      if (fault_of(K_MASK_ALL, k2, c2) != at) return fail("a code outside its k");
      checks += 3;
    }
    if (fault_of(1u << 3, k, code) != 0) return fail("a k outside K at the front");
    std::vector<uint32_t> k3(k.begin() + BASE3, k.begin() + BASE4), c3(code.begin() + BASE3, code.begin() + BASE4);
    if (fault_of(1u << 3, k3, c3) != k3.size()) return fail("K = {3} alone");
    k3.push_back(4); c3.push_back(0);
    if (fault_of(1u << 3, k3, c3) != k3.size() - 1) return fail("a k outside K at the end");
    checks += 3;
  }
  if (fault_of(K_MASK_ALL, {}, {}) != 0) return fail("the empty list");
  // the members' sort: every row lies below the mark of an unused slot under the sorted bits, and one sort holds the keys
  const uint64_t low = NO_MEMBER_ROW & ((1ull << MEMBER_ROW_BITS) - 1);
  if (low <= MOTIFS - 1) return fail("NO_MEMBER_ROW");
  if (MAX_MEMBER_KEYS != (1ull << 31) || MAX_UNITS + MAX_UNITS > MAX_MEMBER_KEYS) return fail("MAX_MEMBER_KEYS");
  std::printf("motif_groups_host: %llu checks, ok\n", (unsigned long long)checks);
  return 0;
}

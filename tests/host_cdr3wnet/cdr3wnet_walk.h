// Test-only: the weighted walk of the CDR3 network (cdr3_walk_kernel<WRITE, Within, Weighted>, decombinator_amd/csrc/dcrx_cdr3walk.h)
// step by step on the host, with the kernel's own look-ups (dcrx_cdr3match_core.h) and pair test (dcrx_cdr3w_core.h): keys, a
// stable sort of (key, rank) by class, packed strings, the class starts (the run marks, max-scanned), then per block of 256
// sorted nodes the tiles of 256 entries of the SAME table from the block's first node's class start, with the letters test at
// staging, per wave of 64 lanes the skip, per lane the class, its own entry left out, the length window and weighted_within.
// Every array access is a std::vector::at(); a staged string is copied into a buffer of exactly 32 bytes.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_cdr3match_core.h"
#include "../../decombinator_amd/csrc/dcrx_cdr3w_core.h"

namespace cdr3wnet_host {

using namespace dcrx_cdr3match;
using namespace dcrx_cdr3w;
constexpr uint32_t WAVE = 64;

struct Table {      // the nodes, sorted by class
  std::vector<uint64_t> key;
  std::vector<uint32_t> idx, bstart;
  std::vector<uint32_t> words;      // WORDS per sorted position
};

struct Hit {
  uint32_t node, dist;
};

inline Table prepare(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text) {
  std::vector<uint64_t> key(m);
  for (uint64_t e = 0; e < m; e++) key[e] = node_key(cls[e], off[e + 1] < off[e] ? (uint64_t)MAX_LEN + 1 : off[e + 1] - off[e]);
  Table S;
  S.idx.resize(m);
  std::iota(S.idx.begin(), S.idx.end(), 0u);
  std::stable_sort(S.idx.begin(), S.idx.end(), [&](uint32_t a, uint32_t b) { return key_class(key[a]) < key_class(key[b]); });
  S.key.resize(m); S.bstart.resize(m); S.words.resize(m * WORDS);
  for (uint64_t s = 0; s < m; s++) {
    const uint32_t e = S.idx[s];
    S.key[s] = key[e];
    S.bstart[s] = s && key_class(S.key[s]) == key_class(S.key[s - 1]) ? S.bstart[s - 1] : (uint32_t)s;
    const bool out = key[e] == KEY_OUT_OF_REACH;
    pack(text + (out ? 0 : off[e]), out ? 0 : key_length(key[e]), &S.words[s * WORDS]);
  }
  return S;
}

// per node rank its neighbours (rank and distance, in the order the walk meets them)
inline std::vector<std::vector<Hit>> walk(const Table &X, const Cost &C, uint32_t radius) {
  const uint32_t n = (uint32_t)X.key.size();
  std::vector<std::vector<Hit>> hits(n);
  for (uint32_t s0 = 0; s0 < n; s0 += QUERIES) {
    const Range R = within_range<true>(X.key.data(), n, s0, X.bstart.data());
    for (uint32_t t = R.first; t < n; t += TILE) {
      if (!goes_on<true>(R, X.key.at(t))) break;
      const uint32_t tile_n = std::min<uint32_t>(TILE, n - t);
      std::vector<uint64_t> staged(tile_n);      // the keys as staged: length 0 for an entry with a non-letter
      for (uint32_t q = 0; q < tile_n; q++) {
        const uint64_t key = X.key.at(t + q);
        staged.at(q) = letters_only(&X.words.at((t + q) * WORDS), key_length(key)) ? key : key & ~LEN_MASK;
      }
      for (uint32_t w0 = s0; w0 < s0 + QUERIES; w0 += WAVE) {
        auto k_of = [&](uint32_t s) { return key_class(s < n ? X.key.at(s) : KEY_OUT_OF_REACH); };
        const uint64_t w_lo = k_of(w0), w_hi = k_of(w0 + WAVE - 1);
        if (wave_skips(key_class(staged.at(0)), key_class(staged.at(tile_n - 1)), w_lo, w_hi)) continue;
        for (uint32_t s = w0; s < std::min(w0 + WAVE, n); s++) {
          const uint64_t key_own = X.key.at(s);
          if (key_own == KEY_OUT_OF_REACH) continue;
          const uint32_t len_own = key_length(key_own);
          const uint32_t *own = &X.words.at(s * WORDS);
          if (!letters_only(own, len_own)) continue;
          for (uint32_t q = 0; q < tile_n; q++) {
            const uint64_t key_q = staged.at(q), kq = key_class(key_q);
            if (kq < w_lo) continue;
            if (kq > w_hi) break;
            const uint32_t len_q = key_length(key_q);
            const uint32_t apart = len_q > len_own ? len_q - len_own : len_own - len_q;
            if (kq != key_class(key_own) || t + q == s || len_q == 0 || apart * C.gap > radius) continue;
            std::array<uint8_t, MAX_LEN> other;
            std::memcpy(other.data(), &X.words.at((t + q) * WORDS), MAX_LEN);
            const uint32_t dist = weighted_within(own, len_own, other.data(), len_q, C, radius);
            if (dist <= radius) hits.at(X.idx.at(s)).push_back(Hit{X.idx.at(t + q), dist});
          }
        }
      }
    }
  }
  return hits;
}

inline std::vector<std::vector<Hit>> network(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text, const Cost &C,
                                             uint32_t radius) {
  return walk(prepare(m, cls, off, text), C, radius);
}

}  // namespace cdr3wnet_host

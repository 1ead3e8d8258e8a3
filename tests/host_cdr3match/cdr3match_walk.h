// Test-only: the bipartite walk of `match` (cdr3_walk_kernel with the Bipartite side, decombinator_amd/csrc/dcrx_cdr3walk.h) step by step on the host, with the
// kernel's own look-ups (dcrx_cdr3match_core.h: block range, tile test, wave skip) and pair tests (dcrx_cdr3net_core.h): keys,
// a stable sort of (key, rank) on either side, packed strings and presence masks, then per block of 256 sorted queries the
// tiles of 256 targets, per wave of 64 lanes the skip, per lane the pair test.  Every array access is a std::vector::at().
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_cdr3match_core.h"

namespace cdr3match_host {

using namespace dcrx_cdr3match;
constexpr uint32_t WAVE = 64;

struct Side {      // one side, sorted in the walk's bucket order
  std::vector<uint64_t> key;
  std::vector<uint32_t> idx, pres;
  std::vector<uint32_t> words;      // WORDS per sorted position
};

template <bool LEV> Side prepare(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text) {
  std::vector<uint64_t> key(m);
  for (uint64_t e = 0; e < m; e++) key[e] = node_key(cls[e], off[e + 1] < off[e] ? (uint64_t)MAX_LEN + 1 : off[e + 1] - off[e]);
  Side S;
  S.idx.resize(m);
  std::iota(S.idx.begin(), S.idx.end(), 0u);
  std::stable_sort(S.idx.begin(), S.idx.end(), [&](uint32_t a, uint32_t b) { return bucket_of<LEV>(key[a]) < bucket_of<LEV>(key[b]); });
  S.key.resize(m); S.pres.resize(m); S.words.resize(m * WORDS);
  for (uint64_t s = 0; s < m; s++) {
    const uint32_t e = S.idx[s];
    S.key[s] = key[e];
    const uint64_t len = key_length(key[e]);      // (0 out of reach)
    pack(text + (key[e] == KEY_OUT_OF_REACH ? 0 : off[e]), key[e] == KEY_OUT_OF_REACH ? 0 : len, &S.words[s * WORDS]);
    S.pres[s] = presence(&S.words[s * WORDS], key[e] == KEY_OUT_OF_REACH ? 0u : (uint32_t)len);
  }
  return S;
}

// per query rank its hits (target ranks in the order the walk meets them)
template <bool LEV> std::vector<std::vector<uint32_t>> walk(const Side &Q, const Side &T, uint32_t limit) {
  const uint32_t n_q = (uint32_t)Q.key.size(), n_t = (uint32_t)T.key.size();
  std::vector<std::vector<uint32_t>> hits(n_q);
  for (uint32_t s0 = 0; s0 < n_q; s0 += QUERIES) {
    const Range R = block_range<LEV>(Q.key.data(), n_q, s0, T.key.data(), n_t);
    for (uint32_t t = R.first; t < n_t; t += TILE) {
      if (!goes_on<LEV>(R, T.key.at(t))) break;
      const uint32_t tile_n = std::min<uint32_t>(TILE, n_t - t);
      for (uint32_t w0 = s0; w0 < s0 + QUERIES; w0 += WAVE) {
        auto k_of = [&](uint32_t s) { return bucket_of<LEV>(s < n_q ? Q.key.at(s) : KEY_OUT_OF_REACH); };
        const uint64_t w_lo = k_of(w0), w_hi = k_of(w0 + WAVE - 1);
        if (wave_skips(bucket_of<LEV>(T.key.at(t)), bucket_of<LEV>(T.key.at(t + tile_n - 1)), w_lo, w_hi)) continue;
        for (uint32_t s = w0; s < std::min(w0 + WAVE, n_q); s++) {
          const uint64_t key_own = Q.key.at(s);
          if (key_own == KEY_OUT_OF_REACH) continue;
          const uint32_t len_own = key_length(key_own);
          for (uint32_t q = 0; q < tile_n; q++) {
            const uint64_t key_q = T.key.at(t + q), kq = bucket_of<LEV>(key_q);
            if (kq < w_lo) continue;
            if (kq > w_hi) break;
            if (kq != bucket_of<LEV>(key_own)) continue;
            bool hit;
            if (LEV) {
              const uint32_t len_q = key_length(key_q);
              hit = len_q + limit >= len_own && len_own + limit >= len_q && presence_allows(Q.pres.at(s), T.pres.at(t + q), limit) &&
                    lev_within(&Q.words.at(s * WORDS), len_own, &T.words.at((t + q) * WORDS), len_q, limit) <= limit;
            } else {
              hit = distance(&Q.words.at(s * WORDS), &T.words.at((t + q) * WORDS), limit) <= limit;
            }
            if (hit) hits.at(Q.idx.at(s)).push_back(T.idx.at(t + q));
          }
        }
      }
    }
  }
  return hits;
}

// the whole step: D = 0 takes the Hamming walk under either metric
inline std::vector<std::vector<uint32_t>> match(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text,
                                                uint64_t m_q, const uint32_t *q_cls, const uint64_t *q_off, const uint8_t *q_text,
                                                uint32_t limit, uint32_t metric) {
  if (metric == METRIC_LEVENSHTEIN && limit > 0)
    return walk<true>(prepare<true>(m_q, q_cls, q_off, q_text), prepare<true>(m_t, t_cls, t_off, t_text), limit);
  return walk<false>(prepare<false>(m_q, q_cls, q_off, q_text), prepare<false>(m_t, t_cls, t_off, t_text), limit);
}

}  // namespace cdr3match_host

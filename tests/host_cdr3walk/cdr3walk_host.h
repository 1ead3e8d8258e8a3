// Test-only: the tile walk (cdr3_walk_kernel<WRITE, Side, Pair, Sink>, decombinator_amd/csrc/dcrx_cdr3walk.h) step by step on
// the host, once for every side, pair test and sink.  The sides and the pair tests are the kernel's own structs
// (dcrx_cdr3pair_core.h), the look-ups dcrx_cdr3match_core.h's: nothing of them is stated again here.  Prepare: keys, a stable
// sort of (key, rank) in the pair test's bucket order, packed strings, presence masks and bucket starts.  Walk: per block of 256
// sorted nodes of Q the tiles of 256 entries of T with their keys as staged, per wave of 64 lanes the skip, per lane the pair
// test.  A lane takes its entries in order (the kernel's pending / settle scheme changes when a test runs, not which).
// Every array access is a std::vector::at(); a staged string is copied into a buffer of exactly 32 bytes.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_cdr3pair_core.h"
#include "../../decombinator_amd/csrc/dcrx_cdr3profile_core.h"

namespace cdr3walk_host {

using namespace dcrx_cdr3pair;
constexpr uint32_t WAVE = 64;

struct Sorted {      // one table, sorted in a pair test's bucket order
  std::vector<uint64_t> key;
  std::vector<uint32_t> idx, pres, bstart;      // rank, presence mask, start of the position's bucket
  std::vector<uint32_t> words;                  // WORDS per sorted position
};

template <bool CLS> Sorted prepare(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text) {
  std::vector<uint64_t> key(m);
  for (uint64_t e = 0; e < m; e++) key[e] = node_key(cls[e], off[e + 1] < off[e] ? (uint64_t)MAX_LEN + 1 : off[e + 1] - off[e]);
  Sorted S;
  S.idx.resize(m);
  std::iota(S.idx.begin(), S.idx.end(), 0u);
  std::stable_sort(S.idx.begin(), S.idx.end(), [&](uint32_t a, uint32_t b) { return bucket_of<CLS>(key[a]) < bucket_of<CLS>(key[b]); });
  S.key.resize(m); S.pres.resize(m); S.bstart.resize(m); S.words.resize(m * WORDS);
  for (uint64_t s = 0; s < m; s++) {
    const uint32_t e = S.idx[s];
    S.key[s] = key[e];
    S.bstart[s] = s && bucket_of<CLS>(S.key[s]) == bucket_of<CLS>(S.key[s - 1]) ? S.bstart[s - 1] : (uint32_t)s;
    const bool out = key[e] == KEY_OUT_OF_REACH;
    pack(text + (out ? 0 : off[e]), out ? 0 : key_length(key[e]), &S.words[s * WORDS]);
    S.pres[s] = presence(&S.words[s * WORDS], out ? 0u : key_length(key[e]));
  }
  return S;
}

// the walk's begin(): the weighted cost reads its table where the launch argument holds it
template <class Pair> typename Pair::Ctx begin(const Pair &) { return {}; }
inline Cost begin(const Weighted &pair) {
  return Cost{reinterpret_cast<const uint8_t *>(pair.cost.sub), pair.cost.gap, pair.cost.ntrim, pair.cost.ctrim};
}
inline Weighted weighted(const uint8_t *sub, uint32_t gap, uint32_t ntrim, uint32_t ctrim, uint32_t radius) {
  Weighted W{{{}, gap, ntrim, ctrim}, radius};
  std::memcpy(W.cost.sub, sub, SUB_BYTES);
  return W;
}

// ---- the two sinks.  clear(): in front of a block; add(): lane `lane`, whose node has rank e, hits the entry of rank j at
// distance d; read_out(): behind the block, for every lane that holds a node

struct Hit {
  uint32_t rank, dist;
  bool operator==(const Hit &o) const { return rank == o.rank && dist == o.dist; }
};

// per rank of Q its hits, in the order the walk meets them
struct Hits {
  std::vector<std::vector<Hit>> rows;
  explicit Hits(uint64_t m_q) : rows(m_q) {}
  void clear() {}
  void add(uint32_t, uint32_t e, uint32_t j, uint32_t d) { rows.at(e).push_back(Hit{j, d}); }
  void read_out(uint32_t, uint32_t) {}
};

// ... as the entries leave them: degree (m), off (m + 1) and, where they fit cap, the hits and (dist not null) their distances;
// returns the need
inline uint64_t flat(const Hits &H, uint32_t *degree, uint64_t *off, uint32_t *hit, uint32_t *dist, uint64_t cap) {
  uint64_t at = 0;
  for (size_t i = 0; i < H.rows.size(); i++) {
    degree[i] = (uint32_t)H.rows[i].size();
    off[i] = at;
    for (const Hit &h : H.rows[i]) {
      if (at < cap) {
        hit[at] = h.rank;
        if (dist) dist[at] = h.dist;
      }
      at++;
    }
  }
  off[H.rows.size()] = at;
  return at;
}

// the Profile sink: a block's counters are ONE array of bins * 256 cells, cell b * 256 + lane, zeroed per block, one added
// per hit at bin_of(d, step), and read out per lane into the row of its rank
struct Histogram {
  uint32_t step, bins;
  std::vector<uint32_t> row, hist;
  Histogram(uint64_t m_q, uint32_t step, uint32_t bins) : step(step), bins(bins), row(m_q * bins, 0xA5A5A5A5u) {}      // (what the read-out does not write stays visible)
  void clear() { hist.assign((size_t)bins * QUERIES, 0u); }
  void add(uint32_t lane, uint32_t, uint32_t, uint32_t d) { hist.at((size_t)dcrx_cdr3profile::bin_of(d, step) * QUERIES + lane) += 1; }
  void read_out(uint32_t lane, uint32_t e) {
    for (uint32_t b = 0; b < bins; b++) row.at((size_t)e * bins + b) = hist.at((size_t)b * QUERIES + lane);
  }
};

// Q: the blocks' nodes, T: the entries they walk, both sorted in Pair's bucket order (Within: one table, given twice)
template <class Side, class Pair, class Sink> void walk(const Sorted &Q, const Sorted &T, const Side &side, const Pair &pair, Sink &sink) {
  constexpr bool CLS = Pair::CLS;
  const typename Pair::Ctx ctx = begin(pair);
  const uint32_t n_q = (uint32_t)Q.key.size(), n_t = (uint32_t)T.key.size();
  for (uint32_t s0 = 0; s0 < n_q; s0 += QUERIES) {
    sink.clear();
    const Range R = side.template range<CLS>(Q.key.data(), n_q, T.key.data(), n_t, s0);
    for (uint32_t t = R.first; t < n_t; t += TILE) {
      if (!goes_on<CLS>(R, T.key.at(t))) break;
      const uint32_t tile_n = std::min<uint32_t>(TILE, n_t - t);
      std::vector<uint64_t> staged(tile_n);      // the keys as staged
      for (uint32_t q = 0; q < tile_n; q++) staged.at(q) = pair.staged(&T.words.at((t + q) * WORDS), T.key.at(t + q));
      for (uint32_t w0 = s0; w0 < s0 + QUERIES; w0 += WAVE) {
        auto k_of = [&](uint32_t s) { return bucket_of<CLS>(s < n_q ? Q.key.at(s) : KEY_OUT_OF_REACH); };
        const uint64_t w_lo = k_of(w0), w_hi = k_of(w0 + WAVE - 1);
        if (wave_skips(bucket_of<CLS>(staged.at(0)), bucket_of<CLS>(staged.at(tile_n - 1)), w_lo, w_hi)) continue;
        for (uint32_t s = w0; s < std::min(w0 + WAVE, n_q); s++) {
          const uint64_t key_own = Q.key.at(s);
          if (key_own == KEY_OUT_OF_REACH) continue;
          const uint32_t len_own = key_length(key_own), pres_own = Pair::MASKS ? Q.pres.at(s) : 0u;
          const uint32_t *own = &Q.words.at(s * WORDS);
          if (!pair.admits(own, len_own)) continue;
          for (uint32_t q = 0; q < tile_n; q++) {
            const uint64_t key_q = staged.at(q), kq = bucket_of<CLS>(key_q);
            if (kq < w_lo) continue;
            if (kq > w_hi) break;
            const uint32_t len_q = key_length(key_q);
            if (kq != bucket_of<CLS>(key_own) || side.self(t + q, s) ||
                !pair.window(ctx, len_own, pres_own, len_q, Pair::MASKS ? T.pres.at(t + q) : 0u))
              continue;
            std::array<uint32_t, WORDS> other;
            std::memcpy(other.data(), &T.words.at((t + q) * WORDS), MAX_LEN);
            const uint32_t d = pair.test(ctx, own, len_own, other.data(), len_q);
            if (d <= pair.bound()) sink.add(s - s0, Q.idx.at(s), T.idx.at(t + q), d);
          }
        }
      }
    }
    for (uint32_t s = s0; s < std::min(s0 + QUERIES, n_q); s++) sink.read_out(s - s0, Q.idx.at(s));
  }
}

// ---- the whole steps, as the entries route them

// `match` and the network under the two plain metrics: D = 0 takes the Hamming walk under either
template <class Pair> Hits plain_walk(const Sorted &Q, const Sorted &T, bool within, uint32_t limit) {
  Hits H(Q.key.size());
  if (within) walk(Q, Q, Within{Q.bstart.data()}, Pair{limit}, H);
  else walk(Q, T, Bipartite{}, Pair{limit}, H);
  return H;
}
inline Hits match(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q, const uint32_t *q_cls,
                  const uint64_t *q_off, const uint8_t *q_text, uint32_t limit, uint32_t metric) {
  if (metric == METRIC_LEVENSHTEIN && limit > 0)
    return plain_walk<Levenshtein>(prepare<true>(m_q, q_cls, q_off, q_text), prepare<true>(m_t, t_cls, t_off, t_text), false, limit);
  return plain_walk<Hamming>(prepare<false>(m_q, q_cls, q_off, q_text), prepare<false>(m_t, t_cls, t_off, t_text), false, limit);
}
inline Hits network(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text, uint32_t limit, uint32_t metric) {
  if (metric == METRIC_LEVENSHTEIN && limit > 0) return plain_walk<Levenshtein>(prepare<true>(m, cls, off, text), Sorted{}, true, limit);
  return plain_walk<Hamming>(prepare<false>(m, cls, off, text), Sorted{}, true, limit);
}

// ... under the weighted metric
inline Hits match(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q, const uint32_t *q_cls,
                  const uint64_t *q_off, const uint8_t *q_text, const Weighted &pair) {
  Hits H(m_q);
  walk(prepare<true>(m_q, q_cls, q_off, q_text), prepare<true>(m_t, t_cls, t_off, t_text), Bipartite{}, pair, H);
  return H;
}
inline Hits network(uint64_t m, const uint32_t *cls, const uint64_t *off, const uint8_t *text, const Weighted &pair) {
  const Sorted X = prepare<true>(m, cls, off, text);
  Hits H(m);
  walk(X, X, Within{X.bstart.data()}, pair, H);
  return H;
}

// profile[m_q * bins] of a ladder that stands (refuse_ladder), at radius step * (bins - 1); every cell is written
inline std::vector<uint32_t> profile(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q,
                                     const uint32_t *q_cls, const uint64_t *q_off, const uint8_t *q_text, Weighted pair, uint32_t step,
                                     uint32_t bins) {
  pair.radius = step * (bins - 1);
  Histogram H(m_q, step, bins);
  walk(prepare<true>(m_q, q_cls, q_off, q_text), prepare<true>(m_t, t_cls, t_off, t_text), Bipartite{}, pair, H);
  return H.row;
}

}  // namespace cdr3walk_host

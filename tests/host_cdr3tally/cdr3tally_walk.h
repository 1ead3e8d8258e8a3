// Test-only: the tally's walk (cdr3_walk_kernel<false, Bipartite, WeightedPer, Tally>, decombinator_amd/csrc/dcrx_cdr3walk.h) step
// by step on the host.  prepare() and the structs are the one host walk's (../host_cdr3walk/cdr3walk_host.h); the walk loop
// stands here because every staged entry carries a bound of its own: staged beside its key (bound_of by the entry's rank), it
// decides the key (an entry without a radius gets length 0), the window and the pair test, all through WeightedPer itself
// (dcrx_cdr3pair_core.h).  The sink is done as the kernel does it: a count and a weight per staged entry of the tile, zeroed in
// front of the block, flushed — the non-zero cells only — at the top of the next tile and once behind the walk onto
// accumulators indexed by SORTED POSITION, then scattered by rank.  Every array access is a std::vector::at().
#pragma once
#include "../host_cdr3walk/cdr3walk_host.h"

namespace cdr3tally_host {

using namespace cdr3walk_host;

inline WeightedPer weighted_per(const uint8_t *sub, uint32_t gap, uint32_t ntrim, uint32_t ctrim, const uint32_t *radius) {
  WeightedPer W{{{}, gap, ntrim, ctrim}, radius};
  std::memcpy(W.cost.sub, sub, SUB_BYTES);
  return W;
}

struct Totals {
  std::vector<uint32_t> t_count, q_degree;
  std::vector<uint64_t> t_weight;
  uint64_t flushes = 0;      // the (block, staged entry) pairs that reached the accumulators
};

inline Totals tally(uint64_t m_t, const uint32_t *t_cls, const uint64_t *t_off, const uint8_t *t_text, uint64_t m_q, const uint32_t *q_cls,
                    const uint64_t *q_off, const uint8_t *q_text, const uint64_t *weight, const WeightedPer &pair) {
  const Sorted Q = prepare<true>(m_q, q_cls, q_off, q_text), T = prepare<true>(m_t, t_cls, t_off, t_text);
  const Cost ctx{reinterpret_cast<const uint8_t *>(pair.cost.sub), pair.cost.gap, pair.cost.ntrim, pair.cost.ctrim};
  const uint32_t n_q = (uint32_t)m_q, n_t = (uint32_t)m_t;
  Totals out;
  out.t_count.assign(m_t, 0xA5A5A5A5u);      // (what the scatter and the lanes do not write stays visible)
  out.t_weight.assign(m_t, 0xA5A5A5A5A5A5A5A5ull);
  out.q_degree.assign(m_q, 0xA5A5A5A5u);
  if (!m_q || !m_t) {      // the entries: nothing can hit, every cell is zero
    std::fill(out.t_count.begin(), out.t_count.end(), 0u);
    std::fill(out.t_weight.begin(), out.t_weight.end(), 0ull);
    std::fill(out.q_degree.begin(), out.q_degree.end(), 0u);
    return out;
  }
  std::vector<uint32_t> acc_count(m_t, 0u);      // by sorted position, zeroed in front of the walk
  std::vector<uint64_t> acc_weight(m_t, 0ull);
  const Bipartite side;
  for (uint32_t s0 = 0; s0 < n_q; s0 += QUERIES) {
    std::vector<uint32_t> lds_c(TILE, 0u), count(QUERIES, 0u);
    std::vector<uint64_t> lds_w(TILE, 0ull);
    uint32_t flush_at = 0;
    auto flush = [&]() {
      for (uint32_t k = 0; k < TILE; k++) {
        if (!lds_c.at(k)) continue;
        acc_count.at(flush_at + k) += lds_c.at(k);
        acc_weight.at(flush_at + k) += lds_w.at(k);
        lds_c.at(k) = 0;
        lds_w.at(k) = 0;
        out.flushes++;
      }
    };
    const Range R = side.range<true>(Q.key.data(), n_q, T.key.data(), n_t, s0);
    for (uint32_t t = R.first; t < n_t; t += TILE) {
      if (!goes_on<true>(R, T.key.at(t))) break;
      flush();
      flush_at = t;
      const uint32_t tile_n = std::min<uint32_t>(TILE, n_t - t);
      std::vector<uint64_t> staged(tile_n);
      std::vector<uint32_t> lds_b(tile_n);
      for (uint32_t q = 0; q < tile_n; q++) {
        lds_b.at(q) = pair.bound_of(T.idx.at(t + q));
        staged.at(q) = pair.staged(&T.words.at((t + q) * WORDS), T.key.at(t + q), lds_b.at(q));
      }
      for (uint32_t w0 = s0; w0 < s0 + QUERIES; w0 += WAVE) {
        auto k_of = [&](uint32_t s) { return bucket_of<true>(s < n_q ? Q.key.at(s) : KEY_OUT_OF_REACH); };
        const uint64_t w_lo = k_of(w0), w_hi = k_of(w0 + WAVE - 1);
        if (wave_skips(bucket_of<true>(staged.at(0)), bucket_of<true>(staged.at(tile_n - 1)), w_lo, w_hi)) continue;
        for (uint32_t s = w0; s < std::min(w0 + WAVE, n_q); s++) {
          const uint64_t key_own = Q.key.at(s);
          if (key_own == KEY_OUT_OF_REACH) continue;
          const uint32_t len_own = key_length(key_own);
          const uint32_t *own = &Q.words.at(s * WORDS);
          if (!pair.admits(own, len_own)) continue;
          for (uint32_t q = 0; q < tile_n; q++) {
            const uint64_t key_q = staged.at(q), kq = bucket_of<true>(key_q);
            if (kq < w_lo) continue;
            if (kq > w_hi) break;
            const uint32_t len_q = key_length(key_q), bound = lds_b.at(q);
            if (kq != bucket_of<true>(key_own) || !pair.window(ctx, len_own, 0u, len_q, 0u, bound)) continue;
            std::array<uint32_t, WORDS> other;
            std::memcpy(other.data(), &T.words.at((t + q) * WORDS), MAX_LEN);
            if (pair.test(ctx, own, len_own, other.data(), len_q, bound) <= bound) {
              lds_c.at(q) += 1;
              lds_w.at(q) += weight[Q.idx.at(s)];
              count.at(s - s0) += 1;
            }
          }
        }
      }
    }
    flush();
    for (uint32_t s = s0; s < std::min(s0 + QUERIES, n_q); s++) out.q_degree.at(Q.idx.at(s)) = count.at(s - s0);
  }
  for (uint32_t p = 0; p < n_t; p++) {      // the scatter: every target's two cells, by rank
    out.t_count.at(T.idx.at(p)) = acc_count.at(p);
    out.t_weight.at(T.idx.at(p)) = acc_weight.at(p);
  }
  return out;
}

}  // namespace cdr3tally_host

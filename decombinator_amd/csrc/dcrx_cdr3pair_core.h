// dcrx_cdr3pair_core.h — the policies of the tile walk (dcrx_cdr3walk.h: cdr3_walk_kernel<WRITE, Side, Pair, Sink>), shared by
// the kernel and a plain host build (tests/host_cdr3walk: the one host walk calls these structs themselves): the two sides,
// Bipartite and Within, and the pair tests, Hamming, Levenshtein, Weighted and WeightedPer (a bound per entry), with the weighted
// walk's launch argument.
// What needs the device stays in dcrx_cdr3walk.h: begin(), which for Weighted stages the cost table in LDS.
// The look-ups are dcrx_cdr3match_core.h's, the per-pair distances dcrx_cdr3net_core.h's and dcrx_cdr3w_core.h's.
#pragma once
#include <stdint.h>

#include "dcrx_cdr3match_core.h"
#include "dcrx_cdr3w_core.h"

namespace dcrx_cdr3pair {

using namespace dcrx_cdr3match;
using namespace dcrx_cdr3w;

// ---- the two sides: range() is the same for every lane of a block (s0: its first node; the sorted keys of Q and of T)

// Q's nodes against another table's entries
struct Bipartite {
  template <bool CLS>
  DCRX_CDR3NET_HD Range range(const uint64_t *q_key, uint32_t n_q, const uint64_t *t_key, uint32_t n_t, uint32_t s0) const {
    return block_range<CLS>(q_key, n_q, s0, t_key, n_t);
  }
  DCRX_CDR3NET_HD bool self(uint32_t, uint32_t) const { return false; }
};

// a table against itself (Q and T are one): from the block's first node's bucket start, and a node is no neighbour of its own
struct Within {
  const uint32_t *bstart;
  template <bool CLS>
  DCRX_CDR3NET_HD Range range(const uint64_t *q_key, uint32_t n_q, const uint64_t *, uint32_t, uint32_t s0) const {
    return within_range<CLS>(q_key, n_q, s0, bstart);
  }
  DCRX_CDR3NET_HD bool self(uint32_t p, uint32_t s) const { return p == s; }
};

// ---- the pair tests.  CLS: the bucket is the class alone (else class and length).  MASKS: the presence masks are
// staged and handed to window().  DEFER: an entry that passes window() waits, and test() runs on it later (see the walk).
// DIST: test()'s value is stored beside the hit.  PER: every entry has a bound of its own, staged beside its key (bound_of(),
// by the entry's rank) and handed to staged(), window() and test(), which then read no member; there is no bound().  Ctx is
// what the walk's begin() returns once per lane in front of the walk and hands back to window() and test(); admits(): whether
// the lane's own node takes part at all; staged(): the key a staged entry gets (its eight words in hand); window(): the cheap
// tests of a pair of one bucket; test(): the distance, a hit when <= bound() (PER: <= the entry's bound).

struct Hamming {
  static constexpr bool CLS = false, MASKS = false, DEFER = false, DIST = false, PER = false;
  uint32_t limit;
  struct Ctx {};
  DCRX_CDR3NET_HD bool admits(const uint32_t *, uint32_t) const { return true; }
  DCRX_CDR3NET_HD uint64_t staged(const uint32_t *, uint64_t key) const { return key; }
  DCRX_CDR3NET_HD bool window(const Ctx &, uint32_t, uint32_t, uint32_t, uint32_t) const { return true; }      // (one bucket: one length)
  DCRX_CDR3NET_HD uint32_t test(const Ctx &, const uint32_t *own, uint32_t, const uint32_t *other, uint32_t) const {
    return distance(own, other, limit);
  }
  DCRX_CDR3NET_HD uint32_t bound() const { return limit; }
};

struct Levenshtein {
  static constexpr bool CLS = true, MASKS = true, DEFER = true, DIST = false, PER = false;
  uint32_t limit;
  struct Ctx {};
  DCRX_CDR3NET_HD bool admits(const uint32_t *, uint32_t) const { return true; }
  DCRX_CDR3NET_HD uint64_t staged(const uint32_t *, uint64_t key) const { return key; }
  DCRX_CDR3NET_HD bool window(const Ctx &, uint32_t len_own, uint32_t pres_own, uint32_t len, uint32_t pres) const {
    return len + limit >= len_own && len_own + limit >= len && presence_allows(pres_own, pres, limit);
  }
  DCRX_CDR3NET_HD uint32_t test(const Ctx &, const uint32_t *own, uint32_t len_own, const uint32_t *other, uint32_t len) const {
    return lev_within(own, len_own, other, len, limit);
  }
  DCRX_CDR3NET_HD uint32_t bound() const { return limit; }
};

// the cost as the weighted walk's launch argument: the table as the 256 dwords the block's lanes copy into LDS, one each
struct CostArg {
  uint32_t sub[SUB_BYTES / 4];
  uint32_t gap, ntrim, ctrim;
};
static_assert(SUB_BYTES / 4 == QUERIES, "a lane stages one dword of the cost table");

// The class, the length window |la - lb| * gap <= radius, then weighted_within.  A string with a non-letter takes part in
// nothing: such a node is not admitted, and the lane that stages such an entry stages a key of length 0, which no lane tests.
// The presence masks are not read (a substitution may cost nothing).  A pair is tested where it is met: at such radii most
// pairs of a class pass the window, so there is nothing for the pending / settle scheme to collect.
struct Weighted {
  static constexpr bool CLS = true, MASKS = false, DEFER = false, DIST = true, PER = false;
  CostArg cost;
  uint32_t radius;
  using Ctx = Cost;      // (its table: wherever begin() has put cost.sub)
  DCRX_CDR3NET_HD bool admits(const uint32_t *own, uint32_t len_own) const { return letters_only(own, len_own); }
  DCRX_CDR3NET_HD uint64_t staged(const uint32_t *w, uint64_t key) const {
    return letters_only(w, key_length(key)) ? key : key & ~LEN_MASK;      // (the class stays: the tile stays sorted)
  }
  DCRX_CDR3NET_HD bool window(const Cost &C, uint32_t len_own, uint32_t, uint32_t len, uint32_t) const {
    const uint32_t apart = len > len_own ? len - len_own : len_own - len;
    return len != 0 && apart * C.gap <= radius;      // (0: an entry with a non-letter, or out of reach)
  }
  DCRX_CDR3NET_HD uint32_t test(const Cost &C, const uint32_t *own, uint32_t len_own, const uint32_t *other, uint32_t len) const {
    return weighted_within(own, len_own, reinterpret_cast<const uint8_t *>(other), len, C, radius);
  }
  DCRX_CDR3NET_HD uint32_t bound() const { return radius; }
};

// Weighted with a radius per entry (include/dcrx.h "tally, weighted"): radius[rank] is 0 .. 65535, and anything above — NO_RADIUS
// is the one the contract names — means that the entry takes part in nothing: it is staged as an entry with a non-letter is,
// with a key of length 0.  The window and weighted_within, early exits and all, run at the entry's own bound.
constexpr uint32_t NO_RADIUS = 0xFFFFFFFFu;
struct WeightedPer {
  static constexpr bool CLS = true, MASKS = false, DEFER = false, DIST = true, PER = true;
  CostArg cost;
  const uint32_t *radius;      // by rank
  using Ctx = Cost;
  DCRX_CDR3NET_HD bool admits(const uint32_t *own, uint32_t len_own) const { return letters_only(own, len_own); }
  DCRX_CDR3NET_HD uint32_t bound_of(uint32_t rank) const {
    const uint32_t r = radius[rank];
    return r > MAX_RADIUS ? NO_RADIUS : r;
  }
  DCRX_CDR3NET_HD uint64_t staged(const uint32_t *w, uint64_t key, uint32_t bound) const {
    return bound != NO_RADIUS && letters_only(w, key_length(key)) ? key : key & ~LEN_MASK;
  }
  DCRX_CDR3NET_HD bool window(const Cost &C, uint32_t len_own, uint32_t, uint32_t len, uint32_t, uint32_t bound) const {
    const uint32_t apart = len > len_own ? len - len_own : len_own - len;
    return len != 0 && apart * C.gap <= bound;      // (0: an entry without a radius, with a non-letter, or out of reach)
  }
  DCRX_CDR3NET_HD uint32_t test(const Cost &C, const uint32_t *own, uint32_t len_own, const uint32_t *other, uint32_t len, uint32_t bound) const {
    return weighted_within(own, len_own, reinterpret_cast<const uint8_t *>(other), len, C, bound);
  }
};

// what the host entry refuses of the m_t radii, as a message; null: they stand
inline const char *refuse_radii(const uint32_t *radius, uint64_t m_t) {
  for (uint64_t j = 0; j < m_t; j++)
    if (radius[j] > MAX_RADIUS && radius[j] != NO_RADIUS) return "a radius is 0 .. 65535 or DCRX_CDR3_NO_RADIUS";
  return nullptr;
}

}  // namespace dcrx_cdr3pair

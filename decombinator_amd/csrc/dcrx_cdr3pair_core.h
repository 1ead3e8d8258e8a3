// dcrx_cdr3pair_core.h — the policies of the tile walk (dcrx_cdr3walk.h: cdr3_walk_kernel<WRITE, Side, Pair, Sink>), shared by
// the kernel and a plain host build (tests/host_cdr3walk: the one host walk calls these structs themselves): the two sides,
// Bipartite and Within, and the three pair tests, Hamming, Levenshtein and Weighted, with the weighted walk's launch argument.
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

// ---- the three pair tests.  CLS: the bucket is the class alone (else class and length).  MASKS: the presence masks are
// staged and handed to window().  DEFER: an entry that passes window() waits, and test() runs on it later (see the walk).
// DIST: test()'s value is stored beside the hit.  Ctx is what the walk's begin() returns once per lane in front of the walk
// and hands back to window() and test(); admits(): whether the lane's own node takes part at all; staged(): the key a staged
// entry gets (its eight words in hand); window(): the cheap tests of a pair of one bucket; test(): the distance, a hit when
// <= bound().

struct Hamming {
  static constexpr bool CLS = false, MASKS = false, DEFER = false, DIST = false;
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
  static constexpr bool CLS = true, MASKS = true, DEFER = true, DIST = false;
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
  static constexpr bool CLS = true, MASKS = false, DEFER = false, DIST = true;
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

}  // namespace dcrx_cdr3pair

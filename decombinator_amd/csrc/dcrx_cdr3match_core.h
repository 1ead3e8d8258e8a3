// dcrx_cdr3match_core.h — the look-ups of the tile walk (dcrx_cdr3walk.h: `match` and the CDR3 network), shared by the kernel
// and a plain host build (tests/host_cdr3walk, the one host walk): a bucket of a key under either metric, where a block of sorted queries starts
// in the sorted targets (the index's, or under the network its own table) and at which bucket it stops, whether the walk goes
// on to a tile, and whether a wave skips one.
// The per-node and per-pair code (keys, packed strings, Hamming and edit-distance tests) is dcrx_cdr3net_core.h's; the sides
// and pair tests that call both are dcrx_cdr3pair_core.h's.
#pragma once
#include <stdint.h>

#include "dcrx_cdr3net_core.h"

namespace dcrx_cdr3match {

using namespace dcrx_cdr3net;

constexpr uint32_t QUERIES = 256;      // sorted queries of one block (a lane each)
constexpr uint32_t TILE = 256;         // staged targets per step

// the key a bucket is made of: the whole key (class, length), or under the Levenshtein walk its class (and out-of-reach) bits
template <bool LEV> DCRX_CDR3NET_HD uint64_t bucket_of(uint64_t key) { return LEV ? key_class(key) : key; }

// the largest bucket a node in reach can have
template <bool LEV> DCRX_CDR3NET_HD uint64_t last_bucket() { return bucket_of<LEV>(KEY_OUT_OF_REACH) - 1; }

// The first of n sorted keys whose bucket is >= k (n: none is).  A plain binary search: at most 31 steps below 2^30 keys.
template <bool LEV> DCRX_CDR3NET_HD uint32_t first_at_or_above(const uint64_t *key, uint32_t n, uint64_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bucket_of<LEV>(key[mid]) < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// What the block of sorted queries s0 .. min(s0 + QUERIES, n_q) - 1 walks: the targets from `first` on, tile by tile, while
// goes_on() holds of the tile's first key.  A block of queries out of reach alone walks nothing (its first bucket lies
// behind `stop`).
struct Range {
  uint32_t first;      // the first target at or above the block's first query's bucket
  uint64_t stop;       // the block's last query's bucket, or the last bucket in reach if that is smaller
};
template <bool LEV> DCRX_CDR3NET_HD uint64_t block_stop(const uint64_t *q_key, uint32_t n_q, uint32_t s0) {
  const uint32_t last = (n_q - s0 < QUERIES ? n_q : s0 + QUERIES) - 1;
  const uint64_t k_last = bucket_of<LEV>(q_key[last]);
  return k_last < last_bucket<LEV>() ? k_last : last_bucket<LEV>();
}
// two tables (`match`): the first target comes from a binary search over the index's sorted keys
template <bool LEV> DCRX_CDR3NET_HD Range block_range(const uint64_t *q_key, uint32_t n_q, uint32_t s0, const uint64_t *t_key, uint32_t n_t) {
  Range r;
  r.stop = block_stop<LEV>(q_key, n_q, s0);
  r.first = first_at_or_above<LEV>(t_key, n_t, bucket_of<LEV>(q_key[s0]));
  return r;
}
// one table walked against itself (the network): bstart[s] is the start of sorted position s's bucket (the gather's run
// marks, max-scanned), so the first entry is read, not searched
template <bool LEV> DCRX_CDR3NET_HD Range within_range(const uint64_t *key, uint32_t n, uint32_t s0, const uint32_t *bstart) {
  Range r;
  r.stop = block_stop<LEV>(key, n, s0);
  r.first = bstart[s0];
  return r;
}
template <bool LEV> DCRX_CDR3NET_HD bool goes_on(const Range &r, uint64_t tile_first_key) { return bucket_of<LEV>(tile_first_key) <= r.stop; }

// a wave whose queries' buckets are w_lo .. w_hi skips a tile whose targets' buckets are tile_lo .. tile_hi when they miss
DCRX_CDR3NET_HD bool wave_skips(uint64_t tile_lo, uint64_t tile_hi, uint64_t w_lo, uint64_t w_hi) { return tile_hi < w_lo || tile_lo > w_hi; }

}  // namespace dcrx_cdr3match

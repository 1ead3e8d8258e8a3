// dcrx_cdr3net_core.h — the per-node and per-pair code of the CDR3 network (`--cdr3-network`, dcrx_cdr3net.hip), shared by
// the kernels and a plain host build (tests/host_cdr3net).
//
// Per node (class, string): whether it is in reach (1 .. MAX_LEN bytes), the bucket key (class, length) — a node out of reach
// is keyed behind every bucket —, and the string as eight dwords (byte p in bits [8(p % 4), 8(p % 4) + 7] of word p / 4, zero
// beyond the length; the bytes as they are: nothing is folded or decoded).
// Per pair: the Hamming distance of two packed strings of one length, given up once it has passed the limit; and for the
// Levenshtein metric (second half of the file) a letter-presence filter and lev_within, the exact edit distance up to the
// limit of two packed strings whose lengths may differ (also built into tests/host_cdr3lev).
#pragma once
#include <stdint.h>

#include "../../include/dcrx.h"

#if defined(__HIPCC__)
#define DCRX_CDR3NET_HD __host__ __device__ __forceinline__
#else
#define DCRX_CDR3NET_HD inline
#endif

namespace dcrx_cdr3net {

constexpr uint32_t MAX_LEN = DCRX_CDR3NET_MAX_LEN;
constexpr uint32_t WORDS = MAX_LEN / 4;                       // dwords of one string
constexpr uint32_t LEN_BITS = 6;                              // 1 .. 32
constexpr uint64_t KEY_OUT_OF_REACH = 1ull << (32 + LEN_BITS);      // sorts behind every bucket of nodes in reach
constexpr uint32_t KEY_BITS = 32 + LEN_BITS + 1;
static_assert(MAX_LEN == 32 && WORDS == 8, "a string is two uint4");

DCRX_CDR3NET_HD bool in_reach(uint64_t len) { return len >= 1 && len <= MAX_LEN; }

DCRX_CDR3NET_HD uint64_t bucket_key(uint32_t cls, uint32_t len) { return ((uint64_t)cls << LEN_BITS) | (uint64_t)len; }

DCRX_CDR3NET_HD uint64_t node_key(uint32_t cls, uint64_t len) { return in_reach(len) ? bucket_key(cls, (uint32_t)len) : KEY_OUT_OF_REACH; }

// The string into out[WORDS]; a node out of reach gets zero words.
DCRX_CDR3NET_HD void pack(const uint8_t *s, uint64_t len, uint32_t *out) {
  for (uint32_t w = 0; w < WORDS; w++) out[w] = 0;
  if (!in_reach(len)) return;
  for (uint32_t p = 0; p < (uint32_t)len; p++) out[p / 4] |= (uint32_t)s[p] << (8 * (p % 4));
}

DCRX_CDR3NET_HD uint32_t popcount32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

// bytes at which two words differ: bit 7 of every non-zero byte of a ^ b, counted
DCRX_CDR3NET_HD uint32_t word_mismatches(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  return popcount32((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

// Hamming distance of two packed strings of one length when it is <= limit, else some value > limit (given up after the
// first half — 16 bytes, which holds most CDR3s whole — once that alone has passed the limit).
DCRX_CDR3NET_HD uint32_t distance(const uint32_t *a, const uint32_t *b, uint32_t limit) {
  uint32_t d = 0;
  for (uint32_t w = 0; w < WORDS / 2; w++) d += word_mismatches(a[w], b[w]);
  if (d > limit) return d;
  for (uint32_t w = WORDS / 2; w < WORDS; w++) d += word_mismatches(a[w], b[w]);
  return d;
}

// ---- the Levenshtein metric (`--cdr3-metric levenshtein`): the bucket is the class alone ----
//
// The key stays (class, length): the sort then runs over the class bits and the out-of-reach bit only (from bit LEN_BITS
// up), so a class stays in rank order and the sorted keys still carry every node's length in their low bits.

constexpr uint32_t METRIC_HAMMING = DCRX_CDR3NET_HAMMING, METRIC_LEVENSHTEIN = DCRX_CDR3NET_LEVENSHTEIN;

DCRX_CDR3NET_HD uint64_t key_class(uint64_t key) { return key >> LEN_BITS; }      // (out of reach: 2^32, behind every class)
DCRX_CDR3NET_HD uint32_t key_length(uint64_t key) { return (uint32_t)key & ((1u << LEN_BITS) - 1u); }

#if defined(__HIPCC__)
#define DCRX_CDR3NET_UNROLL _Pragma("unroll")
#else
#define DCRX_CDR3NET_UNROLL
#endif

// Which letters a packed string of `len` bytes holds: bit (byte & 31).  One substitution moves at most two of these bits
// and one insertion or deletion at most one, so two strings within D edits differ in at most 2 D of them: a filter in
// front of lev_within, nothing more (DCRX_CDR3NET_NO_PRESENCE compiles it out; the result is the same without it).
DCRX_CDR3NET_HD uint32_t presence(const uint32_t *w, uint32_t len) {
  uint32_t seen = 0;
  DCRX_CDR3NET_UNROLL
  for (uint32_t p = 0; p < MAX_LEN; p++) seen |= p < len ? 1u << ((w[p / 4] >> (8 * (p % 4))) & 31u) : 0u;
  return seen;
}

DCRX_CDR3NET_HD bool presence_allows(uint32_t pa, uint32_t pb, uint32_t limit) {
#if defined(DCRX_CDR3NET_NO_PRESENCE)
  (void)pa; (void)pb; (void)limit;
  return true;
#else
  return popcount32(pa ^ pb) <= 2u * limit;
#endif
}

// the low n bits, n in 0 .. 32 (below 0 counts as 0, above 32 as 32)
DCRX_CDR3NET_HD uint32_t low_bits(int32_t n) { return n <= 0 ? 0u : n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

// ({hi, lo} >> 8 k) & 0xFFFFFFFF, k in 1 .. 3
DCRX_CDR3NET_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, k);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * k));
#endif
}

// Diagonal K of the pair: bit i is set where byte i of a DIFFERS from byte i + K of b (b shifted by K bytes across
// neighbouring words, zero beyond both ends; the non-zero bytes of the XOR flagged as word_mismatches does, the four flags of
// a word folded to four bits).  What lies outside either string is masked by the caller.
template <int K> DCRX_CDR3NET_HD uint32_t diagonal_differs(const uint32_t *a, const uint32_t *b) {
  static_assert(K >= -3 && K <= 3, "a shift stays inside the neighbouring word");
  uint32_t differs = 0;
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) {
    uint32_t shifted;
    if (K == 0) shifted = b[w];
    else if (K > 0) shifted = align_bytes(w + 1 < WORDS ? b[w + 1] : 0u, b[w], (uint32_t)K);
    else shifted = align_bytes(b[w], w ? b[w - 1] : 0u, (uint32_t)(4 + K));
    const uint32_t x = a[w] ^ shifted;
    const uint32_t t = ((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u) >> 7;      // bits 0, 8, 16, 24
    differs |= ((t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xFu) << (4 * w);
  }
  return differs;
}

// Diagonal K's match mask: bit i is set iff a[i] == b[i + K] with 0 <= i < la and 0 <= i + K < lb — a real 0x00 byte never
// matches padding, because padding lies outside the mask.
template <int K> DCRX_CDR3NET_HD uint32_t diagonal_matches(const uint32_t *a, int32_t la, const uint32_t *b, int32_t lb) {
  const int32_t end = la < lb - K ? la : lb - K;
  return ~diagonal_differs<K>(a, b) & low_bits(end) & ~low_bits(-K);
}

// from row i (0 .. 32) along a diagonal's matches as far as they go
DCRX_CDR3NET_HD int32_t extend(int32_t i, uint32_t matches) {
  const uint32_t rest = i < 32 ? matches >> i : 0u;
  const uint64_t stop = ~(uint64_t)rest;      // (the high half is all ones: the count ends at 32)
#if defined(__HIP_DEVICE_COMPILE__)
  return i + (int32_t)__ffsll((unsigned long long)stop) - 1;
#else
  return i + (int32_t)__builtin_ctzll(stop);
#endif
}

DCRX_CDR3NET_HD int32_t row_cap(int32_t i, int32_t cap) { return i < cap ? (i < 0 ? 0 : i) : (cap < 0 ? 0 : cap); }

// The Levenshtein distance (substitution, insertion and deletion cost 1 each) of two packed strings of la and lb bytes when it
// is <= D, else D + 1.  Furthest-reaching rows on the diagonals (Landau-Vishkin): f_e[k] is the furthest row i of a that e
// edits reach on diagonal k (byte i of a against byte i + k of b),
//   f_0[0] = extend(0, 0),  f_e[k] = extend(min(max(f_{e-1}[k] + 1, f_{e-1}[k-1], f_{e-1}[k+1] + 1), la, lb - k), k),
// and the answer is the first e with f_e[lb - la] >= la.  The distance is symmetric, so the shorter string is taken for a
// (a select per word, no branch): lb - la is then 0 .. D, only the diagonals between 0 and lb - la and those that can still
// come back to lb - la are ever read, and of step D only diagonal lb - la itself: at D = 1 diagonals 0 and 1, at D = 2
// diagonals -1 (for lb == la), 0, 1 and 2 (for lb == la + 2).  Every index into the words is static once the loops are
// unrolled: nothing goes to scratch; no LDS; the branches depend on the pair alone.
template <int D> DCRX_CDR3NET_HD uint32_t lev_within_d(const uint32_t *a_in, uint32_t la_in, const uint32_t *b_in, uint32_t lb_in) {
  static_assert(D == 1 || D == 2, "the distance is 1 or 2");
  const bool swap = la_in > lb_in;
  uint32_t a[WORDS], b[WORDS];
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) {
    a[w] = swap ? b_in[w] : a_in[w];
    b[w] = swap ? a_in[w] : b_in[w];
  }
  const int32_t la = (int32_t)(swap ? lb_in : la_in), lb = (int32_t)(swap ? la_in : lb_in);
  const int32_t delta = lb - la;
  if (delta > D) return D + 1;
  const uint32_t m0 = diagonal_matches<0>(a, la, b, lb);
  const int32_t f0 = extend(0, m0);
  if (delta == 0 && f0 >= la) return 0;
  if (D == 1) {
    // step 1 on diagonal delta alone: a substitution (delta 0) or an insertion into a (delta 1)
    uint32_t m = m0;
    if (delta == 1) m = diagonal_matches<1>(a, la, b, lb);
    return extend(row_cap(delta ? f0 : f0 + 1, la), m) >= la ? 1u : 2u;
  }
  const uint32_t p1 = diagonal_matches<1>(a, la, b, lb);
  uint32_t n1 = 0, p2 = 0;
  if (delta == 0) n1 = diagonal_matches<-1>(a, la, b, lb);      // (diagonal -1 comes back to 0 only)
  if (delta == 2) p2 = diagonal_matches<2>(a, la, b, lb);
  const int32_t g0 = extend(row_cap(f0 + 1, la), m0);
  const int32_t gp = extend(row_cap(f0, la < lb - 1 ? la : lb - 1), p1);
  const int32_t gn = extend(row_cap(f0 + 1, la), n1);           // (lb + 1 > la)
  if ((delta == 0 ? g0 : gp) >= la && delta < 2) return 1;
  // step 2 on diagonal delta alone (la == lb - delta is its last row)
  int32_t from;
  uint32_t m;
  if (delta == 0) {
    from = g0 + 1 > gp + 1 ? g0 + 1 : gp + 1;
    from = from > gn ? from : gn;
    m = m0;
  } else if (delta == 1) {
    from = gp + 1 > g0 ? gp + 1 : g0;
    m = p1;
  } else {
    from = gp;
    m = p2;
  }
  return extend(row_cap(from, la), m) >= la ? 2u : 3u;
}

// ... for a limit given at run time (1 or 2; the same for every pair of a launch)
DCRX_CDR3NET_HD uint32_t lev_within(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb, uint32_t limit) {
  return limit == 1 ? lev_within_d<1>(a, la, b, lb) : lev_within_d<2>(a, la, b, lb);
}

}  // namespace dcrx_cdr3net

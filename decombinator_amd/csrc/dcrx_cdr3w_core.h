// dcrx_cdr3w_core.h — the pair test of the weighted (TCRdist-style) CDR3 distance of `match --cdr3-metric weighted`
// (dcrx_cdr3match.hip; include/dcrx.h "match, weighted"), shared by the kernel and a plain host build (tests/host_cdr3wmatch).
//
// Per node: whether a packed string (dcrx_cdr3net_core.h: eight dwords, zero beyond the length) holds letters 'A' .. 'Z' alone.
// Per pair: weighted_within, min(dist, R + 1) of the lane's OWN string (eight dwords in registers: every index into them is
// static once the loops are unrolled) and an OTHER string given as bytes (the kernel's LDS tile, where a run-time byte offset
// costs nothing), under a cost whose 32 x 32 byte table the caller has put where `sub` points (the kernel: LDS).
//
// The distance (a the shorter string, la bytes; b the longer, lb = la + d): d * gap + min over p in 0 .. la of
//   sum over counted i < p of sub[a[i]][b[i]]  +  sum over counted i >= p of sub[a[i]][b[i + d]],
// i counted when ntrim <= i < la - ctrim.  With P[i] = sub[a[i]][b[i]] and S[i] = sub[a[i]][b[i + d]] over the counted i (0
// elsewhere), total(p + 1) - total(p) = P[p] - S[p], so min over p of total(p) = sum S + min over p of sum over i < p of
// (P[i] - S[i]): one pass.  An uncounted i moves nothing, which is the plateau below ntrim and above la - ctrim.
// When the own string is the longer one its bytes i + d are needed at static i: the own words are shifted down by d bytes
// first (selects by the bits of d, then one byte alignment per word), and the other string is read at i alone.
#pragma once
#include <stdint.h>

#include "dcrx_cdr3net_core.h"

namespace dcrx_cdr3w {

using namespace dcrx_cdr3net;

constexpr uint32_t METRIC_WEIGHTED = DCRX_CDR3NET_WEIGHTED;
constexpr uint32_t SUB_DIM = 32, SUB_BYTES = SUB_DIM * SUB_DIM;
constexpr uint32_t MAX_GAP = 255, MAX_TRIM = 16, MAX_RADIUS = 65535;
constexpr uint64_t LEN_MASK = (1ull << LEN_BITS) - 1;

struct Cost {
  const uint8_t *sub;      // SUB_BYTES: row (byte & 31), column (byte & 31)
  uint32_t gap, ntrim, ctrim;
};

// Every one of the first len bytes (len <= MAX_LEN) of a packed string is 'A' .. 'Z'.  Per word, on the low seven bits of
// every byte: + 0x3F sets bit 7 from 'A' up, + 0x25 sets it from '[' up; a byte of 0x80 and more is out by its own bit 7.
DCRX_CDR3NET_HD bool letters_only(const uint32_t *w, uint32_t len) {
  uint32_t bad = 0;
  DCRX_CDR3NET_UNROLL
  for (uint32_t k = 0; k < WORDS; k++) {
    const uint32_t x = w[k], low = x & 0x7F7F7F7Fu;
    const uint32_t letter = (low + 0x3F3F3F3Fu) & ~(low + 0x25252525u) & ~x & 0x80808080u;
    const uint32_t expect = 0x80808080u & low_bits(8 * ((int32_t)len - 4 * (int32_t)k));
    bad |= letter ^ expect;      // (a byte beyond the length is zero: never a letter, never expected)
  }
  return bad == 0;
}

DCRX_CDR3NET_HD uint32_t byte_of(const uint32_t *w, uint32_t p) { return (w[p / 4] >> (8 * (p % 4))) & 0xFFu; }

// out's byte i = in's byte i + d (d in 0 .. 31), zero beyond the end
DCRX_CDR3NET_HD void shift_down(const uint32_t *in, uint32_t d, uint32_t *out) {
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) out[w] = in[w];
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) out[w] = (d & 16u) ? (w + 4 < WORDS ? out[w + 4] : 0u) : out[w];
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) out[w] = (d & 8u) ? (w + 2 < WORDS ? out[w + 2] : 0u) : out[w];
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) out[w] = (d & 4u) ? (w + 1 < WORDS ? out[w + 1] : 0u) : out[w];
  DCRX_CDR3NET_UNROLL
  for (uint32_t w = 0; w < WORDS; w++) out[w] = align_bytes(w + 1 < WORDS ? out[w + 1] : 0u, out[w], d & 3u);
}

DCRX_CDR3NET_HD uint32_t sub_cost(const Cost &C, uint32_t x, uint32_t y) { return C.sub[(x & 31u) * SUB_DIM + (y & 31u)]; }

// min(dist(own, other), R + 1) of two strings in reach that hold letters alone.  The lower bound d * gap + the sum of
// min(P, S) so far only grows and never passes the distance, so giving up once it has passed R changes no result.
DCRX_CDR3NET_HD uint32_t weighted_within(const uint32_t *own, uint32_t l_own, const uint8_t *other, uint32_t l_other, const Cost &C,
                                         uint32_t R) {
  const bool own_longer = l_own > l_other;
  const uint32_t la = own_longer ? l_other : l_own, d = own_longer ? l_own - l_other : l_other - l_own;
  const uint32_t base = d * C.gap;
  if (base > R) return R + 1;
  const int32_t lo = (int32_t)C.ntrim, hi = (int32_t)la - (int32_t)C.ctrim;
  if (d == 0) {      // no gap, no minimum
    uint32_t sum = 0;
    DCRX_CDR3NET_UNROLL
    for (uint32_t p = 0; p < MAX_LEN; p++) {
      if ((int32_t)p >= lo && (int32_t)p < hi) sum += sub_cost(C, byte_of(own, p), other[p]);
      if (p % 8 == 7 && sum > R) return R + 1;
    }
    return sum > R ? R + 1 : sum;
  }
  uint32_t shifted[WORDS];
  shift_down(own, own_longer ? d : 0u, shifted);
  const uint32_t d_other = own_longer ? 0u : d;
  uint32_t s_total = 0, lower = base;
  int32_t run = 0, best = 0;      // sum over i < p of (P[i] - S[i]), and its minimum over p (p = 0: nothing)
  DCRX_CDR3NET_UNROLL
  for (uint32_t p = 0; p < MAX_LEN; p++) {
    if ((int32_t)p >= lo && (int32_t)p < hi) {
      const uint32_t P = sub_cost(C, byte_of(own, p), other[p]), S = sub_cost(C, byte_of(shifted, p), other[p + d_other]);
      s_total += S;
      lower += P < S ? P : S;
      run += (int32_t)P - (int32_t)S;
      best = run < best ? run : best;
    }
    if (p % 8 == 7 && lower > R) return R + 1;
  }
  const uint32_t dist = base + (uint32_t)((int32_t)s_total + best);
  return dist > R ? R + 1 : dist;
}

}  // namespace dcrx_cdr3w

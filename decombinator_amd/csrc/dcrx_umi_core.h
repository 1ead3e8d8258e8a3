// dcrx_umi_core.h — the decisions of the UMI neighbour search (dcrx_umi.hip), shared by the kernel and a plain host build
// (tests/host_umi): can two tiles hold a pair within k (tiles_may_match), and is levenshtein(a, b) <= k for two UMIs of at
// most DCRX_UMI_MAX_LEN symbols (pair_distance)?
//
// A record (DCRX_UMI_REC_WORDS words) holds one UMI as the kernel needs it on both sides of a pair:
//   [0..7]   Peq: bit p of word s is set when symbol p is s (the pattern side of Myers' algorithm)
//   [8..10]  the symbols, 4 bits each, position p in word p / 8 (the text side)
//   [11]     length
//   [12..13] composition: byte s = how many times symbol s occurs (8 counts, one per byte)
//   [14]     the UMI's index in the caller's list
// Two filters come before the exact check, both lower bounds of the distance:
//   |len(a) - len(b)| > k, and the L1 distance of the compositions > 2k (one edit changes it by at most 2).
// The exact check is Myers' bit-vector edit distance in Hyyrö's global form (one 32-bit word: 24 bits suffice), with an
// early exit once the score can no longer come down to k (each remaining text symbol lowers it by one at most).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DCRX_UMI_HD __host__ __device__ __forceinline__
#else
#define DCRX_UMI_HD inline
#endif

namespace dcrx_umi {

enum { W_PEQ = 0, W_CODES = 8, W_LEN = 11, W_COMP = 12, W_INDEX = 14 };

DCRX_UMI_HD uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sad_u8(a, b, acc);        // v_sad_u8: sum of |a.byte - b.byte| plus acc
#else
  for (int s = 0; s < 32; s += 8) {
    const int x = (int)((a >> s) & 255u), y = (int)((b >> s) & 255u);
    acc += (uint32_t)(x > y ? x - y : y - x);
  }
  return acc;
#endif
}

// Lower bounds only: true when the pair may be within k.
DCRX_UMI_HD bool may_match(uint32_t len_a, uint32_t ca0, uint32_t ca1, uint32_t len_b, uint32_t cb0, uint32_t cb1, int32_t k) {
  const int32_t dl = (int32_t)len_a - (int32_t)len_b;
  if (dl > k || -dl > k) return false;
  return (int64_t)sad4(ca1, cb1, sad4(ca0, cb0, 0)) <= 2 * (int64_t)k;
}

// Levenshtein distance of pattern (Peq of m symbols) and text (n symbols, 4 bits each in codes[0..2]) when it is <= k,
// else some value > k.  m, n <= 24; requires |m - n| <= k (may_match).
DCRX_UMI_HD int32_t myers(const uint32_t *peq, uint32_t m, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t n, int32_t k) {
  if (m == 0) return (int32_t)n;
  const uint32_t hi = 1u << (m - 1);
  uint32_t pv = ~0u, mv = 0u;
  int32_t score = (int32_t)m;
  for (uint32_t t = 0; t < n; t++) {
    const uint32_t w = t < 8 ? c0 : (t < 16 ? c1 : c2);
    const uint32_t eq = peq[(w >> ((t & 7u) * 4u)) & 7u];
    const uint32_t xv = eq | mv;
    const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint32_t ph = mv | ~(xh | pv);
    uint32_t mh = pv & xh;
    score += (ph & hi) ? 1 : 0;
    score -= (mh & hi) ? 1 : 0;
    ph = (ph << 1) | 1u;                              // global distance: row 0 of the table grows by one per column
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    if (score - (int32_t)(n - 1 - t) > k) return k + 1;
  }
  return score;
}

// No two UMIs are farther apart than UMI_MAX_LEN edits, so a larger k asks for the same pairs: both entries of the search
// clamp k on the way in, and every int32 expression in k below (2 * k, k + 1) stays in range.
enum { UMI_MAX_LEN = 24 };
DCRX_UMI_HD int32_t clamp_k(int32_t k) { return k > UMI_MAX_LEN ? (int32_t)UMI_MAX_LEN : k; }

DCRX_UMI_HD int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

// Whole-tile lower bound: the smallest distance any pair of the two tiles can have by length and composition.  ta, tb: tile
// summaries (min length, max length, composition minima[2], maxima[2]).  k <= UMI_MAX_LEN (clamp_k).
DCRX_UMI_HD bool tiles_may_match(const uint32_t *ta, const uint32_t *tb, int32_t k) {
  const int32_t gap_len = imax((int32_t)tb[0] - (int32_t)ta[1], (int32_t)ta[0] - (int32_t)tb[1]);
  if (gap_len > k) return false;
  int32_t gap = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int w = 0; w < 2; w++) {
    const uint32_t amin = ta[2 + w], amax = ta[4 + w], bmin = tb[2 + w], bmax = tb[4 + w];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 0; s < 32; s += 8) {
      const int32_t a0 = (amin >> s) & 255, a1 = (amax >> s) & 255, b0 = (bmin >> s) & 255, b1 = (bmax >> s) & 255;
      gap += imax(0, imax(b0 - a1, a0 - b1));
    }
  }
  return gap <= 2 * k;
}

// The whole decision on two records, as the kernel takes it (b is the pattern, a the text).
DCRX_UMI_HD int32_t pair_distance(const uint32_t *a, const uint32_t *b, int32_t k) {
  if (!may_match(a[W_LEN], a[W_COMP], a[W_COMP + 1], b[W_LEN], b[W_COMP], b[W_COMP + 1], k)) return k + 1;
  return myers(b + W_PEQ, b[W_LEN], a[W_CODES], a[W_CODES + 1], a[W_CODES + 2], a[W_LEN], k);
}

}  // namespace dcrx_umi

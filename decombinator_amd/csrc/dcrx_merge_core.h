// dcrx_merge_core.h — the per-entry and per-pair code of the error merge (`decombine -nbc --count-dcrs --merge-errors`,
// dcrx_merge.hip), shared by the kernels and a plain host build (tests/host_merge).
//
// Per entry (v, j, vdel, jdel, insert): the junction string
//     Vr[len(Vr) - aV : len(Vr) - vdel] + insert + Jr[jdel : aJ],   aV = min(ANCHOR, len(Vr)), aJ = min(ANCHOR, len(Jr))
// — the slice of translate's rebuilt sequence (V[:-vdel] + insert + J[jdel:]) between two anchors that depend on (v, j)
// alone — as eight dwords of 2-bit bases (base p in bits [2(p % 16), 2(p % 16) + 1] of word p / 16; A=0 C=1 G=2 T=3, zero
// beyond the length), its length, whether the entry is in reach, and the bucket key (v, j, length).
// A gene's window is one row of WIN_WORDS words: the ANCHOR germline bytes next to the junction (the last aV of a V
// region, the first aJ of a J region; ASCII, upper case, zero padded), the window's length, and whether it holds only ACGT.
// Per pair: the Hamming distance of two junctions of one length, given up once it has passed the limit.
#pragma once
#include <stdint.h>

#include "../../include/dcrx.h"

#if defined(__HIPCC__)
#define DCRX_MERGE_HD __host__ __device__ __forceinline__
#else
#define DCRX_MERGE_HD inline
#endif

namespace dcrx_merge {

constexpr uint32_t ANCHOR = DCRX_MERGE_ANCHOR;
constexpr uint32_t MAX_JUNCTION = DCRX_MERGE_MAX_JUNCTION;
constexpr uint32_t WORDS = MAX_JUNCTION / 16;                 // dwords of one junction
constexpr uint32_t WIN_WORDS = ANCHOR / 4 + 2;                // bytes, length, clean flag
constexpr uint64_t KEY_OUT_OF_REACH = 1ull << 40;             // sorts behind every bucket of entries in reach
constexpr uint32_t KEY_BITS = 41;
static_assert(ANCHOR % 4 == 0 && MAX_JUNCTION % 16 == 0 && MAX_JUNCTION <= 255, "the key keeps the length in 8 bits");

// 0..3 for ACGT (upper case only: the insert is compared as stored), 4 for every other byte
DCRX_MERGE_HD uint32_t base_code(uint32_t c) {
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// One gene's window row out of its (upper-cased) region; is_v: the region's last bytes, else its first.
inline void make_window(const char *region, uint32_t len, bool is_v, uint32_t *row) {
  for (uint32_t w = 0; w < WIN_WORDS; w++) row[w] = 0;
  const uint32_t a = len < ANCHOR ? len : ANCHOR;
  const char *src = is_v ? region + (len - a) : region;
  uint32_t clean = 1;
  for (uint32_t p = 0; p < a; p++) {
    const uint32_t c = (uint8_t)src[p];
    row[p / 4] |= c << (8 * (p % 4));
    if (base_code(c) > 3) clean = 0;
  }
  row[ANCHOR / 4] = a;
  row[ANCHOR / 4 + 1] = clean;
}

DCRX_MERGE_HD uint32_t window_byte(const uint32_t *row, uint32_t p) { return (row[p / 4] >> (8 * (p % 4))) & 255u; }

DCRX_MERGE_HD uint64_t bucket_key(uint32_t v, uint32_t j, uint32_t length) {
  return ((uint64_t)(v & 0xFFFFu) << 24) | ((uint64_t)(j & 0xFFFFu) << 8) | (uint64_t)(length & 0xFFu);
}

// The junction of one entry into out[WORDS] and *length; returns whether the entry is in reach.  An entry out of reach
// gets zero words and length 0.
DCRX_MERGE_HD bool encode(const uint32_t *vrow, const uint32_t *jrow, uint32_t vdel, uint32_t jdel, const uint8_t *ins,
                          uint64_t ins_len, uint32_t *out, uint32_t *length) {
  for (uint32_t w = 0; w < WORDS; w++) out[w] = 0;
  *length = 0;
  const uint32_t av = vrow[ANCHOR / 4], aj = jrow[ANCHOR / 4];
  if (!vrow[ANCHOR / 4 + 1] || !jrow[ANCHOR / 4 + 1] || vdel > av || jdel > aj) return false;
  const uint64_t total = (uint64_t)(av - vdel) + ins_len + (uint64_t)(aj - jdel);
  if (total > MAX_JUNCTION) return false;
  uint32_t at = 0;
  for (uint32_t p = 0; p < av - vdel; p++, at++) out[at / 16] |= base_code(window_byte(vrow, p)) << (2 * (at % 16));
  bool clean = true;
  for (uint32_t p = 0; p < (uint32_t)ins_len; p++, at++) {
    const uint32_t c = base_code(ins[p]);
    clean = clean && c < 4;
    out[at / 16] |= (c & 3u) << (2 * (at % 16));
  }
  for (uint32_t p = jdel; p < aj; p++, at++) out[at / 16] |= base_code(window_byte(jrow, p)) << (2 * (at % 16));
  if (!clean) {
    for (uint32_t w = 0; w < WORDS; w++) out[w] = 0;
    return false;
  }
  *length = at;
  return true;
}

DCRX_MERGE_HD uint32_t popcount32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

// positions at which two words of 2-bit bases differ
DCRX_MERGE_HD uint32_t word_mismatches(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  return popcount32((x | (x >> 1)) & 0x55555555u);
}

// Hamming distance of two junctions of one length when it is <= limit, else some value > limit (given up after the
// first half once that alone has passed the limit).
DCRX_MERGE_HD uint32_t distance(const uint32_t *a, const uint32_t *b, uint32_t limit) {
  uint32_t d = 0;
  for (uint32_t w = 0; w < WORDS / 2; w++) d += word_mismatches(a[w], b[w]);
  if (d > limit) return d;
  for (uint32_t w = WORDS / 2; w < WORDS; w++) d += word_mismatches(a[w], b[w]);
  return d;
}

// count_c <= count_p / ratio, i.e. ratio * count_c <= count_p, without overflow: `need` = ratio * count_c, saturated.
DCRX_MERGE_HD bool needed_count(uint64_t count_c, uint64_t ratio, uint64_t *need) {
  if (count_c && ratio > ~0ull / count_c) return false;       // no 64-bit count reaches it
  *need = ratio * count_c;
  return true;
}

}  // namespace dcrx_merge

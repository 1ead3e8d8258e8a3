// dcrx_motif_core.h — the per-unit code of the motif step (`motifs`, dcrx_motif.hip), shared by the kernels and a plain host
// build (tests/host_motif): whether a unit takes part, the window range of a k under a trim, the code of a motif, a unit's
// motifs of one k with what occurs twice taken once, the digits the selection of a resample looks at, and how many resamples
// a chunk holds.  include/dcrx.h "motifs" holds the contract.
//
// A unit is packed as the CDR3 walk packs a string (dcrx_cdr3net_core.h: eight dwords, zero beyond the length) and takes part
// when dcrx_cdr3w_core.h's letters_only says so.  The words of a unit are read through a stride: a host caller hands eight
// consecutive words (stride 1), a kernel a column of an LDS array (stride: the block), so that no lane indexes registers at
// run time.
#pragma once
#include <stdint.h>

#include "dcrx_cdr3w_core.h"
#include "dcrx_rarefy_core.h"

namespace dcrx_motif {

constexpr uint32_t MAX_LEN = dcrx_cdr3net::MAX_LEN;      // 32
constexpr uint32_t WORDS = dcrx_cdr3net::WORDS;          // 8
constexpr uint32_t K_MIN = 2, K_MAX = 4;
constexpr uint32_t K_MASK_ALL = (1u << 2) | (1u << 3) | (1u << 4);      // bit k of a k_mask: k is in K
constexpr uint32_t MAX_TRIM = DCRX_CDR3_MOTIF_MAX_TRIM;
constexpr uint32_t MAX_RESAMPLES = DCRX_CDR3_MOTIF_MAX_RESAMPLES;
constexpr uint64_t MAX_UNITS = 1ull << 30;
constexpr uint32_t MAX_WINDOWS = MAX_LEN - K_MIN + 1;     // of one k in one unit (no trim, 32 letters, k = 2)
constexpr uint32_t MAX_PER_UNIT = (MAX_LEN - 1) + (MAX_LEN - 2) + (MAX_LEN - 3);      // motifs of one unit, all k
constexpr uint32_t LETTERS = 26;
constexpr uint32_t BASE2 = 0, BASE3 = BASE2 + 26 * 26, BASE4 = BASE3 + 26 * 26 * 26;
constexpr uint32_t MOTIFS = BASE4 + 26 * 26 * 26 * 26;    // 475 228: every (k, letters), numbered in motif order
constexpr uint32_t BLOCK = 256;                           // a block (dcrx_group.h's BLOCK); the kept lists are cut into runs of BLOCK
// the selection of one resample: a block, a histogram of one 8-bit digit of the keys per level, a bin per lane
constexpr uint32_t BIN_BITS = 8;
constexpr uint32_t BINS = 1u << BIN_BITS;
constexpr uint32_t LEVELS = 64 / BIN_BITS;
constexpr uint32_t CANDIDATES = 512;                      // keys of the threshold's bin that are written out, at most
// a chunk of resamples: its kept lists (n entries per resample) and its plane of counts (a row of the reported motifs per
// resample) fill CHUNK_WORDS dwords at most, and a chunk holds 1 .. MAX_CHUNK resamples
constexpr uint64_t CHUNK_WORDS = 1ull << 25;
constexpr uint32_t MAX_CHUNK = 64;
static_assert(BINS == BLOCK, "a lane owns a bin");
static_assert(BIN_BITS * LEVELS == 64, "the last level decides the key");

// the reported motifs of n sample units, at most
DCRX_CDR3NET_HD uint64_t max_reported(uint64_t n) { return n * MAX_PER_UNIT < MOTIFS ? n * MAX_PER_UNIT : MOTIFS; }
// the resamples of one chunk for n sample units
DCRX_CDR3NET_HD uint32_t chunk_of(uint64_t n) {
  const uint64_t row = max_reported(n) + n, fit = row ? CHUNK_WORDS / row : MAX_CHUNK;
  return fit < 1 ? 1u : fit > MAX_CHUNK ? MAX_CHUNK : (uint32_t)fit;
}

// the digit of level `level` (0: the top BIN_BITS bits), and the `levels` digits above it as one number
DCRX_CDR3NET_HD uint32_t digit(uint64_t k, uint32_t level) { return (uint32_t)(k >> (64 - BIN_BITS * (level + 1))) & (BINS - 1); }
DCRX_CDR3NET_HD uint64_t prefix_of(uint64_t k, uint32_t levels) { return levels ? k >> (64 - BIN_BITS * levels) : 0; }

// A unit takes part: 1 .. 32 bytes, all 'A' .. 'Z' (w: the packed unit, eight consecutive words)
DCRX_CDR3NET_HD bool takes_part(const uint32_t *w, uint64_t len) { return dcrx_cdr3net::in_reach(len) && dcrx_cdr3w::letters_only(w, (uint32_t)len); }

// The windows of k letters in a unit of L letters under the trim (N, C): p with N <= p and p + k <= L - C; their number
DCRX_CDR3NET_HD uint32_t window_count(uint32_t L, uint32_t N, uint32_t C, uint32_t k) {
  const int32_t last = (int32_t)L - (int32_t)C - (int32_t)k;
  return last >= (int32_t)N ? (uint32_t)(last - (int32_t)N + 1) : 0u;
}

DCRX_CDR3NET_HD uint32_t letter_at(const uint32_t *w, uint32_t stride, uint32_t p) { return ((w[(p / 4) * stride] >> (8 * (p % 4))) & 0xFFu) - 'A'; }

// The code of the k letters at p: the letters as a number to the base 26, the first one leading, so that codes of one k go
// up as the letters do; and the motif's number among all motifs, which goes up with (k, letters)
DCRX_CDR3NET_HD uint32_t code_at(const uint32_t *w, uint32_t stride, uint32_t p, uint32_t k) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < k; i++) c = c * LETTERS + letter_at(w, stride, p + i);
  return c;
}
DCRX_CDR3NET_HD uint32_t motif_id(uint32_t k, uint32_t code) { return (k == 2 ? BASE2 : k == 3 ? BASE3 : BASE4) + code; }
DCRX_CDR3NET_HD uint32_t id_k(uint32_t id) { return id < BASE3 ? 2u : id < BASE4 ? 3u : 4u; }
DCRX_CDR3NET_HD uint32_t id_code(uint32_t id) { return id - (id < BASE3 ? BASE2 : id < BASE4 ? BASE3 : BASE4); }

// The motifs of one k in a unit that takes part, each once: f(motif_id) per window whose code no earlier window has.
// codes: MAX_WINDOWS words of the caller's, read and written through cstride.
template <class F>
DCRX_CDR3NET_HD void unit_motifs(const uint32_t *w, uint32_t stride, uint32_t L, uint32_t N, uint32_t C, uint32_t k, uint32_t *codes,
                                 uint32_t cstride, F f) {
  uint32_t n = window_count(L, N, C, k);
  if (n > MAX_WINDOWS) n = MAX_WINDOWS;      // (never: L <= 32)
  for (uint32_t i = 0; i < n; i++) codes[i * cstride] = code_at(w, stride, N + i, k);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = codes[i * cstride];
    bool seen = false;
    for (uint32_t q = 0; q < i; q++) seen = seen || codes[q * cstride] == c;
    if (!seen) f(motif_id(k, c));
  }
}

// ---- motif groups (include/dcrx.h "motif groups"): the selected motifs and the members' sort

DCRX_CDR3NET_HD uint32_t codes_of(uint32_t k) { return k == 2 ? 26u * 26 : k == 3 ? 26u * 26 * 26 : k == 4 ? 26u * 26 * 26 * 26 : 0u; }
// whether (k, code) is a motif of K
DCRX_CDR3NET_HD bool is_motif(uint32_t k_mask, uint32_t k, uint32_t code) {
  return k >= K_MIN && k <= K_MAX && (k_mask >> k & 1u) && code < codes_of(k);
}
// The first of S selected motifs that is no motif of K or does not come strictly behind the one before it in motif order; S
// where the list is in order
DCRX_CDR3NET_HD uint64_t first_selected_fault(uint64_t S, const uint32_t *k, const uint32_t *code, uint32_t k_mask) {
  for (uint64_t s = 0; s < S; s++) {
    if (!is_motif(k_mask, k[s], code[s])) return s;
    if (s && motif_id(k[s], code[s]) <= motif_id(k[s - 1], code[s - 1])) return s;
  }
  return S;
}

// The members' sort: a posting is (row, unit), written in unit order and sorted stably by its row over MEMBER_ROW_BITS bits, so
// that the rows come out laid end to end, each in unit order.  A slot that holds no posting carries NO_MEMBER_ROW, which lies
// behind every row under those bits.
constexpr uint32_t MEMBER_ROW_BITS = 19;
constexpr uint64_t NO_MEMBER_ROW = ~0ull;
static_assert(MOTIFS <= (1u << MEMBER_ROW_BITS) - 1, "NO_MEMBER_ROW's low bits lie behind every row");
constexpr uint64_t MAX_MEMBER_KEYS = 1ull << 31;      // cap + n stays below it: what one sort takes

}  // namespace dcrx_motif

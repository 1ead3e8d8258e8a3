// dcrx_cdr3net_core.h — the per-node and per-pair code of the CDR3 network (`--cdr3-network`, dcrx_cdr3net.hip), shared by
// the kernels and a plain host build (tests/host_cdr3net).
//
// Per node (class, string): whether it is in reach (1 .. MAX_LEN bytes), the bucket key (class, length) — a node out of reach
// is keyed behind every bucket —, and the string as eight dwords (byte p in bits [8(p % 4), 8(p % 4) + 7] of word p / 4, zero
// beyond the length; the bytes as they are: nothing is folded or decoded).
// Per pair: the Hamming distance of two packed strings of one length, given up once it has passed the limit.
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

}  // namespace dcrx_cdr3net

// dcrx_count_core.h — the per-key code of the DCR count (dcrx_count.hip), shared by the kernels and a plain host build
// (tests/host_count, checked against Python): the key of one decombined read, its hash, and key equality.
//
// A DCR is (v, j, vdel, jdel, insert), insert being the frame read's bytes [ins_start, ins_start + ins_len): the read itself
// when frame == 1, its reverse complement when frame == 0 (decombine.py:1015-1020).  A key is
//   a header word:  v | j << 16 | vdel << 32 | jdel << 40 | ins_len << 48
//   the insert:     ins_len bytes, exactly what the `.n12` row's fifth field holds — exception bytes (lower case, N, IUPAC)
//                   included, complemented as Bio.Seq's ambiguous complement does in the reverse frame.
// Two keys are the same DCR only when the headers and every insert byte compare equal; the hash is a filter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DCRX_COUNT_HD __host__ __device__ __forceinline__
#else
#define DCRX_COUNT_HD inline
#endif

namespace dcrx_count {

// the hash of a read that is not counted (status != OK): never the hash of a key (those keep the top bit clear)
constexpr uint64_t NO_KEY = ~0ull;

DCRX_COUNT_HD uint64_t header(uint32_t v, uint32_t j, uint32_t vdel, uint32_t jdel, uint32_t ins_len) {
  return (uint64_t)(v & 0xFFFFu) | (uint64_t)(j & 0xFFFFu) << 16 | (uint64_t)(vdel & 0xFFu) << 32 |
         (uint64_t)(jdel & 0xFFu) << 40 | (uint64_t)(ins_len & 0xFFFFu) << 48;
}
DCRX_COUNT_HD uint32_t header_len(uint64_t h) { return (uint32_t)(h >> 48); }

// reference revcomp() (Bio.Seq's ambiguous-DNA complement, both cases, U like T) of one byte; other bytes stay as they are
DCRX_COUNT_HD uint8_t complement(uint8_t c) {
  const char *from = "ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu";
  const char *to = "TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna";
  for (int i = 0; i < 34; i++)
    if ((uint8_t)from[i] == c) return (uint8_t)to[i];
  return c;
}

// The insert of a read of `len` bases (2 bits each, base p in byte p / 4 at bit 2 (p % 4), A C G T = 0 1 2 3) into out[0,
// ins_len).  The read's exceptions are n_exc (position, byte) pairs, positions ascending: each replaces the base at its position.
DCRX_COUNT_HD void insert_bytes(const uint8_t *packed, uint32_t len, uint32_t frame, uint32_t ins_start, uint32_t ins_len,
                                const uint16_t *exc_pos, const uint8_t *exc_chr, uint32_t n_exc, uint8_t *out) {
  for (uint32_t i = 0; i < ins_len; i++) {
    const uint32_t q = frame ? ins_start + i : len - 1 - (ins_start + i);
    uint32_t code = (packed[q >> 2] >> (2 * (q & 3))) & 3u;
    if (!frame) code ^= 3u;                                   // A <-> T, C <-> G
    out[i] = (uint8_t)"ACGT"[code];
  }
  // the read positions the insert covers: [lo, hi)
  const uint32_t lo = frame ? ins_start : len - ins_start - ins_len, hi = lo + ins_len;
  for (uint32_t e = 0; e < n_exc; e++) {
    const uint32_t p = exc_pos[e];
    if (p < lo || p >= hi) continue;
    if (frame) out[p - ins_start] = exc_chr[e];
    else out[len - 1 - p - ins_start] = complement(exc_chr[e]);
  }
}

// 63-bit hash of a key (the top bit is clear: NO_KEY is no key's hash)
DCRX_COUNT_HD uint64_t key_hash(uint64_t hdr, const uint8_t *ins, uint32_t ins_len) {
  uint64_t h = hdr * 0x9E3779B97F4A7C15ull;
  for (uint32_t i = 0; i < ins_len; i++) h = (h ^ ins[i]) * 0x100000001B3ull;
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
  return h >> 1;
}

DCRX_COUNT_HD bool key_equal(uint64_t hdr_a, const uint8_t *a, uint64_t hdr_b, const uint8_t *b) {
  if (hdr_a != hdr_b) return false;
  const uint32_t n = header_len(hdr_a);
  for (uint32_t i = 0; i < n; i++)
    if (a[i] != b[i]) return false;
  return true;
}

}  // namespace dcrx_count

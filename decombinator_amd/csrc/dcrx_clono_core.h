// dcrx_clono_core.h — the per-entry code of the clonotype step (`translate --clonotypes`, dcrx_clono.hip), shared by the
// kernels and a plain host build (tests/host_clono): what dcrx_cdr3_batch (dcrx_translate.cpp) computes for one DCR, restated
// so that a GPU lane can do it without building the sequence or its translation.
//
// The sequence of an entry is V[:vend] + insert + J[jstart:], never materialised: base_at() reads it through the three
// pieces.  Translation starts at the first V base, so every codon wholly inside V[:vend] is a constant of the V gene and
// every codon wholly inside the J piece is a constant of (J gene, phase of its first base in J): the gene tables (one blob,
// build_blob) hold, per V gene, its frame-0 translation with the index of its first stop and of its first invalid codon, and
// per J gene and phase the translation with "next stop / next invalid codon at or after codon k".  aa_at() is then a
// look-up outside the insert, and a lane translates only the codons that touch the insert.
//
// Per entry (entry_calls): the calls of dcrx_cdr3_batch — status, in frame, stop, conserved C / F, productive, start and end
// of the CDR3, the lengths — with Python's index and slice rules, and for a productive entry where junction_aa / junction
// lie and the hash of its clonotype key (V call group, J call group, junction_aa bytes).  write_junction() writes the bytes,
// key_equal() compares two keys in full: the hash is a filter, never a verdict.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/dcrx.h"

#if defined(__HIPCC__)
#define DCRX_CLONO_HD __host__ __device__ __forceinline__
#else
#define DCRX_CLONO_HD inline
#endif

namespace dcrx_clono {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t MOTIF_TOKENS = 4;                     // the search looks at four residues: a longer motif never matches
constexpr uint32_t MOTIF_WORDS = 1 + MOTIF_TOKENS * 8;   // token count, then one 256-bit byte class per token
constexpr uint32_t MOTIF_TOO_LONG = MOTIF_TOKENS + 1;
constexpr uint32_t MOTIF_UNSERVED = NONE;                // syntax beyond literals, '.', classes: DCRX_CDR3_MOTIF_LEFT

enum : uint8_t { F_PRODUCTIVE = 1, F_IN_FRAME = 2, F_STOP = 4, F_CONSERVED_C = 8, F_CONSERVED_F = 16 };

// ---- translation: NCBI table 1 and Bio.Seq.translate's rules for ambiguity codes, as dcrx_translate.cpp has them ----

DCRX_CLONO_HD uint32_t upper_t(uint32_t c) {                 // str.upper(), then U read as T
  if (c >= 'a' && c <= 'z') c -= 32;
  return c == 'U' ? (uint32_t)'T' : c;
}
DCRX_CLONO_HD uint32_t base_code(uint32_t c) { return c == 'T' ? 0u : c == 'C' ? 1u : c == 'A' ? 2u : c == 'G' ? 3u : 4u; }
// bit k set: the letter can stand for base k (T C A G = 0 1 2 3); 0 for a letter that is no nucleotide code
DCRX_CLONO_HD uint32_t base_opts(uint32_t c) {
  switch (c) {
    case 'T': return 1; case 'C': return 2; case 'A': return 4; case 'G': return 8;
    case 'M': return 4 | 2; case 'R': return 4 | 8; case 'W': return 4 | 1; case 'S': return 2 | 8; case 'Y': return 2 | 1;
    case 'K': return 8 | 1; case 'V': return 4 | 2 | 8; case 'H': return 4 | 2 | 1; case 'D': return 4 | 8 | 1;
    case 'B': return 2 | 8 | 1; case 'X': return 15; case 'N': return 15;
    default: return 0;
  }
}
DCRX_CLONO_HD uint32_t codon_aa(uint32_t k) { return (uint32_t)"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"[k]; }

// one codon (letters already through upper_t); 0 when a letter is no nucleotide code
DCRX_CLONO_HD uint32_t translate_codon(uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t ia = base_code(a), ib = base_code(b), ic = base_code(c);
  if ((ia | ib | ic) < 4) return codon_aa(16 * ia + 4 * ib + ic);
  if (a == '-' && b == '-' && c == '-') return '-';
  const uint32_t oa = base_opts(a), ob = base_opts(b), oc = base_opts(c);
  if (!oa || !ob || !oc) return 0;
  uint32_t seen = 0;      // bit per letter 'A'..'Z', bit 26 for '*'
  for (uint32_t x = 0; x < 4; x++) if (oa >> x & 1)
    for (uint32_t y = 0; y < 4; y++) if (ob >> y & 1)
      for (uint32_t z = 0; z < 4; z++) if (oc >> z & 1) {
        const uint32_t r = codon_aa(16 * x + 4 * y + z);
        seen |= r == '*' ? (1u << 26) : (1u << (r - 'A'));
      }
  if (seen == (1u << 26)) return '*';
  if (seen & (1u << 26)) return 'X';
  if ((seen & (seen - 1)) == 0) {
    uint32_t k = 0;
    while (!(seen >> k & 1)) k++;
    return 'A' + k;
  }
  if (seen == ((1u << ('D' - 'A')) | (1u << ('N' - 'A')))) return 'B';
  if (seen == ((1u << ('E' - 'A')) | (1u << ('Q' - 'A')))) return 'Z';
  if (seen == ((1u << ('I' - 'A')) | (1u << ('L' - 'A')))) return 'J';
  return 'X';
}

// Python's s[start:stop] on a string of n characters
DCRX_CLONO_HD void pyslice(int64_t n, int64_t start, int64_t stop, int64_t &lo, int64_t &hi) {
  if (start < 0) { start += n; if (start < 0) start = 0; }
  if (start > n) start = n;
  if (stop < 0) { stop += n; if (stop < 0) stop = 0; }
  if (stop > n) stop = n;
  lo = start; hi = stop < start ? start : stop;
}

// ---- the gene tables: one blob, the same bytes on the host and on the device ----

struct Header {      // byte offsets into the blob (every array 8-byte aligned)
  uint32_t n_v, n_j;
  uint32_t v_off, v_text, j_off, j_text;            // regions: n + 1 uint32 offsets, then the bytes
  uint32_t v_pos, v_res, j_pos, j_motif;            // int32 positions; the V residue's byte (-1: not one character); MOTIF_WORDS per J
  uint32_t v_group, j_group;                        // call groups
  uint32_t vaa_off, vaa, v_stop, v_bad;             // frame-0 translation per V (0 for an invalid codon), first stop / invalid codon
  uint32_t jaa_off, jaa, j_stop, j_bad;             // per (J, phase): 3 n_j + 1 offsets; translation; next stop / invalid at or after k
  uint32_t bytes, pad;
};

struct View {
  uint32_t n_v, n_j;
  const uint32_t *v_off, *j_off, *j_motif, *v_group, *j_group, *vaa_off, *v_stop, *v_bad, *jaa_off, *j_stop, *j_bad;
  const int32_t *v_pos, *v_res, *j_pos;
  const uint8_t *v_text, *j_text, *vaa, *jaa;
};

inline View make_view(const Header &h, const uint8_t *base) {
  View G;
  G.n_v = h.n_v; G.n_j = h.n_j;
  auto u32 = [&](uint32_t off) { return reinterpret_cast<const uint32_t *>(base + off); };
  auto i32 = [&](uint32_t off) { return reinterpret_cast<const int32_t *>(base + off); };
  G.v_off = u32(h.v_off); G.j_off = u32(h.j_off); G.j_motif = u32(h.j_motif); G.v_group = u32(h.v_group); G.j_group = u32(h.j_group);
  G.vaa_off = u32(h.vaa_off); G.v_stop = u32(h.v_stop); G.v_bad = u32(h.v_bad);
  G.jaa_off = u32(h.jaa_off); G.j_stop = u32(h.j_stop); G.j_bad = u32(h.j_bad);
  G.v_pos = i32(h.v_pos); G.v_res = i32(h.v_res); G.j_pos = i32(h.j_pos);
  G.v_text = base + h.v_text; G.j_text = base + h.j_text; G.vaa = base + h.vaa; G.jaa = base + h.jaa;
  return G;
}

// A J gene's motif in the class-mask form: the subset of Python's `re` dcrx_cdr3_batch's matcher serves (literal characters,
// '.', character classes with ranges and a leading '^', a backslash in front of a literal).  row: MOTIF_WORDS words.
inline void compile_motif(const char *p, size_t n, uint32_t *row) {
  for (uint32_t w = 0; w < MOTIF_WORDS; w++) row[w] = 0;
  uint32_t count = 0;
  auto unserved = [&]() { row[0] = MOTIF_UNSERVED; };
  size_t i = 0;
  while (i < n) {
    uint32_t set[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto put = [&](uint32_t k) { set[k >> 5] |= 1u << (k & 31); };
    const char c = p[i];
    if (c == '.') { for (uint32_t k = 0; k < 256; k++) if (k != '\n') put(k); i++; }
    else if (c == '\\') {
      if (i + 1 >= n) return unserved();
      const char d = p[i + 1];
      if ((d >= 'a' && d <= 'z') || (d >= 'A' && d <= 'Z') || (d >= '0' && d <= '9')) return unserved();
      put((uint8_t)d); i += 2;
    } else if (c == '[') {
      size_t k = i + 1;
      bool neg = false, first = true, closed = false;
      if (k < n && p[k] == '^') { neg = true; k++; }
      while (k < n) {
        if (p[k] == ']' && !first) { closed = true; k++; break; }
        if (p[k] == '\\' || p[k] == '[') return unserved();
        if (k + 2 < n && p[k + 1] == '-' && p[k + 2] != ']') {
          const uint32_t lo = (uint8_t)p[k], hi = (uint8_t)p[k + 2];
          if (lo > hi) return unserved();
          for (uint32_t x = lo; x <= hi; x++) put(x);
          k += 3;
        } else { put((uint8_t)p[k]); k++; }
        first = false;
      }
      if (!closed) return unserved();
      if (neg) for (uint32_t w = 0; w < 8; w++) set[w] = ~set[w];
      i = k;
    } else if (strchr("()|*+?{}^$", c)) return unserved();
    else { put((uint8_t)c); i++; }
    if (i < n && strchr("*+?{", p[i])) return unserved();
    if (count < MOTIF_TOKENS) for (uint32_t w = 0; w < 8; w++) row[1 + count * 8 + w] = set[w];
    count++;
  }
  row[0] = count > MOTIF_TOKENS ? MOTIF_TOO_LONG : count;
}

// The blob of a gene set (v_group / j_group: one call group per gene).  Empty when a region or the whole passes 2^31 bytes.
inline std::vector<uint8_t> build_blob(const dcrx_cdr3_genes_t &S, const uint32_t *v_group, const uint32_t *j_group) {
  std::vector<uint8_t> blob(sizeof(Header));
  Header h;
  memset(&h, 0, sizeof h);
  h.n_v = S.n_v; h.n_j = S.n_j;
  bool ok = true;
  auto put = [&](const void *src, size_t bytes) {
    const size_t at = blob.size();
    if (at + bytes + 8 >= (1ull << 31)) { ok = false; return (uint32_t)0; }
    blob.resize(at + ((bytes + 7) & ~(size_t)7));
    if (bytes) memcpy(blob.data() + at, src, bytes);
    return (uint32_t)at;
  };
  auto put_u32 = [&](const std::vector<uint32_t> &x) { return put(x.data(), x.size() * 4); };
  auto regions = [&](uint32_t n, const char *text, const uint64_t *off, uint32_t &o_off, uint32_t &o_text) {
    std::vector<uint32_t> o(n + 1);
    for (uint32_t k = 0; k <= n; k++) {
      if (off[k] - off[0] >= (1ull << 31)) ok = false;
      o[k] = (uint32_t)(off[k] - off[0]);
    }
    o_off = put_u32(o);
    o_text = put(n ? text + off[0] : nullptr, n ? (size_t)(off[n] - off[0]) : 0);
  };
  {
    const uint64_t zero = 0;
    regions(S.n_v, S.v_regions, S.n_v ? S.v_region_off : &zero, h.v_off, h.v_text);
    regions(S.n_j, S.j_regions, S.n_j ? S.j_region_off : &zero, h.j_off, h.j_text);
  }
  if (!ok) return {};
  h.v_pos = put(S.v_pos, (size_t)S.n_v * 4);
  std::vector<uint32_t> res(S.n_v);
  for (uint32_t k = 0; k < S.n_v; k++)
    res[k] = S.v_res_off[k + 1] - S.v_res_off[k] == 1 ? (uint32_t)(uint8_t)S.v_res[S.v_res_off[k]] : NONE;
  h.v_res = put_u32(res);
  h.j_pos = put(S.j_pos, (size_t)S.n_j * 4);
  std::vector<uint32_t> motif((size_t)S.n_j * MOTIF_WORDS);
  for (uint32_t k = 0; k < S.n_j; k++)
    compile_motif(S.j_motif + S.j_motif_off[k], S.j_motif_off[k + 1] - S.j_motif_off[k], motif.data() + (size_t)k * MOTIF_WORDS);
  h.j_motif = put_u32(motif);
  h.v_group = put(v_group, (size_t)S.n_v * 4);
  h.j_group = put(j_group, (size_t)S.n_j * 4);
  // a piece's codons from base `from` on: the translation (0: invalid), and per codon the next stop / invalid codon at or
  // after it (one entry more than codons: NONE behind the last)
  auto codons = [&](const char *r, uint64_t len, uint64_t from, std::vector<uint8_t> &aa, std::vector<uint32_t> &stop,
                    std::vector<uint32_t> &bad) {
    const size_t at = aa.size();
    const uint64_t n = len >= from ? (len - from) / 3 : 0;
    aa.resize(at + n + 1, 0); stop.resize(at + n + 1, NONE); bad.resize(at + n + 1, NONE);
    for (uint64_t k = 0; k < n; k++) {
      const uint64_t b = from + 3 * k;
      aa[at + k] = (uint8_t)translate_codon(upper_t((uint8_t)r[b]), upper_t((uint8_t)r[b + 1]), upper_t((uint8_t)r[b + 2]));
    }
    for (uint64_t k = n; k-- > 0;) {
      stop[at + k] = aa[at + k] == '*' ? (uint32_t)k : stop[at + k + 1];
      bad[at + k] = aa[at + k] == 0 ? (uint32_t)k : bad[at + k + 1];
    }
  };
  {
    std::vector<uint8_t> aa;
    std::vector<uint32_t> stop, bad, off(S.n_v + 1, 0), first_stop(S.n_v), first_bad(S.n_v);
    for (uint32_t k = 0; k < S.n_v; k++) {
      codons(S.v_regions + S.v_region_off[k], S.v_region_off[k + 1] - S.v_region_off[k], 0, aa, stop, bad);
      first_stop[k] = stop[off[k]]; first_bad[k] = bad[off[k]];
      off[k + 1] = (uint32_t)aa.size();
    }
    h.vaa_off = put_u32(off); h.vaa = put(aa.data(), aa.size()); h.v_stop = put_u32(first_stop); h.v_bad = put_u32(first_bad);
  }
  {
    std::vector<uint8_t> aa;
    std::vector<uint32_t> stop, bad, off(3 * (size_t)S.n_j + 1, 0);
    for (uint32_t k = 0; k < S.n_j; k++)
      for (uint32_t p = 0; p < 3; p++) {
        codons(S.j_regions + S.j_region_off[k], S.j_region_off[k + 1] - S.j_region_off[k], p, aa, stop, bad);
        off[3 * (size_t)k + p + 1] = (uint32_t)aa.size();
      }
    h.jaa_off = put_u32(off); h.jaa = put(aa.data(), aa.size()); h.j_stop = put_u32(stop); h.j_bad = put_u32(bad);
  }
  if (!ok) return {};
  h.bytes = (uint32_t)blob.size();
  memcpy(blob.data(), &h, sizeof h);
  return blob;
}

// ---- one entry ----

struct Entry {
  const uint8_t *vr, *ins, *jr;      // jr points at J[jstart]
  int64_t vend, il, jlen, sn;        // bases taken from V, of the insert, from J; their sum
  uint32_t vi, ji, jstart;
};

// false: a gene index outside its table (Python's list index rules)
DCRX_CLONO_HD bool make_entry(const View &G, int32_t v, int32_t j, int32_t vdel, int32_t jdel, const uint8_t *ins, uint64_t il,
                              Entry &E) {
  int64_t vi = v, ji = j;
  if (vi < 0) vi += G.n_v;
  if (ji < 0) ji += G.n_j;
  if (vi < 0 || vi >= (int64_t)G.n_v || ji < 0 || ji >= (int64_t)G.n_j) return false;
  const int64_t vn = (int64_t)(G.v_off[vi + 1] - G.v_off[vi]), jn = (int64_t)(G.j_off[ji + 1] - G.j_off[ji]);
  int64_t lo = 0, hi = 0;
  if (vdel == 0) hi = vn;                            // ([:-0] would be empty: vdel == 0 is its own case)
  else pyslice(vn, 0, -(int64_t)vdel, lo, hi);
  E.vr = G.v_text + G.v_off[vi]; E.vend = hi;
  E.ins = ins; E.il = (int64_t)il;
  pyslice(jn, jdel, jn, lo, hi);
  E.jr = G.j_text + G.j_off[ji] + lo; E.jstart = (uint32_t)lo; E.jlen = hi - lo;
  E.sn = E.vend + E.il + E.jlen;
  E.vi = (uint32_t)vi; E.ji = (uint32_t)ji;
  return true;
}

DCRX_CLONO_HD uint32_t base_at(const Entry &E, int64_t i) {
  if (i < E.vend) return E.vr[i];
  i -= E.vend;
  if (i < E.il) return E.ins[i];
  return E.jr[i - E.il];
}

// the first codon that does not lie wholly inside V[:vend], and the first that lies wholly inside the J piece
DCRX_CLONO_HD int64_t codons_in_v(const Entry &E) { return E.vend / 3; }
DCRX_CLONO_HD int64_t first_j_codon(const Entry &E) { return (E.vend + E.il + 2) / 3; }
// the (J, phase) table of an entry and the table's codon that is the sequence's codon first_j_codon()
DCRX_CLONO_HD void j_table(const View &G, const Entry &E, uint32_t &table_at, int64_t &k0) {
  const int64_t jb = (int64_t)E.jstart + 3 * first_j_codon(E) - E.vend - E.il;
  table_at = G.jaa_off[3 * E.ji + (uint32_t)(jb % 3)];
  k0 = jb / 3;
}

DCRX_CLONO_HD uint32_t direct_aa(const Entry &E, int64_t i) {
  return translate_codon(upper_t(base_at(E, 3 * i)), upper_t(base_at(E, 3 * i + 1)), upper_t(base_at(E, 3 * i + 2)));
}

// residue i of the translation (0 <= i < sn / 3; 0 for an invalid codon)
DCRX_CLONO_HD uint32_t aa_at(const View &G, const Entry &E, int64_t i) {
  if (i < codons_in_v(E)) return G.vaa[G.vaa_off[E.vi] + i];
  const int64_t fj = first_j_codon(E);
  if (i >= fj) {
    uint32_t t; int64_t k0;
    j_table(G, E, t, k0);
    return G.jaa[t + k0 + (i - fj)];
  }
  return direct_aa(E, i);
}

DCRX_CLONO_HD uint64_t hash_mix(uint64_t h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}

// What entry_calls leaves of an entry: dcrx_clono_row_t (include/dcrx.h) and, for a productive entry, where the junctions lie.
struct Spans { int64_t aa_lo, aa_len, nt_lo, nt_len; };

DCRX_CLONO_HD void junction_spans(int64_t sn, int64_t start, int64_t end, Spans &S) {
  int64_t lo, hi;
  pyslice(sn / 3, start, end, lo, hi);
  S.aa_lo = lo; S.aa_len = hi - lo;
  pyslice(sn, start * 3, 3 * end, lo, hi);
  S.nt_lo = lo; S.nt_len = hi - lo;
}

DCRX_CLONO_HD void entry_calls(const View &G, int32_t v, int32_t j, int32_t vdel, int32_t jdel, const uint8_t *ins, uint64_t il,
                               dcrx_clono_row_t &R, Spans &S) {
  R.hash = 0; R.arena_off = 0; R.start_cdr3 = 0; R.end_cdr3 = 0; R.seq_len = 0; R.status = DCRX_CDR3_OK; R.flags = 0; R.pad = 0;
  S.aa_lo = S.aa_len = S.nt_lo = S.nt_len = 0;
  Entry E;
  if (!make_entry(G, v, j, vdel, jdel, ins, il, E)) { R.status = DCRX_CDR3_INDEX_ERROR; return; }
  const int64_t sn = E.sn, an = sn / 3, nv = codons_in_v(E), fj = first_j_codon(E);
  // the first invalid codon and whether there is a stop: V by its table, the codons that touch the insert one by one, J by its table
  int64_t bad = -1;
  bool stop = false;
  if (G.v_bad[E.vi] != NONE && (int64_t)G.v_bad[E.vi] < nv && (int64_t)G.v_bad[E.vi] < an) bad = G.v_bad[E.vi];
  stop = G.v_stop[E.vi] != NONE && (int64_t)G.v_stop[E.vi] < nv && (int64_t)G.v_stop[E.vi] < an;
  for (int64_t i = nv; bad < 0 && i < fj && i < an; i++) {
    const uint32_t r = direct_aa(E, i);
    if (!r) bad = i;
    stop |= r == '*';
  }
  if (fj < an) {
    uint32_t t; int64_t k0;
    j_table(G, E, t, k0);
    if (bad < 0 && G.j_bad[t + k0] != NONE) bad = fj + ((int64_t)G.j_bad[t + k0] - k0);
    stop |= G.j_stop[t + k0] != NONE;
  }
  if (bad >= 0) { R.status = DCRX_CDR3_BAD_CODON; R.start_cdr3 = (int32_t)(uint32_t)(3 * bad); return; }
  uint8_t flags = 0;
  bool productive = sn % 3 == 1;                        // the reference's test, (len - 1) % 3 == 0
  if (productive) flags |= F_IN_FRAME;
  if (stop) { flags |= F_STOP; productive = false; }
  int64_t start = 0;
  {
    int64_t idx = (int64_t)G.v_pos[E.vi] - 1;
    const int64_t raw = idx;
    if (idx < 0) idx += an;
    if (idx < 0 || idx >= an) { R.status = DCRX_CDR3_INDEX_ERROR; return; }
    if (G.v_res[E.vi] >= 0 && aa_at(G, E, idx) == (uint32_t)G.v_res[E.vi]) { start = raw; flags |= F_CONSERVED_C; }
    else productive = false;
  }
  int64_t dlo, dhi, slo, shi;
  pyslice(an, start, an, dlo, dhi);
  const int64_t dn = dhi - dlo, jp = G.j_pos[E.ji];
  pyslice(dn, jp, jp + 4, slo, shi);
  int64_t end = 0;
  const uint32_t *M = G.j_motif + (size_t)E.ji * MOTIF_WORDS;
  if (M[0] == MOTIF_UNSERVED) R.status = DCRX_CDR3_MOTIF_LEFT;
  else {
    const int64_t k = M[0], wn = shi - slo;
    bool found = false;
    for (int64_t o = 0; !found && o + k <= wn; o++) {
      bool hit = true;
      for (int64_t x = 0; x < k && hit; x++) {
        const uint32_t r = aa_at(G, E, dlo + slo + o + x);
        hit = (M[1 + x * 8 + (r >> 5)] >> (r & 31)) & 1u;
      }
      found = hit;
    }
    if (found) { end = dn + jp + start + 1; flags |= F_CONSERVED_F; }
    else productive = false;
  }
  if (productive) flags |= F_PRODUCTIVE;
  R.flags = flags; R.start_cdr3 = (int32_t)start; R.end_cdr3 = (int32_t)end; R.seq_len = (uint32_t)sn;
  if (productive && R.status == DCRX_CDR3_OK) {
    junction_spans(sn, start, end, S);
    uint64_t h = hash_mix(((uint64_t)G.v_group[E.vi] << 32 | G.j_group[E.ji]) ^ ((uint64_t)S.aa_len * 0x9e3779b97f4a7c15ull));
    for (int64_t i = 0; i < S.aa_len; i++) h = (h ^ aa_at(G, E, S.aa_lo + i)) * 0x100000001b3ull;
    R.hash = hash_mix(h);
  }
}

// the junction bytes of a productive entry: junction_aa (S.aa_len bytes), then junction (S.nt_len, as the sequence holds them)
DCRX_CLONO_HD void write_junction(const View &G, int32_t v, int32_t j, int32_t vdel, int32_t jdel, const uint8_t *ins, uint64_t il,
                                  const dcrx_clono_row_t &R, uint8_t *out) {
  Entry E;
  if (!make_entry(G, v, j, vdel, jdel, ins, il, E)) return;
  Spans S;
  junction_spans(E.sn, R.start_cdr3, R.end_cdr3, S);
  for (int64_t i = 0; i < S.aa_len; i++) out[i] = (uint8_t)aa_at(G, E, S.aa_lo + i);
  for (int64_t i = 0; i < S.nt_len; i++) out[S.aa_len + i] = (uint8_t)base_at(E, S.nt_lo + i);
}

DCRX_CLONO_HD uint32_t gene_index(int32_t g, uint32_t n) { return g < 0 ? (uint32_t)(g + (int64_t)n) : (uint32_t)g; }

// Two members' keys in full: the call groups, the junction_aa's length and its bytes (a: the bytes at the row's arena_off).
DCRX_CLONO_HD bool key_equal(const View &G, int32_t va, int32_t ja, uint64_t len_a, const uint8_t *a, int32_t vb, int32_t jb,
                             uint64_t len_b, const uint8_t *b) {
  if (G.v_group[gene_index(va, G.n_v)] != G.v_group[gene_index(vb, G.n_v)]) return false;
  if (G.j_group[gene_index(ja, G.n_j)] != G.j_group[gene_index(jb, G.n_j)]) return false;
  if (len_a != len_b) return false;
  for (uint64_t i = 0; i < len_a; i++) if (a[i] != b[i]) return false;
  return true;
}

// the junction_aa's length of a member's row
DCRX_CLONO_HD uint64_t junction_aa_len(const dcrx_clono_row_t &R) {
  Spans S;
  junction_spans(R.seq_len, R.start_cdr3, R.end_cdr3, S);
  return (uint64_t)S.aa_len;
}

}  // namespace dcrx_clono

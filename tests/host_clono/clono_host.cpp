// Test-only: the clonotype step's per-entry code (dcrx_clono_core.h) built by g++, for a check against dcrx_cdr3_batch on the
// host.  clono_host_calls is the primitive in its plainest form: the calls of every entry in a loop, the junction bytes of
// the productive ones back to back in an arena, through the same entry_calls / write_junction the kernels use.
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_clono_core.h"

using namespace dcrx_clono;

extern "C" {
// rows: n dcrx_clono_row_t; returns the bytes the arena takes (written when they fit arena_cap), -1 for tables past 2^31 bytes
int64_t clono_host_calls(const dcrx_cdr3_genes_t *genes, const uint32_t *v_group, const uint32_t *j_group, uint64_t n, const int32_t *v,
                         const int32_t *j, const int32_t *vdel, const int32_t *jdel, const uint64_t *ins_off, const uint8_t *ins_text,
                         dcrx_clono_row_t *rows, uint8_t *arena, uint64_t arena_cap) {
  const std::vector<uint8_t> blob = build_blob(*genes, v_group, j_group);
  if (blob.empty()) return -1;
  Header h;
  memcpy(&h, blob.data(), sizeof h);
  const View G = make_view(h, blob.data());
  uint64_t at = 0;
  for (uint64_t k = 0; k < n; k++) {
    Spans S;
    const uint8_t *ins = ins_text + ins_off[k];
    const uint64_t il = ins_off[k + 1] - ins_off[k];
    entry_calls(G, v[k], j[k], vdel[k], jdel[k], ins, il, rows[k], S);
    const uint64_t bytes = (uint64_t)(S.aa_len + S.nt_len);
    if (rows[k].status == DCRX_CDR3_OK && (rows[k].flags & F_PRODUCTIVE)) {
      rows[k].arena_off = at;
      if (arena && at + bytes <= arena_cap) write_junction(G, v[k], j[k], vdel[k], jdel[k], ins, il, rows[k], arena + at);
    }
    at += bytes;
  }
  return (int64_t)at;
}

// 1 when the two members' keys compare equal in full (a, b: their junction_aa bytes)
int clono_host_key_equal(const dcrx_cdr3_genes_t *genes, const uint32_t *v_group, const uint32_t *j_group, int32_t va, int32_t ja,
                         uint64_t len_a, const uint8_t *a, int32_t vb, int32_t jb, uint64_t len_b, const uint8_t *b) {
  const std::vector<uint8_t> blob = build_blob(*genes, v_group, j_group);
  if (blob.empty()) return -1;
  Header h;
  memcpy(&h, blob.data(), sizeof h);
  return key_equal(make_view(h, blob.data()), va, ja, len_a, a, vb, jb, len_b, b) ? 1 : 0;
}

// Python's s[start:stop] on n characters, as the per-entry code has it
void clono_host_pyslice(int64_t n, int64_t start, int64_t stop, int64_t *lo, int64_t *hi) { pyslice(n, start, stop, *lo, *hi); }
}

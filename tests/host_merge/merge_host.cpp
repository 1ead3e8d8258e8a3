// Test-only: the merge kernels' per-entry and per-pair code (dcrx_merge_core.h) built by g++, for a check against Python on
// the host.  merge_host_parents is the parents step over a whole table in its plainest form (every pair of a bucket, through
// the same encode / distance / needed_count the kernels use).
#include <vector>

#include "../../decombinator_amd/csrc/dcrx_merge_core.h"

using namespace dcrx_merge;

extern "C" {
uint32_t merge_host_win_words(void) { return WIN_WORDS; }
uint32_t merge_host_words(void) { return WORDS; }
void merge_host_window(const char *region, uint32_t len, int is_v, uint32_t *row) { make_window(region, len, is_v != 0, row); }
int merge_host_encode(const uint32_t *vrow, const uint32_t *jrow, uint32_t vdel, uint32_t jdel, const uint8_t *ins, uint64_t ins_len,
                      uint32_t *out, uint32_t *length) {
  return encode(vrow, jrow, vdel, jdel, ins, ins_len, out, length) ? 1 : 0;
}
uint32_t merge_host_distance(const uint32_t *a, const uint32_t *b, uint32_t limit) { return distance(a, b, limit); }
uint64_t merge_host_key(uint32_t v, uint32_t j, uint32_t length) { return bucket_key(v, j, length); }

// rows: n_v V windows, then n_j J windows.  parent[k] = the eligible parent of the smallest rank, or k.
void merge_host_parents(const uint32_t *rows, uint32_t n_v, uint64_t n, const uint16_t *v, const uint16_t *j, const uint8_t *vdel,
                        const uint8_t *jdel, const uint64_t *count, const uint64_t *ins_off, const uint8_t *ins_text,
                        uint32_t limit, uint64_t ratio, uint32_t *parent, uint8_t *reach) {
  std::vector<uint32_t> junc(n * WORDS);
  std::vector<uint64_t> key(n);
  for (uint64_t k = 0; k < n; k++) {
    uint32_t length = 0;
    const bool ok = encode(rows + (size_t)v[k] * WIN_WORDS, rows + (size_t)(n_v + j[k]) * WIN_WORDS, vdel[k], jdel[k],
                           ins_text + ins_off[k], ins_off[k + 1] - ins_off[k], junc.data() + k * WORDS, &length);
    reach[k] = ok ? 1 : 0;
    key[k] = ok ? bucket_key(v[k], j[k], length) : KEY_OUT_OF_REACH;
  }
  for (uint64_t c = 0; c < n; c++) {
    parent[c] = (uint32_t)c;
    uint64_t need = 0;
    if (!reach[c] || !needed_count(count[c], ratio, &need)) continue;
    for (uint64_t p = 0; p < c; p++)
      if (key[p] == key[c] && count[p] >= need && distance(junc.data() + c * WORDS, junc.data() + p * WORDS, limit) <= limit) {
        parent[c] = (uint32_t)p;
        break;
      }
  }
}
}

// dcrx_merge.hip — the error merge of the barcode-free count (`decombine -nbc --count-dcrs --merge-errors`): every counted
// DCR whose junction (dcrx_merge_core.h) lies within D substitutions of a DCR of the same (v, j, length) that is at least R
// times as abundant is folded into it; include/dcrx.h holds the contract.
//
// The primitive (dcrx_merge_parents_device), all on the caller's stream and in the caller's work space:
//   keys     one lane per entry: the junction's length and reach flag, hence the bucket key (v, j, length); entries out of
//            reach get a key behind every bucket
//   sort     the keys with the entries' ranks (hipCUB radix sort, 41 bits; stable: a bucket stays in rank order, which is
//            count descending)
//   gather   one lane per sorted position: the junction's eight dwords and the count next to each other in sorted order,
//            and a flag where a bucket starts (a max scan then gives every position its bucket's start)
//   parents  one lane per child.  Its eligible parents by ratio are a PREFIX of its bucket (the bucket is in count order),
//            and the parent wanted is the first hit there.  A block of BLOCK consecutive children walks the sorted entries
//            from its first child's bucket start upwards in tiles of TILE: the tile's junctions and counts go to LDS, and
//            every lane reads the same staged entry at the same time (one broadcast read per dword, no bank conflicts),
//            XORs its own eight dwords held in registers against it and counts the mismatches, giving up after four
//            dwords once the limit is passed.  A lane drops out at its first hit, at the first staged count below
//            R * its own, or when the walk reaches the lane itself; a wave leaves a tile, and the block the walk, once all
//            lanes have.  Every child writes its own parent: no atomics.
// The host entry (dcrx_merge_dcrs) adds: pointer jumping to the roots (with the depth of every entry), the trees' totals
// (integer atomicAdd / atomicMin onto the roots, results unused), and the roots compacted in rank order (exclusive scan)
// and put in most_common() order.  The sorts, scans, run heads, compaction and order are dcrx_group.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_group.h"
#include "dcrx_merge_core.h"

namespace dcrx {
// dcrx_api.cpp: the handle's window rows (n_v rows for V, then n_j for J) on the current device
int merge_windows(dcrx_tables_t *t, const uint32_t **d_rows, uint32_t *n_v, uint32_t *n_j);
}
using dcrx::set_err;
using namespace dcrx_merge;
using namespace dcrx_group;

namespace {

constexpr int TILE = 256;        // staged entries per step: 8 KB of junctions + 2 KB of counts

struct Entries {
  const uint16_t *v, *j;
  const uint8_t *vdel, *jdel;
  const uint64_t *count, *ins_off;
  const uint8_t *ins_text;
  uint64_t text_bytes;
  const uint32_t *rows;
  uint32_t n_v, n_j;
};

// the junction of entry e (false and zeroes when it is out of reach)
__device__ __forceinline__ bool encode_entry(const Entries &E, uint32_t e, uint32_t *out, uint32_t *length) {
  const uint32_t v = E.v[e], j = E.j[e];
  const uint64_t a = E.ins_off[e], b = E.ins_off[e + 1];
  if (v >= E.n_v || j >= E.n_j || b < a || b > E.text_bytes) {
    for (uint32_t w = 0; w < WORDS; w++) out[w] = 0;
    *length = 0;
    return false;
  }
  return encode(E.rows + (size_t)v * WIN_WORDS, E.rows + (size_t)(E.n_v + j) * WIN_WORDS, E.vdel[e], E.jdel[e], E.ins_text + a,
                b - a, out, length);
}

__global__ __launch_bounds__(BLOCK) void merge_keys_kernel(Entries E, uint32_t n, uint64_t *__restrict__ key,
                                                           uint32_t *__restrict__ idx) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  uint32_t words[WORDS], length;
  const bool reach = encode_entry(E, e, words, &length);
  key[e] = reach ? bucket_key(E.v[e], E.j[e], length) : KEY_OUT_OF_REACH;
  idx[e] = e;
}

__global__ __launch_bounds__(BLOCK) void merge_gather_kernel(Entries E, uint32_t n, const uint64_t *__restrict__ key,
                                                             const uint32_t *__restrict__ idx, uint4 *__restrict__ sj,
                                                             uint64_t *__restrict__ sc, uint32_t *__restrict__ head) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= n) return;
  const uint32_t e = idx[s];
  uint32_t w[WORDS], length;
  encode_entry(E, e, w, &length);
  sj[2 * (size_t)s] = make_uint4(w[0], w[1], w[2], w[3]);
  sj[2 * (size_t)s + 1] = make_uint4(w[4], w[5], w[6], w[7]);
  sc[s] = E.count[e];
  head[s] = run_mark(s, [&](uint32_t k) { return key[k]; });
}

__global__ __launch_bounds__(BLOCK) void merge_parents_kernel(const uint4 *__restrict__ sj, const uint64_t *__restrict__ sc,
                                                              const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx,
                                                              const uint32_t *__restrict__ bstart, uint32_t n, uint32_t limit,
                                                              uint64_t ratio, uint32_t *__restrict__ parent,
                                                              uint8_t *__restrict__ reach_out) {
  __shared__ uint4 lds_j[TILE * 2];
  __shared__ uint64_t lds_c[TILE];
  const uint32_t s0 = blockIdx.x * BLOCK;
  const uint32_t s = s0 + threadIdx.x;
  const bool valid = s < n;
  uint32_t own[WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t start = s, found = s;
  uint64_t need = 0;
  bool done = true, reach = false;
  if (valid) {
    reach = key[s] != KEY_OUT_OF_REACH;
    start = bstart[s];
    // nothing to search: out of reach, first of its bucket, or even the bucket's largest count is below R * own
    if (reach && start < s && needed_count(sc[s], ratio, &need) && sc[start] >= need) {
      done = false;
      const uint4 a = sj[2 * (size_t)s], b = sj[2 * (size_t)s + 1];
      own[0] = a.x; own[1] = a.y; own[2] = a.z; own[3] = a.w; own[4] = b.x; own[5] = b.y; own[6] = b.z; own[7] = b.w;
    }
  }
  const uint32_t lo = bstart[s0];                           // (bstart never falls along s: the block's smallest)
  const uint32_t hi = min(n, s0 + (uint32_t)BLOCK);         // a parent stands before its child
  for (uint32_t t = lo; t < hi; t += TILE) {
    if (!__syncthreads_or(!done)) break;                    // (also: the previous tile is no longer read)
    const uint32_t tile_n = min((uint32_t)TILE, hi - t);
    if (threadIdx.x < tile_n) {
      const uint32_t p = t + threadIdx.x;
      lds_j[2 * threadIdx.x] = sj[2 * (size_t)p];
      lds_j[2 * threadIdx.x + 1] = sj[2 * (size_t)p + 1];
      lds_c[threadIdx.x] = sc[p];
    }
    __syncthreads();
    const uint32_t *lj = reinterpret_cast<const uint32_t *>(lds_j);
    for (uint32_t q = 0; q < tile_n; q++) {
      const uint32_t p = t + q;
      if (!done && p >= start) {
        if (p >= s || lds_c[q] < need) done = true;         // the walk reached the child, or its prefix has ended
        else if (distance(own, lj + q * WORDS, limit) <= limit) { found = p; done = true; }
      }
      if ((q & 7u) == 7u && !__ballot(!done)) break;        // the whole wave has dropped out
    }
  }
  if (valid) {
    const uint32_t e = idx[s];
    parent[e] = found == s ? e : idx[found];
    if (reach_out) reach_out[e] = reach ? 1 : 0;
  }
}

// ---- roots, totals, order (the host entry) ----

__global__ __launch_bounds__(BLOCK) void merge_depth_init_kernel(const uint32_t *__restrict__ parent, uint32_t n,
                                                                 uint32_t *__restrict__ depth) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) depth[i] = parent[i] != i ? 1u : 0u;
}

// one round of pointer jumping: every entry's pointer moves to its pointer's pointer, its depth grows by that entry's
__global__ __launch_bounds__(BLOCK) void merge_jump_kernel(const uint32_t *__restrict__ r_in, const uint32_t *__restrict__ d_in,
                                                           uint32_t n, uint32_t *__restrict__ r_out, uint32_t *__restrict__ d_out,
                                                           uint32_t *__restrict__ changed) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  bool moved = false;
  if (i < n) {
    const uint32_t r = r_in[i], rr = r_in[r];
    r_out[i] = rr;
    d_out[i] = d_in[i] + (rr != r ? d_in[r] : 0u);
    moved = rr != r;
  }
  if (__ballot(moved) && __lane_id() == 0) *changed = 1u;
}

enum { MS_OUT_OF_REACH = 0, MS_MERGED = 1, MS_MOVED = 2, MS_CHAIN = 3, MS_WORDS = 4 };

__global__ __launch_bounds__(BLOCK) void merge_totals_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ depth,
                                                             const uint8_t *__restrict__ reach, const uint64_t *__restrict__ count,
                                                             const uint64_t *__restrict__ first, uint32_t n,
                                                             unsigned long long *__restrict__ tot_count,
                                                             unsigned long long *__restrict__ tot_first,
                                                             uint32_t *__restrict__ is_root, unsigned long long *__restrict__ stats) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  unsigned long long oor = 0, merged = 0, moved = 0, chain = 0;
  if (i < n) {
    const uint32_t r = root[i];
    is_root[i] = r == i ? 1u : 0u;
    oor = reach[i] ? 0 : 1;
    chain = depth[i];
    if (r != i) {
      merged = 1;
      moved = count[i];
      atomicAdd(&tot_count[r], (unsigned long long)count[i]);
      atomicMin(&tot_first[r], (unsigned long long)first[i]);
    }
  }
#pragma unroll
  for (int d = warpSize / 2; d > 0; d >>= 1) chain = max(chain, (unsigned long long)__shfl_down(chain, d));
  oor = wave_sum(oor); merged = wave_sum(merged); moved = wave_sum(moved);
  if (__lane_id() == 0) {
    if (oor) atomicAdd(&stats[MS_OUT_OF_REACH], oor);
    if (merged) atomicAdd(&stats[MS_MERGED], merged);
    if (moved) atomicAdd(&stats[MS_MOVED], moved);
    if (chain) atomicMax(&stats[MS_CHAIN], chain);
  }
}

// ---- work space of the primitive; when it is done the host entry's compaction and order reuse key, idx and cub
struct Work {
  uint64_t *key[2];
  uint32_t *idx[2];
  uint4 *sj;
  uint64_t *sc;
  uint32_t *head, *bstart;
  Scratch cub;
  int carve(Pool &P, uint64_t n) {
    // (the largest of the primitive's sort and scan and of the host entry's scan and 64-bit sorts)
    const uint64_t wn = std::max<uint64_t>(n, 1);
    size_t cub_bytes = 0;
    int rc;
    if ((rc = sort_pairs_bytes<uint32_t>(wn, (int)KEY_BITS, &cub_bytes)) || (rc = run_heads_bytes(wn, &cub_bytes)) ||
        (rc = exclusive_sum_bytes<uint32_t>(wn, &cub_bytes)) || (rc = sort_pairs_bytes<uint32_t>(wn, 64, &cub_bytes))) return rc;
    P.get(&key[0], n); P.get(&key[1], n); P.get(&idx[0], n); P.get(&idx[1], n); P.get(&sj, 2 * n); P.get(&sc, n);
    P.get(&head, n); P.get(&bstart, n); P.get(&cub, cub_bytes);
    return DCRX_OK;
  }
};

// keys, sort, gather, bucket starts, parents (E.rows are the tables' windows)
int run_parents(const Entries &E, uint64_t n, uint32_t distance, uint64_t ratio, uint32_t *d_parent, uint8_t *d_reach, const Work &W,
                hipStream_t s) {
  const uint32_t n32 = (uint32_t)n;
  int rc;
  merge_keys_kernel<<<grid_for(n), BLOCK, 0, s>>>(E, n32, W.key[0], W.idx[0]);
  HIP_TRY(hipGetLastError());
  if ((rc = sort_pairs(W.cub, W.key[0], W.key[1], W.idx[0], W.idx[1], n, (int)KEY_BITS, s))) return rc;
  merge_gather_kernel<<<grid_for(n), BLOCK, 0, s>>>(E, n32, W.key[1], W.idx[1], W.sj, W.sc, W.head);
  HIP_TRY(hipGetLastError());
  if ((rc = run_heads(W.cub, W.head, W.bstart, n, s))) return rc;
  merge_parents_kernel<<<grid_for(n), BLOCK, 0, s>>>(W.sj, W.sc, W.key[1], W.idx[1], W.bstart, n32, distance, ratio, d_parent, d_reach);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

}  // namespace

extern "C" {

uint64_t dcrx_merge_work_bytes(uint64_t n) {
  Pool P;
  Work W;
  if (n >= (1ull << 31) || W.carve(P, n) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_merge_parents_device(dcrx_tables_t *tables, uint64_t n, const uint16_t *d_v, const uint16_t *d_j,
                              const uint8_t *d_vdel, const uint8_t *d_jdel, const uint64_t *d_count,
                              const uint64_t *d_ins_off, const char *d_ins_text, uint64_t text_bytes, uint32_t distance,
                              uint64_t ratio, uint32_t *d_parent, uint8_t *d_reach, void *d_work, uint64_t work_bytes,
                              void *hip_stream) {
  if (!tables) return set_err(DCRX_E_INVALID, "dcrx_merge_parents_device: tables is null");
  if (distance < 1 || distance > 2) return set_err(DCRX_E_INVALID, "dcrx_merge_parents_device: the distance is 1 or 2");
  if (ratio < 1) return set_err(DCRX_E_INVALID, "dcrx_merge_parents_device: the ratio is an integer >= 1");
  if (n >= (1ull << 31)) return set_err(DCRX_E_UNSUPPORTED, "dcrx_merge_parents_device: 2^31 or more entries");
  if (!n) return DCRX_OK;
  if (!d_v || !d_j || !d_vdel || !d_jdel || !d_count || !d_ins_off || !d_parent || !d_work || (text_bytes && !d_ins_text))
    return set_err(DCRX_E_INVALID, "dcrx_merge_parents_device: null argument");
  if ((uintptr_t)d_work % ALIGN) return set_err(DCRX_E_INVALID, "dcrx_merge_parents_device: the work space is not 256-byte aligned");
  Pool P(d_work);
  Work W;
  int rc = W.carve(P, n);
  if (rc) return rc;
  if (work_bytes < P.bytes()) return set_err(DCRX_E_INVALID, "dcrx_merge_parents_device: the work space is smaller than dcrx_merge_work_bytes(n)");
  Entries E{d_v, d_j, d_vdel, d_jdel, d_count, d_ins_off, reinterpret_cast<const uint8_t *>(d_ins_text), text_bytes, nullptr, 0, 0};
  if ((rc = dcrx::merge_windows(tables, &E.rows, &E.n_v, &E.n_j))) return rc;
  return run_parents(E, n, distance, ratio, d_parent, d_reach, W, (hipStream_t)hip_stream);
}

int64_t dcrx_merge_dcrs(dcrx_tables_t *tables, uint64_t n, const uint16_t *v, const uint16_t *j, const uint8_t *vdel,
                        const uint8_t *jdel, const uint64_t *count, const uint64_t *first, const uint64_t *ins_off,
                        const char *ins_text, uint32_t distance, uint64_t ratio, uint32_t *root_of_out,
                        uint32_t *order_out, uint64_t *count_out, uint64_t *first_out, dcrx_merge_stats_t *stats_out) {
  if (!tables) return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: tables is null");
  if (distance < 1 || distance > 2) return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: the distance is 1 or 2");
  if (ratio < 1) return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: the ratio is an integer >= 1");
  if (n >= (1ull << 31)) return set_err(DCRX_E_UNSUPPORTED, "dcrx_merge_dcrs: 2^31 or more entries");
  if (stats_out) { *stats_out = dcrx_merge_stats_t{}; stats_out->entries_in = n; }
  if (!n) return 0;
  if (!v || !j || !vdel || !jdel || !count || !first || !ins_off || !root_of_out || !order_out || !count_out || !first_out)
    return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: null argument");
  Entries E{};
  int rc = dcrx::merge_windows(tables, &E.rows, &E.n_v, &E.n_j);
  if (rc) return rc;
  for (uint64_t k = 0; k < n; k++) {
    if (v[k] >= E.n_v || j[k] >= E.n_j) return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: an entry names a v or j the tables do not have");
    if (ins_off[k + 1] < ins_off[k]) return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: offsets go backwards");
  }
  const uint64_t text_bytes = ins_off[n] - ins_off[0];
  if (text_bytes && !ins_text) return set_err(DCRX_E_INVALID, "dcrx_merge_dcrs: ins_text is null");
  const uint32_t n32 = (uint32_t)n;

  Pool P;
  Work W;
  uint16_t *d_v, *d_j;
  uint8_t *d_vdel, *d_jdel, *d_reach, *d_text;
  uint64_t *d_count, *d_first, *d_off;
  unsigned long long *d_tc, *d_tf, *d_stats;
  uint32_t *d_r[2], *d_d[2], *d_changed, *d_isroot, *d_slot;
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_v, n); P.get(&d_j, n); P.get(&d_vdel, n); P.get(&d_jdel, n); P.get(&d_reach, n); P.get(&d_text, text_bytes);
    P.get(&d_count, n); P.get(&d_first, n); P.get(&d_off, n + 1); P.get(&d_tc, n); P.get(&d_tf, n); P.get(&d_stats, MS_WORDS);
    P.get(&d_r[0], n); P.get(&d_r[1], n); P.get(&d_d[0], n); P.get(&d_d[1], n); P.get(&d_changed, 1);
    if ((rc = W.carve(P, n)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_table(n, v, j, vdel, jdel, count, ins_off, ins_text, d_v, d_j, d_vdel, d_jdel, d_count, d_off, d_text))) return rc;
  if ((rc = to_device(d_first, first, n))) return rc;

  E.v = d_v; E.j = d_j; E.vdel = d_vdel; E.jdel = d_jdel; E.count = d_count; E.ins_off = d_off; E.ins_text = d_text; E.text_bytes = text_bytes;
  if ((rc = run_parents(E, n, distance, ratio, d_r[0], d_reach, W, nullptr))) return rc;

  // roots: pointer jumping until no pointer moves (a round halves every entry's way to its root)
  merge_depth_init_kernel<<<grid_for(n), BLOCK>>>(d_r[0], n32, d_d[0]);
  HIP_TRY(hipGetLastError());
  int cur = 0;
  for (int round = 0; round < 40; round++) {
    uint32_t changed = 0;
    HIP_TRY(hipMemsetAsync(d_changed, 0, sizeof(uint32_t), nullptr));
    merge_jump_kernel<<<grid_for(n), BLOCK>>>(d_r[cur], d_d[cur], n32, d_r[cur ^ 1], d_d[cur ^ 1], d_changed);
    HIP_TRY(hipGetLastError());
    if ((rc = to_host(&changed, d_changed, 1))) return rc;
    if (!changed) break;                                    // (both buffers hold the same roots and depths now)
    cur ^= 1;
  }
  uint32_t *d_root = d_r[cur], *d_depth = d_d[cur];

  // totals onto the roots, and the statistics
  d_isroot = d_r[cur ^ 1];                                  // (free from here on)
  d_slot = d_d[cur ^ 1];
  HIP_TRY(hipMemcpyAsync(d_tc, d_count, n * 8, hipMemcpyDeviceToDevice, nullptr));
  HIP_TRY(hipMemcpyAsync(d_tf, d_first, n * 8, hipMemcpyDeviceToDevice, nullptr));
  HIP_TRY(hipMemsetAsync(d_stats, 0, MS_WORDS * sizeof(unsigned long long), nullptr));
  merge_totals_kernel<<<grid_for(n), BLOCK>>>(d_root, d_depth, d_reach, d_count, d_first, n32, d_tc, d_tf, d_isroot, d_stats);
  HIP_TRY(hipGetLastError());
  unsigned long long st[MS_WORDS];
  if ((rc = to_host(st, d_stats, MS_WORDS)) || (rc = to_host(root_of_out, d_root, n))) return rc;
  const uint64_t m = n - st[MS_MERGED];
  const uint32_t m32 = (uint32_t)m;

  // the roots in rank order, then by first ordinal, then (stably) by count descending; the work space is free again
  if ((rc = compact(W.cub, d_isroot, d_slot, n32, PutIndex{W.idx[0]}, nullptr, nullptr)) ||      // (their number is m)
      (rc = most_common_order(W.cub, W.idx, W.key, d_tf, 64, d_tc, m32, nullptr)) || (rc = to_host(order_out, W.idx[0], m)) ||
      (rc = gather(d_tc, W.idx[0], m32, 0, W.key[1], nullptr)) || (rc = to_host(count_out, W.key[1], m)) ||
      (rc = gather(d_tf, W.idx[0], m32, 0, W.key[1], nullptr)) || (rc = to_host(first_out, W.key[1], m))) return rc;
  if (stats_out) {
    stats_out->roots_out = m;
    stats_out->out_of_reach = st[MS_OUT_OF_REACH];
    stats_out->merged = st[MS_MERGED];
    stats_out->reads_moved = st[MS_MOVED];
    stats_out->longest_chain = st[MS_CHAIN];
  }
  return (int64_t)m;
}

int64_t dcrx_merge_gather(uint64_t n, uint64_t m, const uint32_t *order, const uint16_t *v, const uint16_t *j,
                          const uint8_t *vdel, const uint8_t *jdel, const uint64_t *ins_off, const char *ins_text,
                          uint16_t *out_v, uint16_t *out_j, uint8_t *out_vdel, uint8_t *out_jdel, uint64_t *out_ins_off,
                          char *out_ins_text) {
  if (!out_ins_off) return set_err(DCRX_E_INVALID, "dcrx_merge_gather: null argument");
  out_ins_off[0] = 0;
  if (m > n) return set_err(DCRX_E_INVALID, "dcrx_merge_gather: more roots than entries");
  if (m && (!order || !v || !j || !vdel || !jdel || !ins_off || !out_v || !out_j || !out_vdel || !out_jdel))
    return set_err(DCRX_E_INVALID, "dcrx_merge_gather: null argument");
  uint64_t at = 0;
  for (uint64_t k = 0; k < m; k++) {
    const uint64_t e = order[k];
    if (e >= n || ins_off[e + 1] < ins_off[e]) return set_err(DCRX_E_INVALID, "dcrx_merge_gather: an entry outside the table");
    out_v[k] = v[e]; out_j[k] = j[e]; out_vdel[k] = vdel[e]; out_jdel[k] = jdel[e];
    const uint64_t len = ins_off[e + 1] - ins_off[e];
    if (len) {
      if (!ins_text || !out_ins_text) return set_err(DCRX_E_INVALID, "dcrx_merge_gather: null text");
      std::memcpy(out_ins_text + at, ins_text + ins_off[e], len);
    }
    at += len;
    out_ins_off[k + 1] = at;
  }
  return (int64_t)at;
}

}  // extern "C"

// dcrx_clono.hip — the clonotype step (`translate --clonotypes`, `pipeline --clonotypes`): every counted DCR translated
// and called as dcrx_cdr3_batch calls it, the productive ones grouped by (V call group, J call group, junction_aa) and the
// groups' reads added up; include/dcrx.h holds the contract, dcrx_clono_core.h the per-entry code.
//
// The primitive (dcrx_cdr3_device), all on the caller's stream and in the caller's work space:
//   calls    clono_calls_kernel, one lane per entry: the 32-byte row, the key's hash, and the bytes its junctions take
//   scan     an exclusive sum of those lengths (hipCUB): every entry's exact offset in the arena
//   write    clono_write_kernel, one lane per entry: junction_aa, then junction, at that offset
// The gene tables are one blob in global memory, read through the caches: every lane of a wave reads the same few KB (the
// tail of its V gene, its J gene), and staging the blob in LDS per block has not been measured against that.
// The host entry (dcrx_clonotypes) adds: the members compacted in rank order, a stable radix sort of (hash, rank), the
// exact groups under the hash (dcrx_group.h's rounds, with SameKey below as the full-key test), totals onto the heads by
// integer atomics whose results are not read (add, max, then min of the rank among the members that hold the max), and
// the rows in most_common() order.
// The sorts, scans, run heads, compactions, those rounds and that order are dcrx_group.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_clono_core.h"
#include "dcrx_group.h"
#include "dcrx_text.h"

using dcrx::set_err;
using namespace dcrx_clono;
using namespace dcrx_group;

struct dcrx_clono_genes {
  std::vector<uint8_t> blob;
  Header h;
  std::vector<std::string> motifs;      // as given, for messages
  dcrx::DevBuf<uint8_t> d_blob;
  int device = -1;
  uint32_t bits = 64;
  std::vector<char> text;               // the junction text of the last dcrx_clonotypes
};

namespace {

constexpr uint64_t MAX_ENTRIES = 1ull << 30;      // (the scans over two words per row count in an int)

struct Entries {
  const int32_t *v, *j, *vdel, *jdel;
  const uint64_t *ins_off;
  const uint8_t *ins_text;
  uint64_t text_bytes;
};

__global__ __launch_bounds__(BLOCK) void clono_calls_kernel(View G, Entries E, uint32_t n, dcrx_clono_row_t *__restrict__ rows,
                                                            uint64_t *__restrict__ len) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  dcrx_clono_row_t R;
  Spans S;
  const uint64_t a = E.ins_off[e], b = E.ins_off[e + 1];
  if (b < a || b > E.text_bytes) {
    R.hash = 0; R.arena_off = 0; R.start_cdr3 = 0; R.end_cdr3 = 0; R.seq_len = 0; R.status = DCRX_CDR3_INDEX_ERROR; R.flags = 0; R.pad = 0;
    S.aa_len = S.nt_len = 0;
  } else {
    entry_calls(G, E.v[e], E.j[e], E.vdel[e], E.jdel[e], E.ins_text + a, b - a, R, S);
  }
  rows[e] = R;
  len[e] = (uint64_t)(S.aa_len + S.nt_len);
}

__device__ __forceinline__ bool is_member(const dcrx_clono_row_t &R) { return R.status == DCRX_CDR3_OK && (R.flags & F_PRODUCTIVE); }

__global__ __launch_bounds__(BLOCK) void clono_write_kernel(View G, Entries E, uint32_t n, dcrx_clono_row_t *__restrict__ rows,
                                                            const uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                            uint8_t *__restrict__ arena, uint64_t arena_cap,
                                                            uint64_t *__restrict__ need) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  const uint64_t at = off[e], bytes = len[e];
  if (e == n - 1 && need) *need = at + bytes;
  if (!is_member(rows[e])) return;
  rows[e].arena_off = at;
  if (!arena || bytes > arena_cap || at > arena_cap - bytes) return;      // (does not fit: the caller reads *need and comes back)
  const uint64_t a = E.ins_off[e];
  write_junction(G, E.v[e], E.j[e], E.vdel[e], E.jdel[e], E.ins_text + a, E.ins_off[e + 1] - a, rows[e], arena + at);
}

// ---- the host entry's kernels ----

enum { CS_PROD = 0, CS_PROD_READS, CS_NONPROD, CS_NONPROD_READS, CS_UNTRANS, CS_UNTRANS_READS, CS_READS, CS_MOTIF_LEFT, CS_WORDS };

// who is a member, and the statistics: the block's sums meet in LDS and ONE vector atomic per block (a lane per counter) adds
// them to the totals
__global__ __launch_bounds__(BLOCK) void clono_members_kernel(const dcrx_clono_row_t *__restrict__ rows,
                                                              const uint64_t *__restrict__ count, uint32_t n,
                                                              uint32_t *__restrict__ flag, unsigned long long *__restrict__ stats) {
  __shared__ unsigned long long part[BLOCK / 64 + 1][CS_WORDS];
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  unsigned long long c[CS_READS + 1] = {0, 0, 0, 0, 0, 0, 0};
  unsigned long long left = ~0ull;
  if (e < n) {
    const dcrx_clono_row_t R = rows[e];
    const unsigned long long reads = count[e];
    const bool member = is_member(R);
    flag[e] = member ? 1u : 0u;
    c[CS_READS] = reads;
    if (member) { c[CS_PROD] = 1; c[CS_PROD_READS] = reads; }
    else if (R.status == DCRX_CDR3_OK) { c[CS_NONPROD] = 1; c[CS_NONPROD_READS] = reads; }
    else if (R.status == DCRX_CDR3_MOTIF_LEFT) left = e;
    else { c[CS_UNTRANS] = 1; c[CS_UNTRANS_READS] = reads; }
  }
  const uint32_t wave = threadIdx.x / warpSize, waves = (BLOCK + warpSize - 1) / warpSize;
#pragma unroll
  for (int k = 0; k <= CS_READS; k++) {
    const unsigned long long s = wave_sum(c[k]);
    if (__lane_id() == 0) part[wave][k] = s;
  }
#pragma unroll
  for (int d = warpSize / 2; d > 0; d >>= 1) left = min(left, (unsigned long long)__shfl_down(left, d));
  if (__lane_id() == 0) part[wave][CS_MOTIF_LEFT] = left;
  __syncthreads();
  if (threadIdx.x < CS_WORDS) {
    const uint32_t k = threadIdx.x;
    unsigned long long x = part[0][k];
    for (uint32_t w = 1; w < waves; w++) x = k == CS_MOTIF_LEFT ? min(x, part[w][k]) : x + part[w][k];
    if (k != CS_MOTIF_LEFT) atomicAdd(&stats[k], x);      // (seven lanes of wave 0: the block's one atomic instruction)
    else if (x != ~0ull) atomicMin(&stats[k], x);         // (only on the way to DCRX_E_UNSUPPORTED)
  }
}

// what the compaction leaves at a slot: a member's hash and rank
struct PutMember {
  const dcrx_clono_row_t *rows;
  uint64_t mask, *key;
  uint32_t *rank;
  __device__ void operator()(uint32_t slot, uint32_t e) const { key[slot] = rows[e].hash & mask; rank[slot] = e; }
};

// the full-key test of the rounds: two members' (V call group, J call group, junction_aa)
struct SameKey {
  View G;
  Entries E;
  const dcrx_clono_row_t *rows;
  const uint8_t *arena;
  __device__ bool operator()(uint32_t ea, uint32_t eb) const {
    const dcrx_clono_row_t Ra = rows[ea], Rb = rows[eb];
    return key_equal(G, E.v[ea], E.j[ea], junction_aa_len(Ra), arena + Ra.arena_off, E.v[eb], E.j[eb], junction_aa_len(Rb),
                     arena + Rb.arena_off);
  }
};

__global__ __launch_bounds__(BLOCK) void clono_totals_kernel(const uint32_t *__restrict__ head_of, const uint32_t *__restrict__ rank,
                                                             const uint64_t *__restrict__ count, uint32_t m,
                                                             unsigned long long *__restrict__ total, uint32_t *__restrict__ members,
                                                             unsigned long long *__restrict__ top, uint32_t *__restrict__ is_head) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= m) return;
  const uint32_t h = head_of[s];
  const unsigned long long c = count[rank[s]];
  atomicAdd(&total[h], c);
  atomicAdd(&members[h], 1u);
  atomicMax(&top[h], c);
  is_head[s] = h == s ? 1u : 0u;
}

// the representative: the smallest rank among the members that hold the clonotype's largest count
__global__ __launch_bounds__(BLOCK) void clono_rep_kernel(const uint32_t *__restrict__ head_of, const uint32_t *__restrict__ rank,
                                                          const uint64_t *__restrict__ count, const unsigned long long *__restrict__ top,
                                                          uint32_t m, uint32_t *__restrict__ rep) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= m) return;
  const uint32_t h = head_of[s], e = rank[s];
  if (count[e] == top[h]) atomicMin(&rep[h], e);
}

// the rows in their final order, and where the representatives' junctions lie
__global__ __launch_bounds__(BLOCK) void clono_rows_kernel(const uint32_t *__restrict__ list, uint32_t c,
                                                           const unsigned long long *__restrict__ total, const uint32_t *__restrict__ members,
                                                           const unsigned long long *__restrict__ top, const uint32_t *__restrict__ rep,
                                                           const dcrx_clono_row_t *__restrict__ rows, uint64_t *__restrict__ dup_out,
                                                           uint32_t *__restrict__ nd_out, uint64_t *__restrict__ top_out,
                                                           uint32_t *__restrict__ rep_out, uint32_t *__restrict__ row_of_head,
                                                           uint64_t *__restrict__ junc_len) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= c) return;
  const uint32_t h = list[r], e = rep[h];
  dup_out[r] = total[h]; nd_out[r] = members[h]; top_out[r] = top[h]; rep_out[r] = e;
  row_of_head[h] = r;
  const dcrx_clono_row_t R = rows[e];
  Spans S;
  junction_spans(R.seq_len, R.start_cdr3, R.end_cdr3, S);
  junc_len[2 * (size_t)r] = (uint64_t)S.aa_len;
  junc_len[2 * (size_t)r + 1] = (uint64_t)S.nt_len;
}

__global__ __launch_bounds__(BLOCK) void clono_of_kernel(const uint32_t *__restrict__ head_of, const uint32_t *__restrict__ rank,
                                                         const uint32_t *__restrict__ row_of_head, uint32_t m,
                                                         uint32_t *__restrict__ clonotype_of) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s < m) clonotype_of[rank[s]] = row_of_head[head_of[s]];
}

__global__ __launch_bounds__(BLOCK) void clono_gather_kernel(const uint32_t *__restrict__ rep_out, const dcrx_clono_row_t *__restrict__ rows,
                                                             const uint8_t *__restrict__ arena, const uint64_t *__restrict__ junc_len,
                                                             const uint64_t *__restrict__ junc_off, uint32_t c, uint8_t *__restrict__ out) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= c) return;
  const uint64_t bytes = junc_len[2 * (size_t)r] + junc_len[2 * (size_t)r + 1];
  const uint8_t *src = arena + rows[rep_out[r]].arena_off;
  uint8_t *dst = out + junc_off[2 * (size_t)r];
  for (uint64_t i = 0; i < bytes; i++) dst[i] = src[i];
}

// ---- work space of the primitive ----
struct Work {
  uint64_t *len, *off;
  Scratch cub;
  int carve(Pool &P, uint64_t n) {
    size_t sum_bytes = 0;
    const int rc = exclusive_sum_bytes<uint64_t>(std::max<uint64_t>(n, 1), &sum_bytes);
    if (rc) return rc;
    P.get(&len, n); P.get(&off, n); P.get(&cub, sum_bytes);
    return DCRX_OK;
  }
};

int device_view(dcrx_clono_genes_t *g, View *G) {
  int dev = -1;
  HIP_TRY(hipGetDevice(&dev));
  if (g->device >= 0 && g->device != dev)
    return set_err(DCRX_E_INVALID, "the gene set lives on the device of its first use: create another handle for another device");
  if (!g->d_blob) {
    int rc;
    if ((rc = g->d_blob.alloc(g->blob.size())) || (rc = to_device(g->d_blob.get(), g->blob.data(), g->blob.size()))) return rc;
    g->device = dev;
  }
  *G = make_view(g->h, g->d_blob);
  return DCRX_OK;
}

// the lengths pass and the scan; then the write pass
int run_lengths(const View &G, const Entries &E, uint64_t n, dcrx_clono_row_t *d_rows, const Work &W, hipStream_t s) {
  clono_calls_kernel<<<grid_for(n), BLOCK, 0, s>>>(G, E, (uint32_t)n, d_rows, W.len);
  HIP_TRY(hipGetLastError());
  return exclusive_sum(W.cub, W.len, W.off, n, s);
}
int run_write(const View &G, const Entries &E, uint64_t n, dcrx_clono_row_t *d_rows, const Work &W, uint8_t *d_arena, uint64_t arena_cap,
              uint64_t *d_need, hipStream_t s) {
  clono_write_kernel<<<grid_for(n), BLOCK, 0, s>>>(G, E, (uint32_t)n, d_rows, W.len, W.off, d_arena, arena_cap, d_need);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

}  // namespace

extern "C" {

int dcrx_clono_genes_create(const dcrx_cdr3_genes_t *S, const uint32_t *v_group, const uint32_t *j_group, dcrx_clono_genes_t **out) {
  if (!S || !out) return set_err(DCRX_E_INVALID, "dcrx_clono_genes_create: null argument");
  *out = nullptr;
  if ((S->n_v && (!S->v_regions || !S->v_region_off || !S->v_pos || !S->v_res || !S->v_res_off || !v_group)) ||
      (S->n_j && (!S->j_regions || !S->j_region_off || !S->j_pos || !S->j_motif || !S->j_motif_off || !j_group)))
    return set_err(DCRX_E_INVALID, "dcrx_clono_genes_create: a gene table is null");
  try {
    auto g = new dcrx_clono_genes();
    g->blob = build_blob(*S, v_group, j_group);
    if (g->blob.empty()) { delete g; return set_err(DCRX_E_UNSUPPORTED, "dcrx_clono_genes_create: the gene tables pass 2^31 bytes"); }
    std::memcpy(&g->h, g->blob.data(), sizeof(Header));
    for (uint32_t k = 0; k < S->n_j; k++) g->motifs.emplace_back(S->j_motif + S->j_motif_off[k], S->j_motif_off[k + 1] - S->j_motif_off[k]);
    *out = g;
    return DCRX_OK;
  } catch (const std::exception &e) {
    return set_err(DCRX_E_NOMEM, e.what());
  }
}

void dcrx_clono_genes_destroy(dcrx_clono_genes_t *g) {
  if (!g) return;
  dcrx::DeviceGuard guard(g->device);
  delete g;
}

int dcrx_clono_set_hash_bits(dcrx_clono_genes_t *g, uint32_t bits) {
  if (!g) return set_err(DCRX_E_INVALID, "dcrx_clono_set_hash_bits: null handle");
  if (bits > 64) return set_err(DCRX_E_INVALID, "dcrx_clono_set_hash_bits: 0 .. 64 bits");
  g->bits = bits;
  return DCRX_OK;
}

uint64_t dcrx_clono_work_bytes(uint64_t n, uint64_t text_bytes) {
  (void)text_bytes;      // (the work space holds per-entry lengths and offsets: the inserts' bytes do not enter it)
  Pool P;
  Work W;
  if (n >= MAX_ENTRIES || W.carve(P, n) != DCRX_OK) return 0;
  return P.bytes();
}

int dcrx_cdr3_device(dcrx_clono_genes_t *g, uint64_t n, const int32_t *d_v, const int32_t *d_j, const int32_t *d_vdel,
                     const int32_t *d_jdel, const uint64_t *d_ins_off, const char *d_ins_text, uint64_t text_bytes,
                     dcrx_clono_row_t *d_rows, char *d_arena, uint64_t arena_cap, uint64_t *d_arena_need, void *d_work,
                     uint64_t work_bytes, void *hip_stream) {
  if (!g) return set_err(DCRX_E_INVALID, "dcrx_cdr3_device: the gene set is null");
  if (n >= MAX_ENTRIES) return set_err(DCRX_E_UNSUPPORTED, "dcrx_cdr3_device: 2^30 or more entries");
  hipStream_t s = (hipStream_t)hip_stream;
  if (!n) {
    if (d_arena_need) HIP_TRY(hipMemsetAsync(d_arena_need, 0, sizeof(uint64_t), s));
    return DCRX_OK;
  }
  if (!d_v || !d_j || !d_vdel || !d_jdel || !d_ins_off || !d_rows || !d_work || (text_bytes && !d_ins_text) || (arena_cap && !d_arena))
    return set_err(DCRX_E_INVALID, "dcrx_cdr3_device: null argument");
  if ((uintptr_t)d_work % ALIGN) return set_err(DCRX_E_INVALID, "dcrx_cdr3_device: the work space is not 256-byte aligned");
  Pool P(d_work);
  Work W;
  int rc = W.carve(P, n);
  if (rc) return rc;
  if (work_bytes < P.bytes()) return set_err(DCRX_E_INVALID, "dcrx_cdr3_device: the work space is smaller than dcrx_clono_work_bytes(n, text_bytes)");
  View G;
  if ((rc = device_view(g, &G))) return rc;
  const Entries E{d_v, d_j, d_vdel, d_jdel, d_ins_off, reinterpret_cast<const uint8_t *>(d_ins_text), text_bytes};
  if ((rc = run_lengths(G, E, n, d_rows, W, s))) return rc;
  return run_write(G, E, n, d_rows, W, reinterpret_cast<uint8_t *>(d_arena), arena_cap, d_arena_need, s);
}

int64_t dcrx_clonotypes(dcrx_clono_genes_t *g, uint64_t n, const int32_t *v, const int32_t *j, const int32_t *vdel,
                        const int32_t *jdel, const uint64_t *count, const uint64_t *ins_off, const char *ins_text,
                        uint32_t *rep_out, uint64_t *dup_out, uint32_t *ndcrs_out, uint64_t *top_out, uint64_t *junc_off_out,
                        uint32_t *clonotype_of_out, dcrx_clonotype_stats_t *stats_out) try {
  if (!g) return set_err(DCRX_E_INVALID, "dcrx_clonotypes: the gene set is null");
  if (n >= MAX_ENTRIES) return set_err(DCRX_E_UNSUPPORTED, "dcrx_clonotypes: 2^30 or more entries");
  if (stats_out) { *stats_out = dcrx_clonotype_stats_t{}; stats_out->entries_in = n; }
  g->text.clear();
  if (junc_off_out) junc_off_out[0] = 0;
  if (!n) return 0;
  if (!v || !j || !vdel || !jdel || !count || !ins_off || !rep_out || !dup_out || !ndcrs_out || !top_out || !junc_off_out || !clonotype_of_out)
    return set_err(DCRX_E_INVALID, "dcrx_clonotypes: null argument");
  for (uint64_t k = 0; k < n; k++)
    if (ins_off[k + 1] < ins_off[k]) return set_err(DCRX_E_INVALID, "dcrx_clonotypes: offsets go backwards");
  const uint64_t text_bytes = ins_off[n] - ins_off[0];
  if (text_bytes && !ins_text) return set_err(DCRX_E_INVALID, "dcrx_clonotypes: ins_text is null");
  const uint32_t n32 = (uint32_t)n;
  int rc;
  size_t cub_bytes = 0;
  if ((rc = sort_pairs_bytes<uint32_t>(n, 64, &cub_bytes)) || (rc = exclusive_sum_bytes<uint32_t>(n, &cub_bytes)) ||
      (rc = run_heads_bytes(n, &cub_bytes)) || (rc = exclusive_sum_bytes<uint64_t>(2 * n, &cub_bytes))) return rc;
  View G;
  if ((rc = device_view(g, &G))) return rc;

  Pool P;
  Work W;
  int32_t *d_v, *d_j, *d_vdel, *d_jdel;
  uint64_t *d_count, *d_off, *d_need, *d_key[2], *d_dup, *d_topo, *d_jlen, *d_joff;
  uint8_t *d_text, *d_cub;
  dcrx_clono_row_t *d_rows;
  unsigned long long *d_stats, *d_total, *d_top;
  uint32_t *d_flag, *d_rank[2], *d_head_of, *d_members, *d_rep, *d_ishead, *d_list[2], *d_nd, *d_repo, *d_rowof, *d_of;
  GroupWork R;      // (its slot and kept serve the other compactions too)
  for (int pass = 0; pass < 2; pass++) {
    P.get(&d_v, n); P.get(&d_j, n); P.get(&d_vdel, n); P.get(&d_jdel, n); P.get(&d_count, n); P.get(&d_off, n + 1);
    P.get(&d_text, text_bytes); P.get(&d_rows, n); P.get(&d_need, 1); P.get(&d_stats, CS_WORDS);
    P.get(&d_cub, cub_bytes); P.get(&d_flag, n); P.get(&d_key[0], n); P.get(&d_key[1], n); P.get(&d_rank[0], n);
    P.get(&d_rank[1], n); R.get(P, n); P.get(&d_head_of, n); P.get(&d_total, n); P.get(&d_members, n); P.get(&d_top, n);
    P.get(&d_rep, n); P.get(&d_ishead, n); P.get(&d_list[0], n); P.get(&d_list[1], n); P.get(&d_dup, n); P.get(&d_topo, n);
    P.get(&d_nd, n); P.get(&d_repo, n); P.get(&d_rowof, n); P.get(&d_of, n); P.get(&d_jlen, 2 * n); P.get(&d_joff, 2 * n);
    if ((rc = W.carve(P, n)) || (pass == 0 && (rc = P.allocate()))) return rc;
  }
  if ((rc = upload_table(n, v, j, vdel, jdel, count, ins_off, ins_text, d_v, d_j, d_vdel, d_jdel, d_count, d_off, d_text))) return rc;
  const Entries E{d_v, d_j, d_vdel, d_jdel, d_off, d_text, text_bytes};

  // the calls, then an arena of exactly the bytes the junctions take
  if ((rc = run_lengths(G, E, n, d_rows, W, nullptr))) return rc;
  if ((rc = run_write(G, E, n, d_rows, W, nullptr, 0, d_need, nullptr))) return rc;
  uint64_t need = 0;
  if ((rc = to_host(&need, d_need, 1))) return rc;
  dcrx::DevBuf<uint8_t> d_arena;
  if ((rc = d_arena.alloc(std::max<uint64_t>(need, 1)))) return rc;
  if ((rc = run_write(G, E, n, d_rows, W, d_arena, need, nullptr, nullptr))) return rc;

  // members and statistics
  unsigned long long st[CS_WORDS];
  std::memset(st, 0, sizeof st);
  st[CS_MOTIF_LEFT] = ~0ull;
  if ((rc = to_device(d_stats, st, CS_WORDS))) return rc;
  clono_members_kernel<<<grid_for(n), BLOCK>>>(d_rows, d_count, n32, d_flag, d_stats);
  HIP_TRY(hipGetLastError());
  if ((rc = to_host(st, d_stats, CS_WORDS))) return rc;
  if (st[CS_MOTIF_LEFT] != ~0ull) {
    const uint64_t e = st[CS_MOTIF_LEFT];
    const int64_t ji = j[e] < 0 ? (int64_t)j[e] + g->h.n_j : (int64_t)j[e];
    const std::string m = "dcrx_clonotypes: entry " + std::to_string(e) + " uses J gene " + std::to_string(ji) + ", whose motif '" +
                          g->motifs[(size_t)ji] + "' needs a regular-expression engine (literals, '.', character classes and escaped "
                          "literals are served); there is no CPU fallback";
    return set_err(DCRX_E_UNSUPPORTED, m.c_str());
  }
  if (stats_out) {
    stats_out->reads_in = st[CS_READS];
    stats_out->productive = st[CS_PROD]; stats_out->productive_reads = st[CS_PROD_READS];
    stats_out->nonproductive = st[CS_NONPROD]; stats_out->nonproductive_reads = st[CS_NONPROD_READS];
    stats_out->untranslatable = st[CS_UNTRANS]; stats_out->untranslatable_reads = st[CS_UNTRANS_READS];
  }
  std::memset(clonotype_of_out, 0xFF, n * 4);
  const uint64_t m = st[CS_PROD];
  if (!m) return 0;
  const uint32_t m32 = (uint32_t)m;

  // the members in rank order, sorted (stably) by hash; then the rounds: head_of
  const Scratch cub{d_cub, cub_bytes};
  if ((rc = compact(cub, d_flag, R.slot, n32, PutMember{d_rows, low_bits(g->bits), d_key[0], d_rank[0]}, nullptr, nullptr)) ||      // (their number is m)
      (rc = sort_pairs(cub, d_key[0], d_key[1], d_rank[0], d_rank[1], m, 64, nullptr))) return rc;
  const uint32_t *d_sorted = d_rank[1];
  if ((rc = exact_groups(cub, d_key[1], d_sorted, m32, SameKey{G, E, d_rows, d_arena}, R, d_head_of,
                         "dcrx_clonotypes: a round resolved nothing", nullptr))) return rc;

  // totals onto the heads, the representatives
  HIP_TRY(hipMemsetAsync(d_total, 0, m * 8, nullptr));
  HIP_TRY(hipMemsetAsync(d_members, 0, m * 4, nullptr));
  HIP_TRY(hipMemsetAsync(d_top, 0, m * 8, nullptr));
  HIP_TRY(hipMemsetAsync(d_rep, 0xFF, m * 4, nullptr));
  clono_totals_kernel<<<grid_for(m), BLOCK>>>(d_head_of, d_sorted, d_count, m32, d_total, d_members, d_top, d_ishead);
  HIP_TRY(hipGetLastError());
  clono_rep_kernel<<<grid_for(m), BLOCK>>>(d_head_of, d_sorted, d_count, d_top, m32, d_rep);
  HIP_TRY(hipGetLastError());
  if ((rc = compact(cub, d_ishead, R.slot, m32, PutIndex{d_list[0]}, R.kept, nullptr))) return rc;
  uint32_t c = 0;
  if ((rc = to_host(&c, R.kept, 1))) return rc;

  // order: by the representative's rank, then (stably) by duplicate_count descending
  if ((rc = most_common_order(cub, d_list, d_key, d_rep, 32, d_total, c, nullptr))) return rc;
  clono_rows_kernel<<<grid_for(c), BLOCK>>>(d_list[0], c, d_total, d_members, d_top, d_rep, d_rows, d_dup, d_nd, d_topo, d_repo, d_rowof, d_jlen);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(d_of, 0xFF, n * 4, nullptr));
  clono_of_kernel<<<grid_for(m), BLOCK>>>(d_head_of, d_sorted, d_rowof, m32, d_of);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_sum(cub, d_jlen, d_joff, 2 * (uint64_t)c, nullptr))) return rc;
  uint64_t last_len = 0;
  if ((rc = to_host(junc_off_out, d_joff, 2 * (uint64_t)c)) || (rc = to_host(&last_len, d_jlen + (2 * (uint64_t)c - 1), 1))) return rc;
  const uint64_t out_bytes = junc_off_out[2 * (uint64_t)c - 1] + last_len;
  junc_off_out[2 * (uint64_t)c] = out_bytes;
  dcrx::DevBuf<uint8_t> d_out;
  if ((rc = d_out.alloc(std::max<uint64_t>(out_bytes, 1)))) return rc;
  clono_gather_kernel<<<grid_for(c), BLOCK>>>(d_repo, d_rows, d_arena, d_jlen, d_joff, c, d_out);
  HIP_TRY(hipGetLastError());
  g->text.resize(out_bytes);
  if ((rc = to_host(reinterpret_cast<uint8_t *>(g->text.data()), d_out.get(), out_bytes)) || (rc = to_host(rep_out, d_repo, c)) ||
      (rc = to_host(dup_out, d_dup, c)) || (rc = to_host(ndcrs_out, d_nd, c)) || (rc = to_host(top_out, d_topo, c)) ||
      (rc = to_host(clonotype_of_out, d_of, n))) return rc;
  if (stats_out) {
    stats_out->clonotypes_out = c;
    for (uint32_t r = 0; r < c; r++) {
      if (ndcrs_out[r] > 1) stats_out->convergent++;
      stats_out->largest_n_dcrs = std::max<uint64_t>(stats_out->largest_n_dcrs, ndcrs_out[r]);
    }
  }
  return (int64_t)c;
} catch (const std::exception &e) {      // (the entry's one guard: the junction text, a message)
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t dcrx_clonotypes_text(dcrx_clono_genes_t *g, char *out, uint64_t cap) {
  if (!g) return set_err(DCRX_E_INVALID, "dcrx_clonotypes_text: null handle");
  if (out && cap >= g->text.size() && !g->text.empty()) std::memcpy(out, g->text.data(), g->text.size());
  return (int64_t)g->text.size();
}

int64_t dcrx_format_clonotypes(uint64_t m, const uint32_t *rep, const uint64_t *dup, const uint32_t *ndcrs, const uint64_t *top,
                               const uint64_t *junc_off, const char *junc_text, uint64_t n, const int32_t *v, const int32_t *j,
                               const int32_t *vdel, const int32_t *jdel, const uint64_t *ins_off, const char *ins_text,
                               uint32_t n_v, const char *v_calls, const uint32_t *v_call_off, uint32_t n_j, const char *j_calls,
                               const uint32_t *j_call_off, char *out, uint64_t out_cap) {
  static const char header[] = "v_call\tj_call\tjunction_aa\tduplicate_count\tn_dcrs\tjunction\tdecombinator_id\ttop_dcr_count\n";
  if (m && (!rep || !dup || !ndcrs || !top || !junc_off || !v || !j || !vdel || !jdel || !ins_off || !v_call_off || !j_call_off))
    return set_err(DCRX_E_INVALID, "dcrx_format_clonotypes: null argument");
  dcrx::TextOut T{out, out_cap};
  T.put(header, sizeof header - 1);
  for (uint64_t r = 0; r < m; r++) {
    const uint64_t e = rep[r];
    if (e >= n) return set_err(DCRX_E_INVALID, "dcrx_format_clonotypes: a representative outside the table");
    const int64_t vi = v[e] < 0 ? (int64_t)v[e] + n_v : (int64_t)v[e], ji = j[e] < 0 ? (int64_t)j[e] + n_j : (int64_t)j[e];
    if (vi < 0 || vi >= (int64_t)n_v || ji < 0 || ji >= (int64_t)n_j) return set_err(DCRX_E_INVALID, "dcrx_format_clonotypes: a gene outside its table");
    T.put_span(v_calls, v_call_off, vi); T.put("\t", 1);
    T.put_span(j_calls, j_call_off, ji); T.put("\t", 1);
    T.put_span(junc_text, junc_off, 2 * r); T.put("\t", 1);
    T.unum(dup[r]); T.put("\t", 1);
    T.unum(ndcrs[r]); T.put("\t", 1);
    T.put_span(junc_text, junc_off, 2 * r + 1); T.put("\t", 1);
    T.num(v[e]); T.put(", ", 2); T.num(j[e]); T.put(", ", 2); T.num(vdel[e]); T.put(", ", 2); T.num(jdel[e]); T.put(", ", 2);
    T.put_span(ins_text, ins_off, e); T.put("\t", 1);
    T.unum(top[r]); T.put("\n", 1);
  }
  return (int64_t)T.at;
}

}  // extern "C"

// dcrx_components.h — the connected components of a graph on n nodes held on the device, written once for the CDR3 network
// (dcrx_cdr3net.hip: the edges are an adjacency in CSR) and the motif groups (dcrx_motif.hip: an adjacency, possibly empty,
// and ROWS — lists of nodes of which any two are linked, in CSR too, possibly empty).
// Rounds of "the smallest label among my neighbours, my rows and me" and pointer jumping, double buffered, until a round moves
// nothing; then the totals (integer atomics onto the heads, results unused) and the heads compacted in node order, so that
// components are numbered by their smallest node.  A label is a node's index and never rises, and a node's label is never above
// the node: the fixed point is every component's smallest node, whatever the order in which the atomics arrive.
// A round:
//   rows   comp_row_min_kernel, a lane per posting (a node in a row): the smallest label of a row's nodes onto row_label[row].
//          Postings lie in (row, node) order, so consecutive lanes share a row: a segmented minimum over the wave's lanes, one
//          atomic per row and wave (WAVE_MIN; without it one atomic per posting)
//   nodes  comp_min_kernel, a lane per node: the smallest among itself and its adjacency; then comp_row_take_kernel, a lane per
//          posting: the row's label onto the node (atomic minimum, result unused)
//   jump   comp_jump_kernel, a lane per node: the label followed to where it ends
// A round synchronises once: the 4 bytes that say whether something moved, by a blocking copy on the stream.
// Private to those translation units (HIP only); everything has internal linkage, as dcrx_group.h's has.
#pragma once

#include "dcrx_group.h"

namespace dcrx_components {
namespace {

using dcrx_group::BLOCK;
using dcrx_group::grid_for;

#ifdef DCRX_COMPONENTS_PLAIN_ROW_MIN      // (a build for measuring what the wave's reduction is worth: DESIGN.md 7l)
constexpr bool WAVE_MIN = false;
#else
constexpr bool WAVE_MIN = true;
#endif
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

__global__ __launch_bounds__(BLOCK) void comp_label_init_kernel(uint32_t n, uint32_t *__restrict__ label) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) label[i] = i;
}

// a round's first half: the smallest label among a node's neighbours and itself
__global__ __launch_bounds__(BLOCK) void comp_min_kernel(const uint32_t *__restrict__ in, const uint64_t *__restrict__ adj_off,
                                                         const uint32_t *__restrict__ adj, uint32_t n, uint32_t *__restrict__ out,
                                                         uint32_t *__restrict__ changed) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  bool moved = false;
  if (i < n) {
    const uint32_t mine = in[i];
    uint32_t l = mine;
    for (uint64_t k = adj_off[i], end = adj_off[i + 1]; k < end; k++) l = min(l, in[adj[k]]);
    out[i] = l;
    moved = l != mine;
  }
  if (__ballot(moved) && __lane_id() == 0) *changed = 1u;
}

// ... and its second: every label followed to where it ends (a label is a node not above its node: the chain falls)
__global__ __launch_bounds__(BLOCK) void comp_jump_kernel(const uint32_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t l = in[i];
  for (uint32_t next = in[l]; next != l; next = in[l]) l = next;
  out[i] = l;
}

// ---- rows
struct Rows {
  const uint64_t *off;      // rows + 1 offsets into node
  const uint32_t *node;     // the postings, in (row, node) order
  uint32_t rows;
  uint64_t postings;        // off[rows], as the host knows it
  uint32_t *row_label;      // rows words of work space
};

// the row of posting p: the last row whose offset is not above p (rows that hold nothing are stepped over)
__device__ __forceinline__ uint32_t row_of_posting(const uint64_t *__restrict__ off, uint32_t rows, uint64_t p) {
  uint32_t lo = 0, hi = rows;      // off[lo] <= p < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// every row takes the smallest label among its nodes
__global__ __launch_bounds__(BLOCK) void comp_row_min_kernel(const uint32_t *__restrict__ in, Rows R, uint32_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  uint32_t row = NO_ROW, l = NO_ROW;
  if (p < R.postings) {
    const uint32_t node = R.node[p];
    if (node < n) { row = row_of_posting(R.off, R.rows, p); l = in[node]; }
  }
  if (!WAVE_MIN) {
    if (row != NO_ROW) atomicMin(&R.row_label[row], l);
    return;
  }
  // a segmented minimum: the rows of a wave's lanes do not fall, so a lane folds in the lanes above it while they hold its row
  const uint32_t lane = __lane_id();
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t other = __shfl_down(l, d), other_row = __shfl_down(row, d);
    if (lane + d < 64 && other_row == row) l = min(l, other);
  }
  const uint32_t before = __shfl_up(row, 1);
  if (row != NO_ROW && (lane == 0 || before != row)) atomicMin(&R.row_label[row], l);
}

// ... and every node the smallest among what it holds and its rows (`before`: the labels the round began with)
__global__ __launch_bounds__(BLOCK) void comp_row_take_kernel(const uint32_t *__restrict__ before, Rows R, uint32_t n,
                                                              uint32_t *__restrict__ out, uint32_t *__restrict__ changed) {
  const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool moved = false;
  if (p < R.postings) {
    const uint32_t node = R.node[p];
    if (node < n) {
      const uint32_t l = R.row_label[row_of_posting(R.off, R.rows, p)];
      moved = l < before[node];
      if (moved) atomicMin(&out[node], l);
    }
  }
  if (__ballot(moved) && __lane_id() == 0) *changed = 1u;
}

// The rounds.  label[0] ends as every node's component's smallest node; label[1] and changed (one word) are work space.
// any_adj: whether the adjacency holds an entry (false: adj may be null; adj_off is read all the same).  R may be null.
// *rounds (may be null): the rounds run, the last one, which moves nothing, included.
inline int components(uint32_t n, const uint64_t *adj_off, const uint32_t *adj, bool any_adj, const Rows *R, uint32_t *const label[2],
                      uint32_t *d_changed, uint32_t *rounds, hipStream_t s) {
  if (rounds) *rounds = 0;
  if (!n) return DCRX_OK;
  comp_label_init_kernel<<<grid_for(n), BLOCK, 0, s>>>(n, label[0]);
  HIP_TRY(hipGetLastError());
  const bool rows = R && R->rows && R->postings;
  for (uint32_t changed = any_adj || rows ? 1u : 0u; changed;) {
    HIP_TRY(hipMemsetAsync(d_changed, 0, 4, s));
    if (rows) {
      HIP_TRY(hipMemsetAsync(R->row_label, 0xFF, (uint64_t)R->rows * 4, s));
      comp_row_min_kernel<<<grid_for(R->postings), BLOCK, 0, s>>>(label[0], *R, n);
      HIP_TRY(hipGetLastError());
    }
    comp_min_kernel<<<grid_for(n), BLOCK, 0, s>>>(label[0], adj_off, adj, n, label[1], d_changed);
    HIP_TRY(hipGetLastError());
    if (rows) {
      comp_row_take_kernel<<<grid_for(R->postings), BLOCK, 0, s>>>(label[0], *R, n, label[1], d_changed);
      HIP_TRY(hipGetLastError());
    }
    comp_jump_kernel<<<grid_for(n), BLOCK, 0, s>>>(label[1], n, label[0]);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyWithStream(&changed, d_changed, 4, hipMemcpyDeviceToHost, s));      // (blocking: the round's one synchronisation)
    if (rounds) ++*rounds;
  }
  return DCRX_OK;
}

// ---- totals: onto the heads; the heads in node order are the component rows
__global__ __launch_bounds__(BLOCK) void comp_totals_kernel(const uint32_t *__restrict__ label, const uint64_t *__restrict__ weight,
                                                            uint32_t n, unsigned long long *__restrict__ total,
                                                            uint32_t *__restrict__ members, uint32_t *__restrict__ is_head) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = label[i];
  atomicAdd(&total[h], (unsigned long long)weight[i]);
  atomicAdd(&members[h], 1u);
  is_head[i] = h == i ? 1u : 0u;
}

__global__ __launch_bounds__(BLOCK) void comp_rows_kernel(const uint32_t *__restrict__ heads, const uint32_t *__restrict__ kept,
                                                          const unsigned long long *__restrict__ total,
                                                          const uint32_t *__restrict__ members, uint32_t *__restrict__ nn_out,
                                                          uint64_t *__restrict__ w_out) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= *kept) return;
  const uint32_t h = heads[r];
  nn_out[r] = members[h];
  w_out[r] = total[h];
}

__global__ __launch_bounds__(BLOCK) void comp_of_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ slot,
                                                        uint32_t n, uint32_t *__restrict__ of) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) of[i] = slot[label[i]];
}

// what the totals take of a work space (n entries each, kept one; cub: dcrx_group's exclusive_sum_bytes<uint32_t>(n))
struct TotalsWork {
  unsigned long long *total;
  uint32_t *members, *is_head, *slot, *kept;
  dcrx_group::Scratch cub;
  int carve(dcrx_group::Pool &P, uint64_t n) {
    size_t b = 0;
    const int rc = dcrx_group::exclusive_sum_bytes<uint32_t>(std::max<uint64_t>(n, 1), &b);
    if (rc) return rc;
    P.get(&total, n); P.get(&members, n); P.get(&is_head, n); P.get(&slot, n); P.get(&kept, 1); P.get(&cub, b);
    return DCRX_OK;
  }
};

// from the labels: per node its component's row (of), per row its head, its nodes and its weight (n entries of room each);
// W.kept ends as the number of rows.  Nothing waits.
inline int totals(uint32_t n, const uint32_t *label, const uint64_t *weight, const TotalsWork &W, uint32_t *of, uint32_t *heads,
                  uint32_t *nn_out, uint64_t *w_out, hipStream_t s) {
  if (!n) {
    HIP_TRY(hipMemsetAsync(W.kept, 0, 4, s));
    return DCRX_OK;
  }
  HIP_TRY(hipMemsetAsync(W.total, 0, (uint64_t)n * 8, s));
  HIP_TRY(hipMemsetAsync(W.members, 0, (uint64_t)n * 4, s));
  comp_totals_kernel<<<grid_for(n), BLOCK, 0, s>>>(label, weight, n, W.total, W.members, W.is_head);
  HIP_TRY(hipGetLastError());
  const int rc = dcrx_group::compact(W.cub, W.is_head, W.slot, n, dcrx_group::PutIndex{heads}, W.kept, s);
  if (rc) return rc;
  comp_rows_kernel<<<grid_for(n), BLOCK, 0, s>>>(heads, W.kept, W.total, W.members, nn_out, w_out);
  HIP_TRY(hipGetLastError());
  comp_of_kernel<<<grid_for(n), BLOCK, 0, s>>>(label, W.slot, n, of);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

}  // namespace
}  // namespace dcrx_components

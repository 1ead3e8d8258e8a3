// dcrx_group.h — what the count (dcrx_count.hip), the error merge (dcrx_merge.hip), the clonotype step (dcrx_clono.hip), the
// CDR3 network (dcrx_cdr3net.hip), the overlap step (dcrx_overlap.hip) and the downsampling step (dcrx_rarefy.hip) share to
// group, compact and order a table on the device, each written once: the launch geometry, the 64-bit wave sum, the pool
// that carves a work space, the typed blocking copies, hipCUB's four calls with their scratch, run heads, the ordered
// compaction, cells (the sums of runs of one key), exact groups under a hash (the rounds of the clonotype and overlap steps),
// the most_common() order and the upload of offsets with their text and of a counted table.
// Private to those translation units (HIP only, as dcrx_hip.h).
// Nothing here allocates behind the caller's back (Pool::allocate is the caller's one allocation), and nothing synchronises
// but exact_groups, once per round, and to_device, to_host and the uploads, which are blocking copies; every launch and
// hipCUB call goes to the stream it is handed.  Everything has internal linkage, as the kernels of those units have: a unit's
// instances of the templated kernels are its own.
#pragma once

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <exception>
#include <vector>

#include "dcrx_hip.h"

namespace dcrx_group {
namespace {

constexpr int BLOCK = 256;
constexpr uint64_t ALIGN = 256;

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }
inline uint64_t aligned(uint64_t bytes) { return (bytes + ALIGN - 1) & ~(ALIGN - 1); }
inline uint64_t low_bits(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }      // the mask of a hash cut to `bits`

// the wave's sum, in lane 0
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int d = warpSize / 2; d > 0; d >>= 1) x += __shfl_down(x, d);
  return x;
}

// hipCUB's scratch: a call takes it BY VALUE, as hipCUB overwrites the size it is handed
struct Scratch {
  void *p;
  size_t bytes;
};

// A work space carved into 256-byte aligned buffers.  One list of typed requests serves three ways: over no memory it adds
// up the size (bytes()); over memory of the caller's (a device entry's d_work) it hands out the pointers; and a host entry
// runs it twice, the second time over its ONE allocation of what the first added up (allocate()).
struct Pool {
  Pool() = default;
  explicit Pool(void *mem) : base(static_cast<uint8_t *>(mem)) {}
  template <class T> void get(T **p, uint64_t count) {
    *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += aligned(std::max<uint64_t>(count, 1) * sizeof(T));
  }
  void get(Scratch *t, size_t bytes) {
    uint8_t *p;
    get(&p, bytes);
    *t = Scratch{p, bytes};
  }
  uint64_t bytes() const { return at; }      // asked for so far
  int allocate() {
    const int rc = own.alloc(std::max<uint64_t>(at, 1));
    base = own;
    at = 0;
    return rc;
  }

 private:
  dcrx::DevBuf<uint8_t> own;
  uint8_t *base = nullptr;
  uint64_t at = 0;
};

// ---- blocking copies of n elements (none: nothing is copied)
template <class T> int to_device(T *d, const T *h, uint64_t n) {
  if (n) HIP_TRY(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
  return DCRX_OK;
}
template <class T> int to_host(T *h, const T *d, uint64_t n) {
  if (n) HIP_TRY(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
  return DCRX_OK;
}

// ---- hipCUB: the four calls in use.  A *_bytes query folds the scratch a call over n items wants into `most` (a carve
// asks for every call it will make and holds the largest).  Sorts are stable and ascending over the key's bits
// [begin_bit, end_bit), begin_bit 0 unless given; results are in *_out.
// (The scans hand hipCUB plain pointers for input too: it makes its kernels per iterator type, and one set is enough.)

template <class V> int sort_pairs_bytes(uint64_t n, int end_bit, size_t *most) {
  size_t b = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (V *)nullptr, (V *)nullptr, (int)n, 0, end_bit));
  *most = std::max(*most, b);
  return DCRX_OK;
}
template <class V> int sort_pairs(Scratch t, const uint64_t *key_in, uint64_t *key_out, const V *val_in, V *val_out, uint64_t n,
                                  int end_bit, hipStream_t s, int begin_bit = 0) {
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(t.p, t.bytes, key_in, key_out, val_in, val_out, (int)n, begin_bit, end_bit, s));
  return DCRX_OK;
}

template <class T> int exclusive_sum_bytes(uint64_t n, size_t *most) {
  size_t b = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (T *)nullptr, (T *)nullptr, (int)n));
  *most = std::max(*most, b);
  return DCRX_OK;
}
template <class T> int exclusive_sum(Scratch t, const T *in, T *out, uint64_t n, hipStream_t s) {
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(t.p, t.bytes, const_cast<T *>(in), out, (int)n, s));
  return DCRX_OK;
}

// ---- run heads: over keys in sorted order, mark[i] = run_mark(i, key) and a max scan of the marks (run_heads) gives every
// position the position where its run of equal keys starts.  key_at(i) is the key at position i.
template <class I, class KeyAt> __device__ __forceinline__ uint32_t run_mark(I i, KeyAt key_at) {
  return (i == 0 || key_at(i) != key_at(i - 1)) ? (uint32_t)i : 0u;
}
inline int run_heads_bytes(uint64_t n, size_t *most) {
  size_t b = 0;
  HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, hipcub::Max(), (int)n));
  *most = std::max(*most, b);
  return DCRX_OK;
}
inline int run_heads(Scratch t, const uint32_t *mark, uint32_t *head_of, uint64_t n, hipStream_t s) {
  HIP_TRY(hipcub::DeviceScan::InclusiveScan(t.p, t.bytes, const_cast<uint32_t *>(mark), head_of, hipcub::Max(), (int)n, s));
  return DCRX_OK;
}

// ---- ordered compaction: the flagged positions of 0 .. n-1 (flags 0 or 1) keep their order.  put(slot, i) writes what
// position i leaves at its slot; *kept is their number (kept may be null where the caller knows it).
template <class Put> __global__ __launch_bounds__(BLOCK) void compact_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ slot,
                                                                             uint32_t n, Put put, uint32_t *__restrict__ kept) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) put(slot[i], i);
  if (kept && i == n - 1) *kept = slot[i] + flag[i];
}
template <class Put> int compact(Scratch t, const uint32_t *flag, uint32_t *slot, uint32_t n, Put put, uint32_t *d_kept, hipStream_t s) {
  if (!n) {      // (nothing to launch; nothing is kept)
    if (d_kept) HIP_TRY(hipMemsetAsync(d_kept, 0, sizeof(uint32_t), s));
    return DCRX_OK;
  }
  const int rc = exclusive_sum(t, flag, slot, n, s);
  if (rc) return rc;
  compact_kernel<<<grid_for(n), BLOCK, 0, s>>>(flag, slot, n, put, d_kept);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}
struct PutIndex {      // the position itself
  uint32_t *list;
  __device__ void operator()(uint32_t slot, uint32_t i) const { list[slot] = i; }
};

// ---- cells: a cell is a run of equal 64-bit keys in sorted order, its members' weights summed onto the run's first position
__global__ __launch_bounds__(BLOCK) void run_marks_kernel(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ mark) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s < n) mark[s] = run_mark(s, [&](uint32_t k) { return key[k]; });
}
inline int run_marks(const uint64_t *key, uint32_t n, uint32_t *mark, hipStream_t s) {
  run_marks_kernel<<<grid_for(n), BLOCK, 0, s>>>(key, n, mark);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// every position's weight onto its cell's first position (64-bit atomics whose results are not read)
__global__ __launch_bounds__(BLOCK) void cell_sums_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ idx,
                                                          const uint64_t *__restrict__ weight, uint32_t n,
                                                          unsigned long long *__restrict__ sum, uint32_t *__restrict__ is_head) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= n) return;
  const uint32_t h = head[s];
  atomicAdd(&sum[h], (unsigned long long)weight[idx[s]]);
  is_head[s] = h == s ? 1u : 0u;
}

// over n >= 1 sorted keys, idx[s] the source position of sorted position s: head[s] is where the cell of s starts,
// sum[head] the cell's weight[idx[.]] added up (zero elsewhere), is_head[s] whether s starts a cell; mark is overwritten
inline int cell_sums(Scratch t, const uint64_t *key, const uint32_t *idx, const uint64_t *weight, uint32_t n, uint32_t *mark,
                     uint32_t *head, unsigned long long *sum, uint32_t *is_head, hipStream_t s) {
  int rc;
  if ((rc = run_marks(key, n, mark, s)) || (rc = run_heads(t, mark, head, n, s))) return rc;
  HIP_TRY(hipMemsetAsync(sum, 0, (uint64_t)n * sizeof *sum, s));
  cell_sums_kernel<<<grid_for(n), BLOCK, 0, s>>>(head, idx, weight, n, sum, is_head);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}

// ---- exact groups under a hash.  The rows come sorted stably by hash: key[s] is the hash at sorted position s, rank[s] the
// row there, so a run of one hash is in rank order.  Rounds: every active position is compared in full, by same(rank, rank),
// with the first active position of its run; what differs stays active, and the first of what stays in a run is the next
// round's head.  head_of[s] ends as the sorted position of the first row whose full key equals that of position s.
// A round synchronises once: the 4 bytes that say how many positions stay, by a blocking copy on the stream (an asynchronous
// copy and a stream wait in its place measured 1 ms slower per call).  `stalled` is the caller's message for a
// round that resolved nothing (the first active position of every run always resolves).
// The work buffers, over n >= m positions; between calls they are the caller's to use.
struct GroupWork {
  uint32_t *run, *mark, *first, *active[2], *keep, *slot, *kept;
  void get(Pool &P, uint64_t n) {
    P.get(&run, n); P.get(&mark, n); P.get(&first, n); P.get(&active[0], n); P.get(&active[1], n); P.get(&keep, n); P.get(&slot, n);
    P.get(&kept, 1);
  }
};

__global__ __launch_bounds__(BLOCK) void group_runs_kernel(const uint64_t *__restrict__ key, uint32_t m, uint32_t *__restrict__ mark,
                                                           uint32_t *__restrict__ active) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= m) return;
  mark[s] = run_mark(s, [&](uint32_t k) { return key[k]; });
  active[s] = s;
}

// a round: the first active position of every run (active: the active positions in sorted order, run: a position's run)
__global__ __launch_bounds__(BLOCK) void group_round_mark_kernel(const uint32_t *__restrict__ active, const uint32_t *__restrict__ run,
                                                                 uint32_t a, uint32_t *__restrict__ mark) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a) return;
  mark[i] = run_mark(i, [&](uint32_t k) { return run[active[k]]; });
}

// ... and every other active position against it, in full
template <class Same>
__global__ __launch_bounds__(BLOCK) void group_round_compare_kernel(Same same, const uint32_t *__restrict__ rank,
                                                                    const uint32_t *__restrict__ active, const uint32_t *__restrict__ first,
                                                                    uint32_t a, uint32_t *__restrict__ head_of, uint32_t *__restrict__ keep) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a) return;
  const uint32_t p = active[i], h = active[first[i]];
  const bool eq = p == h || same(rank[p], rank[h]);
  if (eq) head_of[p] = h;
  keep[i] = eq ? 0u : 1u;
}

struct PutActive {      // an active position of the last round
  const uint32_t *src;
  uint32_t *dst;
  __device__ void operator()(uint32_t slot, uint32_t i) const { dst[slot] = src[i]; }
};

template <class Same> int exact_groups(Scratch t, const uint64_t *key, const uint32_t *rank, uint32_t m, Same same, const GroupWork &W,
                                       uint32_t *head_of, const char *stalled, hipStream_t s) {
  if (!m) return DCRX_OK;
  int rc;
  group_runs_kernel<<<grid_for(m), BLOCK, 0, s>>>(key, m, W.mark, W.active[0]);
  HIP_TRY(hipGetLastError());
  if ((rc = run_heads(t, W.mark, W.run, m, s))) return rc;
  int cur = 0;
  for (uint32_t a = m, left = 0; a; a = left, cur ^= 1) {
    group_round_mark_kernel<<<grid_for(a), BLOCK, 0, s>>>(W.active[cur], W.run, a, W.mark);
    HIP_TRY(hipGetLastError());
    if ((rc = run_heads(t, W.mark, W.first, a, s))) return rc;
    group_round_compare_kernel<<<grid_for(a), BLOCK, 0, s>>>(same, rank, W.active[cur], W.first, a, head_of, W.keep);
    HIP_TRY(hipGetLastError());
    if ((rc = compact(t, W.keep, W.slot, a, PutActive{W.active[cur], W.active[cur ^ 1]}, W.kept, s))) return rc;
    HIP_TRY(hipMemcpyWithStream(&left, W.kept, 4, hipMemcpyDeviceToHost, s));      // (blocking: the round's one synchronisation)
    if (left >= a) return dcrx::set_err(DCRX_E_HIP, stalled);
  }
  return DCRX_OK;
}

// ---- collections.Counter.most_common() order
// dst[k] = src[list[k]] as 64 bits, or its complement (an ascending sort of the complements is a descending one)
template <class S, class L> __global__ __launch_bounds__(BLOCK) void gather_kernel(const S *__restrict__ src, const L *__restrict__ list, uint32_t m,
                                                                                   int negate, uint64_t *__restrict__ dst) {
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= m) return;
  const uint64_t x = src[list[k]];
  dst[k] = negate ? ~x : x;
}
template <class S, class L> int gather(const S *src, const L *list, uint32_t m, int negate, uint64_t *dst, hipStream_t s) {
  if (!m) return DCRX_OK;
  gather_kernel<<<grid_for(m), BLOCK, 0, s>>>(src, list, m, negate, dst);
  HIP_TRY(hipGetLastError());
  return DCRX_OK;
}
// list[0] (m indices) ordered by count[.] descending, ties by tie[.] ascending (tie_bits of it count): a stable sort
// by the tie key (into list[1]), then one by the complemented count (back into list[0]).  key[0], key[1] are overwritten.
template <class L, class T, class C> int most_common_order(Scratch t, L *const list[2], uint64_t *const key[2], const T *tie, int tie_bits,
                                                           const C *count, uint32_t m, hipStream_t s) {
  if (!m) return DCRX_OK;
  int rc;
  if ((rc = gather(tie, list[0], m, 0, key[0], s)) || (rc = sort_pairs(t, key[0], key[1], list[0], list[1], m, tie_bits, s)) ||
      (rc = gather(count, list[1], m, 1, key[0], s)) || (rc = sort_pairs(t, key[0], key[1], list[1], list[0], m, 64, s))) return rc;
  return DCRX_OK;
}

// ---- from the host (blocking copies): the offsets off[0 .. n] rebased to off[0] and the text they span; DCRX_E_NOMEM,
// not an exception, where the host has no room for the rebased offsets
inline int upload_spans(uint64_t n, const uint64_t *off, const char *text, uint64_t *d_off, uint8_t *d_text) {
  const uint64_t text0 = off[0], text_bytes = off[n] - text0;
  std::vector<uint64_t> rebased;
  try {
    rebased.resize(n + 1);
  } catch (const std::exception &e) {
    return dcrx::set_err(DCRX_E_NOMEM, e.what());
  }
  for (uint64_t k = 0; k <= n; k++) rebased[k] = off[k] - text0;
  const int rc = to_device(d_off, rebased.data(), n + 1);
  if (rc || !text_bytes) return rc;      // (no text: `text` may be null)
  return to_device(d_text, reinterpret_cast<const uint8_t *>(text + text0), text_bytes);
}
// ... and a counted table: genes, deletions, counts, and its inserts that way
template <class G, class D> int upload_table(uint64_t n, const G *v, const G *j, const D *vdel, const D *jdel, const uint64_t *count,
                                             const uint64_t *ins_off, const char *ins_text, G *d_v, G *d_j, D *d_vdel, D *d_jdel,
                                             uint64_t *d_count, uint64_t *d_off, uint8_t *d_text) {
  int rc;
  if ((rc = to_device(d_v, v, n)) || (rc = to_device(d_j, j, n)) || (rc = to_device(d_vdel, vdel, n)) || (rc = to_device(d_jdel, jdel, n)) ||
      (rc = to_device(d_count, count, n))) return rc;
  return upload_spans(n, ins_off, ins_text, d_off, d_text);
}

}  // namespace
}  // namespace dcrx_group

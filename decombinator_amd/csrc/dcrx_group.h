// dcrx_group.h — what the count (dcrx_count.hip), the error merge (dcrx_merge.hip) and the clonotype step (dcrx_clono.hip)
// share to group, compact and order a table on the device, each written once: the launch geometry, the 64-bit wave sum,
// the one-allocation pool and the offset carver, hipCUB's four calls with their scratch, run heads, the ordered compaction,
// the most_common() order and the upload of a counted table.  Private to those translation units (HIP only, as dcrx_hip.h).
// Nothing here synchronises or allocates behind the caller's back (Pool::allocate is the caller's one allocation); every
// launch and hipCUB call goes to the stream it is handed.  Everything has internal linkage, as the kernels of those units
// have: a unit's instances of the templated kernels are its own.
#pragma once

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "dcrx_hip.h"

namespace dcrx_group {
namespace {

constexpr int BLOCK = 256;
constexpr uint64_t ALIGN = 256;

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }
inline uint64_t aligned(uint64_t bytes) { return (bytes + ALIGN - 1) & ~(ALIGN - 1); }

// the wave's sum, in lane 0
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int d = warpSize / 2; d > 0; d >>= 1) x += __shfl_down(x, d);
  return x;
}

// device memory of one call of a host entry: ONE allocation, carved into 256-byte aligned buffers (a first pass over the
// same requests, with no memory behind it, adds up the size)
struct Pool {
  dcrx::DevBuf<uint8_t> base;
  uint64_t at = 0;
  template <class T> void get(T **p, uint64_t count) {
    *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += aligned(std::max<uint64_t>(count, 1) * sizeof(T));
  }
  int allocate() {
    const int rc = base.alloc(std::max<uint64_t>(at, 1));
    at = 0;
    return rc;
  }
};

// the offsets of a caller's work space, carved the same way
struct Carver {
  uint64_t at = 0;
  uint64_t take(uint64_t bytes) { const uint64_t here = at; at += aligned(std::max<uint64_t>(bytes, 1)); return here; }
};

// ---- hipCUB: the four calls in use.  A *_bytes query folds the scratch a call over n items wants into `most` (a plan
// asks for every call it will make and holds the largest); the call itself takes its scratch BY VALUE, as hipCUB
// overwrites the size it is handed.  Sorts are stable and ascending over the key's bits [begin_bit, end_bit), begin_bit 0
// unless given; results are in *_out.
// (The scans hand hipCUB plain pointers for input too: it makes its kernels per iterator type, and one set is enough.)
struct Scratch {
  void *p;
  size_t bytes;
};

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

// ---- a counted table from the host (blocking copies): genes, deletions, counts, the offsets rebased to ins_off[0] and the
// text they span
template <class G, class D> int upload_table(uint64_t n, const G *v, const G *j, const D *vdel, const D *jdel, const uint64_t *count,
                                             const uint64_t *ins_off, const char *ins_text, G *d_v, G *d_j, D *d_vdel, D *d_jdel,
                                             uint64_t *d_count, uint64_t *d_off, uint8_t *d_text) {
  const uint64_t text0 = ins_off[0], text_bytes = ins_off[n] - text0;
  std::vector<uint64_t> off(n + 1);
  for (uint64_t k = 0; k <= n; k++) off[k] = ins_off[k] - text0;
  HIP_TRY(hipMemcpy(d_v, v, n * sizeof(G), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_j, j, n * sizeof(G), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_vdel, vdel, n * sizeof(D), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_jdel, jdel, n * sizeof(D), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_count, count, n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
  if (text_bytes) HIP_TRY(hipMemcpy(d_text, ins_text + text0, text_bytes, hipMemcpyHostToDevice));
  return DCRX_OK;
}

}  // namespace
}  // namespace dcrx_group

// dcrx_count.hip — the DCR count of the barcode-free stage (`decombine -nbc --count-dcrs`): every decombined read's DCR
// (v, j, vdel, jdel, insert; dcrx_count_core.h) added into a table that lives on the device across batches, and at the end
// the distinct DCRs in collections.Counter.most_common() order (count descending, ties by the DCR's first read).
//
// One count step over a batch's records (dcrx_count_device), all on the caller's stream:
//   keys     one lane per read: the insert's bytes out of the packed read and its exceptions into a scratch slot of the
//            read's own, and the key's 63-bit hash (NO_KEY for a read that did not decombine)
//   sort     the hashes with the read positions (hipCUB radix sort, stable: a run of one hash keeps its reads in batch order)
//   runs     each run's head (max scan of head positions); every other read of the run compares its key with the head's in
//            full — the same DCR adds nothing but its place in the run, a different one (a hash collision) is a straggler
//   insert   one lane per run head and per straggler: ONE update of the global table per distinct key and batch, however
//            clonal the batch (a clone of a million reads costs one atomic add, not a million).  Arena bytes for the
//            inserting lanes are taken with one atomic per wave.
// The table is open addressing over 64-bit tags (0 empty, 2 being written, hash << 1 | 1 published).  A lane claims an empty
// slot with a CAS, writes the key (header, arena offset), count and first ordinal, and publishes the tag with a release
// store; a lane that meets a published tag with its hash compares the full key (header and every insert byte) before it adds
// its count (atomicAdd) and its first ordinal (atomicMin): a hash match alone never merges two DCRs.  A lane that meets a slot
// being written reads it again in its next pass of the loop, so the writer — in the same wave or another — always finishes.
// Integer atomics only: the counts do not depend on the order in which updates land.
//
// Room: the host keeps upper bounds of the keys and arena bytes the table may hold (each read adds at most one key and its
// insert); before a step would pass them it synchronises, reads the true figures and grows the table (a rehash on the
// device) or the arena.  A step that still ran out of room would set a flag that every read-out reports as an error: a key
// or a count is never dropped silently.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "dcrx_count_core.h"
#include "dcrx_group.h"

using namespace dcrx;
using namespace dcrx_count;
using namespace dcrx_group;

namespace {

constexpr uint64_t TAG_EMPTY = 0, TAG_BUSY = 2;
constexpr uint64_t MIN_SLOTS = 1u << 16;
constexpr uint64_t MIN_ARENA = 16u << 20;

// stats words on the device
enum { ST_ARENA = 0, ST_KEYS = 1, ST_OVERFLOW = 2, ST_WORDS = 4 };

struct Rec {
  uint32_t v, j, ins_start, ins_len, vdel, jdel, status, frame;
};

__device__ __forceinline__ Rec load_rec(const dcrx_record_t *recs, uint64_t r) {
  const uint4 w = reinterpret_cast<const uint4 *>(recs)[r];
  Rec R;
  R.v = w.x & 0xFFFFu; R.j = w.x >> 16;
  R.ins_start = w.z & 0xFFFFu; R.ins_len = w.z >> 16;
  R.vdel = w.w & 0xFFu; R.jdel = (w.w >> 8) & 0xFFu; R.status = (w.w >> 16) & 0xFFu; R.frame = w.w >> 24;
  return R;
}

__device__ __forceinline__ uint64_t ordinal(uint64_t first_index, const uint32_t *index, uint32_t r) {
  return first_index + (index ? (uint64_t)index[r] : (uint64_t)r);
}

__global__ __launch_bounds__(BLOCK) void count_keys_kernel(const dcrx_record_t *__restrict__ recs, dcrx_batch_t B, uint64_t slot,
                                                           uint64_t hash_mask, uint8_t *__restrict__ scratch,
                                                           uint64_t *__restrict__ hash, uint32_t *__restrict__ pos) {
  const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= B.n_reads) return;
  pos[r] = (uint32_t)r;
  const Rec R = load_rec(recs, r);
  if (R.status != DCRX_S_OK) { hash[r] = NO_KEY; return; }
  const uint32_t len = B.lens ? B.lens[r] : B.read_len;
  // the read's exceptions: the first entry of read r (the list is sorted by read, then position)
  uint64_t lo = 0, hi = B.n_exc;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (B.exc_read[mid] < r) lo = mid + 1; else hi = mid;
  }
  uint64_t e1 = lo;
  while (e1 < B.n_exc && B.exc_read[e1] == r) e1++;
  uint8_t *out = scratch + r * slot;
  insert_bytes(B.packed + r * (uint64_t)B.stride, len, R.frame, R.ins_start, R.ins_len, B.exc_pos + lo, B.exc_chr + lo,
               (uint32_t)(e1 - lo), out);
  hash[r] = key_hash(header(R.v, R.j, R.vdel, R.jdel, R.ins_len), out, R.ins_len) & hash_mask;
}

// the mark of a run of equal hashes (dcrx_group.h: run_heads then gives every position its run's head), and the run's state
__global__ __launch_bounds__(BLOCK) void count_heads_kernel(const uint64_t *__restrict__ hash, const uint32_t *__restrict__ pos,
                                                            uint64_t n, uint64_t first_index, const uint32_t *__restrict__ index,
                                                            uint32_t *__restrict__ head, uint32_t *__restrict__ run_strag,
                                                            uint64_t *__restrict__ run_first, uint8_t *__restrict__ strag) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  head[i] = run_mark(i, [&](uint64_t k) { return hash[k]; });
  strag[i] = 0;
  run_strag[i] = 0;
  run_first[i] = ordinal(first_index, index, pos[i]);
}

__device__ __forceinline__ uint64_t rec_header(const Rec &R) { return header(R.v, R.j, R.vdel, R.jdel, R.ins_len); }

__global__ __launch_bounds__(BLOCK) void count_members_kernel(const dcrx_record_t *__restrict__ recs, const uint64_t *__restrict__ hash,
                                                              const uint32_t *__restrict__ pos, const uint32_t *__restrict__ head_of,
                                                              uint64_t n, const uint8_t *__restrict__ scratch, uint64_t slot,
                                                              uint64_t first_index, const uint32_t *__restrict__ index,
                                                              uint32_t *__restrict__ run_len, uint32_t *__restrict__ run_strag,
                                                              uint64_t *__restrict__ run_first, uint8_t *__restrict__ strag) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t hv = hash[i];
  if (hv == NO_KEY) return;
  const uint32_t hd = head_of[i];
  if (i + 1 == n || hash[i + 1] != hv) run_len[hd] = (uint32_t)(i + 1 - hd);       // the run's last read: its length
  if (i == hd) return;
  const uint32_t p = pos[i], q = pos[hd];
  const Rec a = load_rec(recs, p), b = load_rec(recs, q);
  if (!key_equal(rec_header(a), scratch + (uint64_t)p * slot, rec_header(b), scratch + (uint64_t)q * slot)) {
    strag[i] = 1;                                   // same hash, another DCR: inserted on its own
    atomicAdd(&run_strag[hd], 1u);
    return;
  }
  const uint64_t o = ordinal(first_index, index, p);
  if (o < run_first[hd]) atomicMin(reinterpret_cast<unsigned long long *>(&run_first[hd]), (unsigned long long)o);
}

struct Table {
  uint64_t *tag, *hdr, *off, *count, *first;
  uint64_t mask;
};

// inclusive prefix sum of x over the wave's lanes
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x) {
  const int lane = __lane_id();
#pragma unroll
  for (int d = 1; d < warpSize; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

__global__ __launch_bounds__(BLOCK) void count_insert_kernel(const dcrx_record_t *__restrict__ recs, const uint64_t *__restrict__ hash,
                                                             const uint32_t *__restrict__ pos, const uint32_t *__restrict__ head_of,
                                                             uint64_t n, const uint8_t *__restrict__ scratch, uint64_t slot,
                                                             uint64_t first_index, const uint32_t *__restrict__ index,
                                                             const uint32_t *__restrict__ run_len, const uint32_t *__restrict__ run_strag,
                                                             const uint64_t *__restrict__ run_first, const uint8_t *__restrict__ strag,
                                                             Table T, uint8_t *__restrict__ arena, uint64_t arena_cap,
                                                             uint64_t *__restrict__ stats) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool want = false;
  uint64_t cnt = 0, first = 0, hv = 0;
  uint32_t p = 0;
  if (i < n) {
    hv = hash[i];
    if (hv != NO_KEY) {
      p = pos[i];
      const uint32_t hd = head_of[i];
      if (i == hd) { want = true; cnt = run_len[i] - run_strag[i]; first = run_first[i]; }
      else if (strag[i]) { want = true; cnt = 1; first = ordinal(first_index, index, p); }
    }
  }
  Rec R{};
  if (want) R = load_rec(recs, p);
  const uint32_t len = want ? R.ins_len : 0u;
  // arena room for every inserting lane of the wave, one atomic (a key found in the table leaves its bytes unused)
  const uint32_t incl = wave_incl_sum(len);
  const uint32_t total = __shfl(incl, warpSize - 1);
  unsigned long long base = 0;
  if (__lane_id() == warpSize - 1 && total) base = atomicAdd(reinterpret_cast<unsigned long long *>(&stats[ST_ARENA]), (unsigned long long)total);
  base = __shfl(base, warpSize - 1);
  const uint64_t off = base + (incl - len);
  bool claimed = false;
  if (want && off + len > arena_cap) {
    atomicOr(reinterpret_cast<unsigned long long *>(&stats[ST_OVERFLOW]), 1ull);    // (the host's bounds make this unreachable)
    want = false;
  }
  if (want) {
    const uint64_t hdr = rec_header(R);
    const uint8_t *key = scratch + (uint64_t)p * slot;
    const uint64_t tagv = (hv << 1) | 1u;
    uint64_t s = hv & T.mask;
    for (;;) {
      const uint64_t t = __hip_atomic_load(&T.tag[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      if (t == TAG_EMPTY) {
        if (atomicCAS(reinterpret_cast<unsigned long long *>(&T.tag[s]), TAG_EMPTY, TAG_BUSY) == TAG_EMPTY) {
          for (uint32_t b = 0; b < len; b++) arena[off + b] = key[b];
          T.hdr[s] = hdr; T.off[s] = off; T.count[s] = cnt; T.first[s] = first;
          __hip_atomic_store(&T.tag[s], tagv, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          claimed = true;
          break;
        }
        continue;                                   // another lane took it: read the slot again
      }
      if (t == TAG_BUSY) continue;                  // being written: read it again
      if (t == tagv && key_equal(hdr, key, T.hdr[s], arena + T.off[s])) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&T.count[s]), (unsigned long long)cnt);
        atomicMin(reinterpret_cast<unsigned long long *>(&T.first[s]), (unsigned long long)first);
        break;
      }
      s = (s + 1) & T.mask;
    }
  }
  const unsigned long long got = __ballot(claimed);
  if (__lane_id() == 0 && got) atomicAdd(reinterpret_cast<unsigned long long *>(&stats[ST_KEYS]), (unsigned long long)__popcll(got));
}

// the published slots of `from` into `to` (every key is distinct: no comparison)
__global__ __launch_bounds__(BLOCK) void count_rehash_kernel(Table from, uint64_t from_slots, Table to) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= from_slots) return;
  const uint64_t t = from.tag[i];
  if (!(t & 1u)) return;
  uint64_t s = (t >> 1) & to.mask;
  for (;;) {
    if (atomicCAS(reinterpret_cast<unsigned long long *>(&to.tag[s]), TAG_EMPTY, (unsigned long long)t) == TAG_EMPTY) {
      to.hdr[s] = from.hdr[i]; to.off[s] = from.off[i]; to.count[s] = from.count[i]; to.first[s] = from.first[i];
      return;
    }
    s = (s + 1) & to.mask;
  }
}

// the published slots, in any order (the sort that follows orders them)
__global__ __launch_bounds__(BLOCK) void count_compact_kernel(const uint64_t *__restrict__ tag, uint64_t slots,
                                                              uint64_t *__restrict__ list, uint64_t *__restrict__ n_list) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < slots && (tag[i] & 1u);
  const unsigned long long m = __ballot(live);
  unsigned long long base = 0;
  if (__lane_id() == 0 && m) base = atomicAdd(reinterpret_cast<unsigned long long *>(n_list), (unsigned long long)__popcll(m));
  base = __shfl(base, 0);
  if (live) list[base + __popcll(m & ((1ull << __lane_id()) - 1))] = i;
}

inline uint64_t digits(uint64_t x) { uint64_t d = 1; while (x >= 10) { x /= 10; d++; } return d; }
inline char *put_u64(char *o, uint64_t x) {
  char t[20];
  int k = 0;
  do { t[k++] = (char)('0' + x % 10); x /= 10; } while (x);
  while (k) *o++ = t[--k];
  return o;
}

// the insert bytes the published slots hold (the text a read-out returns)
__global__ __launch_bounds__(BLOCK) void count_text_kernel(const uint64_t *__restrict__ tag, const uint64_t *__restrict__ hdr,
                                                           uint64_t slots, unsigned long long *__restrict__ total) {
  unsigned long long sum = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * BLOCK)
    if (tag[i] & 1u) sum += header_len(hdr[i]);
  sum = wave_sum(sum);
  if (__lane_id() == 0 && sum) atomicAdd(total, sum);
}

// (an allocation of no elements still gives a pointer a kernel may be handed)
template <class T> int dev_alloc(DevBuf<T> &b, uint64_t count) { return b.alloc(std::max<uint64_t>(count, 1)); }

// the table's columns in device memory, and the table as the kernels take it
struct TableBufs {
  DevBuf<uint64_t> tag, hdr, off, count, first;
  uint64_t mask = 0;
  Table view() const { return Table{tag, hdr, off, count, first, mask}; }
};

// one step's work space, for up to n reads of up to slot bases
struct Work {
  uint64_t n = 0, slot = 0;
  DevBuf<uint8_t> scratch, strag, cub;
  DevBuf<uint64_t> hash[2], run_first;
  DevBuf<uint32_t> pos[2], head, head_of, run_len, run_strag;
  size_t cub_bytes = 0;
};

}  // namespace

struct dcrx_counts {
  int device = -1;
  TableBufs T;
  uint64_t slots = 0;
  DevBuf<uint8_t> arena;
  uint64_t arena_cap = 0;
  DevBuf<uint64_t> stats;           // ST_WORDS on the device
  uint64_t bound_keys = 0, bound_bytes = 0;    // what the table and the arena can hold at most by now
  Work work;
  DevBuf<uint32_t> index;           // the host entries' copy of a chunk's slice of the caller's index
  uint64_t index_cap = 0;
  uint64_t hash_mask = NO_KEY >> 1;  // the hash bits a key keeps (dcrx_counts_set_hash_bits)
};

namespace {

int alloc_table(TableBufs &T, uint64_t slots, hipStream_t s) {
  TableBufs N;
  int rc;
  if ((rc = dev_alloc(N.tag, slots)) || (rc = dev_alloc(N.hdr, slots)) || (rc = dev_alloc(N.off, slots)) ||
      (rc = dev_alloc(N.count, slots)) || (rc = dev_alloc(N.first, slots))) return rc;
  N.mask = slots - 1;
  HIP_TRY(hipMemsetAsync(N.tag, 0, slots * sizeof(uint64_t), s));
  T = std::move(N);
  return DCRX_OK;
}

int check_device(dcrx_counts *c) {
  int dev = -1;
  HIP_TRY(hipGetDevice(&dev));
  if (c->device < 0) c->device = dev;
  if (c->device != dev) return set_err(DCRX_E_INVALID, "dcrx_counts_t: used on another device than the one it was made on");
  return DCRX_OK;
}

int ensure_stats(dcrx_counts *c, hipStream_t s) {
  if (c->stats) return DCRX_OK;
  int rc = dev_alloc(c->stats, ST_WORDS);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->stats, 0, ST_WORDS * sizeof(uint64_t), s));
  return DCRX_OK;
}

// the true figures of the table (synchronises the stream): bounds come down to them
int read_stats(dcrx_counts *c, hipStream_t s, uint64_t st[ST_WORDS]) {
  HIP_TRY(hipStreamSynchronize(s));
  const int rc = to_host(st, c->stats.get(), ST_WORDS);
  if (rc) return rc;
  if (st[ST_OVERFLOW]) return set_err(DCRX_E_HIP, "dcrx_counts: the arena ran out of room during a count step (counts are incomplete)");
  c->bound_keys = st[ST_KEYS];
  c->bound_bytes = st[ST_ARENA];
  return DCRX_OK;
}

uint64_t pow2_at_least(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }

// room for `keys` more keys (the table at most half full) and `bytes` more arena bytes
int ensure_room(dcrx_counts *c, hipStream_t s, uint64_t keys, uint64_t bytes) {
  int rc = ensure_stats(c, s);
  if (rc) return rc;
  auto fits = [&] { return c->slots >= 2 * (c->bound_keys + keys) && c->arena_cap >= c->bound_bytes + bytes; };
  if (fits()) return DCRX_OK;
  if (c->slots || c->arena_cap) {
    uint64_t st[ST_WORDS];
    rc = read_stats(c, s, st);
    if (rc) return rc;
    if (fits()) return DCRX_OK;
  }
  const uint64_t want_slots = std::max<uint64_t>(MIN_SLOTS, pow2_at_least(2 * (c->bound_keys + keys)));
  if (want_slots > c->slots) {
    TableBufs N;
    rc = alloc_table(N, want_slots, s);
    if (rc) return rc;
    if (c->slots) {
      count_rehash_kernel<<<grid_for(c->slots), BLOCK, 0, s>>>(c->T.view(), c->slots, N.view());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(s));
    }
    c->T = std::move(N);
    c->slots = want_slots;
  }
  const uint64_t need = c->bound_bytes + bytes;
  if (need > c->arena_cap) {
    const uint64_t cap = std::max<uint64_t>({MIN_ARENA, need + need / 2, 2 * c->arena_cap});
    DevBuf<uint8_t> a;
    rc = dev_alloc(a, cap);
    if (rc) return rc;
    if (c->arena && c->bound_bytes) {
      // (the bound is the true figure here: read_stats ran above)
      HIP_TRY(hipMemcpyAsync(a, c->arena, c->bound_bytes, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
    c->arena = std::move(a);
    c->arena_cap = cap;
  }
  return DCRX_OK;
}

int ensure_work(dcrx_counts *c, hipStream_t s, uint64_t n, uint64_t slot) {
  if (n <= c->work.n && n * slot <= c->work.n * c->work.slot) return DCRX_OK;
  HIP_TRY(hipStreamSynchronize(s));         // (the last step on this stream may still read the old buffers)
  const uint64_t wn = std::max(n, c->work.n), ws = std::max(slot, c->work.slot);
  c->work = Work{};
  Work W;
  int rc;
  if ((rc = dev_alloc(W.scratch, wn * ws)) || (rc = dev_alloc(W.hash[0], wn)) || (rc = dev_alloc(W.hash[1], wn)) ||
      (rc = dev_alloc(W.pos[0], wn)) || (rc = dev_alloc(W.pos[1], wn)) || (rc = dev_alloc(W.head, wn)) ||
      (rc = dev_alloc(W.head_of, wn)) || (rc = dev_alloc(W.run_len, wn)) || (rc = dev_alloc(W.run_strag, wn)) ||
      (rc = dev_alloc(W.run_first, wn)) || (rc = dev_alloc(W.strag, wn))) return rc;
  if ((rc = sort_pairs_bytes<uint32_t>(wn, 64, &W.cub_bytes)) || (rc = run_heads_bytes(wn, &W.cub_bytes)) ||
      (rc = dev_alloc(W.cub, W.cub_bytes))) return rc;
  W.n = wn; W.slot = ws;
  c->work = std::move(W);
  return DCRX_OK;
}

int count_step(dcrx_counts *c, const dcrx_record_t *d_records, const dcrx_batch_t *b, uint64_t first_index,
               const uint32_t *d_index, hipStream_t s) {
  const uint64_t n = b->n_reads;
  const uint64_t slot = std::max<uint64_t>(1, b->lens ? 4ull * b->stride : b->read_len);
  int rc = ensure_work(c, s, n, slot);
  if (rc) return rc;
  rc = ensure_room(c, s, n, n * slot);
  if (rc) return rc;
  const Work &W = c->work;
  const unsigned g = grid_for(n);
  count_keys_kernel<<<g, BLOCK, 0, s>>>(d_records, *b, slot, c->hash_mask, W.scratch, W.hash[0], W.pos[0]);
  HIP_TRY(hipGetLastError());
  const Scratch cub{W.cub, W.cub_bytes};
  if ((rc = sort_pairs<uint32_t>(cub, W.hash[0], W.hash[1], W.pos[0], W.pos[1], n, 64, s))) return rc;
  count_heads_kernel<<<g, BLOCK, 0, s>>>(W.hash[1], W.pos[1], n, first_index, d_index, W.head, W.run_strag, W.run_first, W.strag);
  HIP_TRY(hipGetLastError());
  if ((rc = run_heads(cub, W.head, W.head_of, n, s))) return rc;
  count_members_kernel<<<g, BLOCK, 0, s>>>(d_records, W.hash[1], W.pos[1], W.head_of, n, W.scratch, slot, first_index, d_index,
                                           W.run_len, W.run_strag, W.run_first, W.strag);
  HIP_TRY(hipGetLastError());
  count_insert_kernel<<<g, BLOCK, 0, s>>>(d_records, W.hash[1], W.pos[1], W.head_of, n, W.scratch, slot, first_index, d_index,
                                          W.run_len, W.run_strag, W.run_first, W.strag, c->T.view(), c->arena, c->arena_cap, c->stats);
  HIP_TRY(hipGetLastError());
  c->bound_keys += n;
  c->bound_bytes += n * slot;
  return DCRX_OK;
}

}  // namespace

namespace dcrx {
// the host entries' count step over one chunk: `h_index` (host, cn entries, or null) is that chunk's slice of the caller's index
int count_chunk(dcrx_counts *c, const dcrx_record_t *d_records, const dcrx_batch_t *d_batch, uint64_t first_index,
                const uint32_t *h_index, hipStream_t s) {
  const uint32_t *d_index = nullptr;
  if (h_index && d_batch->n_reads) {
    if (d_batch->n_reads > c->index_cap) {
      HIP_TRY(hipStreamSynchronize(s));
      c->index_cap = 0;
      int rc = dev_alloc(c->index, d_batch->n_reads);
      if (rc) return rc;
      c->index_cap = d_batch->n_reads;
    }
    HIP_TRY(hipMemcpyAsync(c->index, h_index, d_batch->n_reads * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    d_index = c->index;
  }
  return dcrx_count_device(c, d_records, d_batch, first_index, d_index, s);
}
// the figures a host entry settles at its end (it has synchronised its streams): the bounds come down to them
int count_settle(dcrx_counts *c, hipStream_t s) {
  if (!c->stats) return DCRX_OK;
  uint64_t st[ST_WORDS];
  return read_stats(c, s, st);
}
}  // namespace dcrx

extern "C" {

int dcrx_counts_create(dcrx_counts_t **out) {
  if (!out) return set_err(DCRX_E_INVALID, "out is null");
  *out = nullptr;
  dcrx_counts *c = new (std::nothrow) dcrx_counts();
  if (!c) return set_err(DCRX_E_NOMEM, "out of host memory in dcrx_counts_create");
  *out = c;
  return DCRX_OK;
}

void dcrx_counts_destroy(dcrx_counts_t *c) {
  if (!c) return;
  if (c->device >= 0) (void)hipDeviceSynchronize();      // (nothing of it is still read when its buffers go)
  delete c;
}

int dcrx_counts_reset(dcrx_counts_t *c) {
  if (!c) return set_err(DCRX_E_INVALID, "counts is null");
  if (c->device < 0) return DCRX_OK;
  int rc = check_device(c);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (c->slots) HIP_TRY(hipMemset(c->T.tag, 0, c->slots * sizeof(uint64_t)));
  if (c->stats) HIP_TRY(hipMemset(c->stats, 0, ST_WORDS * sizeof(uint64_t)));
  c->bound_keys = c->bound_bytes = 0;
  return DCRX_OK;
}

int dcrx_counts_set_hash_bits(dcrx_counts_t *c, uint32_t bits) {
  if (!c) return set_err(DCRX_E_INVALID, "counts is null");
  if (bits > 63) return set_err(DCRX_E_INVALID, "dcrx_counts_set_hash_bits: bits must be 0 .. 63");
  if (c->bound_keys) return set_err(DCRX_E_INVALID, "dcrx_counts_set_hash_bits: the table is not empty (create or reset it first)");
  c->hash_mask = bits ? (NO_KEY >> (64 - bits)) : 0;
  return DCRX_OK;
}

int dcrx_count_device(dcrx_counts_t *c, const dcrx_record_t *d_records, const dcrx_batch_t *b, uint64_t first_index,
                      const uint32_t *d_index, void *stream) {
  if (!c || !b) return set_err(DCRX_E_INVALID, "null argument");
  if (b->n_reads >= (1ull << 31)) return set_err(DCRX_E_INVALID, "dcrx_count_device: more than 2^31-1 reads in one step");
  if (b->n_reads == 0) return DCRX_OK;
  if (!d_records || !b->packed) return set_err(DCRX_E_INVALID, "d_records or the batch's packed reads are null");
  if (b->stride == 0 || (b->stride & 7u)) return set_err(DCRX_E_INVALID, "stride must be a positive multiple of 8");
  if (!b->lens && b->read_len > 4 * b->stride) return set_err(DCRX_E_INVALID, "read_len exceeds 4*stride");
  if (b->n_exc && (!b->exc_read || !b->exc_pos || !b->exc_chr)) return set_err(DCRX_E_INVALID, "exception arrays are null");
  int rc = check_device(c);
  if (rc) return rc;
  try { return count_step(c, d_records, b, first_index, d_index, (hipStream_t)stream); }
  catch (...) { return set_err(DCRX_E_NOMEM, "dcrx_count_device: out of host memory"); }
}

int64_t dcrx_counts_read(dcrx_counts_t *c, uint16_t *v, uint16_t *j, uint8_t *vdel, uint8_t *jdel, uint64_t *count,
                         uint64_t *first, uint64_t *ins_off, char *ins_text, uint64_t cap, uint64_t text_cap,
                         uint64_t *text_bytes) try {
  if (!c || !text_bytes) return set_err(DCRX_E_INVALID, "null argument");
  *text_bytes = 0;
  if (c->device < 0 || !c->slots) {
    if (ins_off) ins_off[0] = 0;
    return 0;
  }
  int rc = check_device(c);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());          // (whatever stream the steps ran on)
  uint64_t st[ST_WORDS];
  rc = read_stats(c, nullptr, st);
  if (rc) return rc;
  const uint64_t n = st[ST_KEYS];
  if (n >= (1ull << 31)) return set_err(DCRX_E_UNSUPPORTED, "dcrx_counts_read: 2^31 or more distinct DCRs");
  if (cap < n || !v || !j || !vdel || !jdel || !count || !first || !ins_off) {
    // sizes only: the key count and the inserts' bytes, no compaction and no sort
    DevBuf<unsigned long long> d_total;
    rc = dev_alloc(d_total, 1);
    if (rc) return rc;
    unsigned long long total = 0;
    HIP_TRY(hipMemset(d_total, 0, sizeof(total)));
    count_text_kernel<<<(unsigned)std::min<uint64_t>(grid_for(c->slots), 2048), BLOCK>>>(c->T.tag, c->T.hdr, c->slots, d_total);
    HIP_TRY(hipGetLastError());
    if ((rc = to_host(&total, d_total.get(), 1))) return rc;
    *text_bytes = total;
    return (int64_t)n;
  }
  // the compact list of live slots, ordered by first ordinal, then (stably) by count descending
  std::vector<uint64_t> hdr(n), off(n), cnt(n), fst(n);
  auto run = [&]() -> int {       // (its device buffers go when it returns)
    DevBuf<uint64_t> list_buf[2], key_buf[2], n_list;
    DevBuf<uint8_t> tmp;
    int r;
    if ((r = dev_alloc(list_buf[0], n)) || (r = dev_alloc(list_buf[1], n)) || (r = dev_alloc(key_buf[0], n)) ||
        (r = dev_alloc(key_buf[1], n)) || (r = dev_alloc(n_list, 1))) return r;
    uint64_t *const list[2] = {list_buf[0], list_buf[1]}, *const key[2] = {key_buf[0], key_buf[1]};
    HIP_TRY(hipMemset(n_list, 0, sizeof(uint64_t)));
    count_compact_kernel<<<grid_for(c->slots), BLOCK>>>(c->T.tag, c->slots, list[0], n_list);
    HIP_TRY(hipGetLastError());
    uint64_t got = 0;
    if ((r = to_host(&got, n_list.get(), 1))) return r;
    if (got != n) return set_err(DCRX_E_HIP, "dcrx_counts_read: the table's live slots differ from its key count");
    if (!n) return DCRX_OK;
    size_t tb = 0;
    if ((r = sort_pairs_bytes<uint64_t>(n, 64, &tb)) || (r = dev_alloc(tmp, tb)) ||
        (r = most_common_order(Scratch{tmp, tb}, list, key, c->T.first.get(), 64, c->T.count.get(), (uint32_t)n, nullptr))) return r;
    // list[0]: the slots in most_common() order
    uint64_t *fields[4] = {c->T.hdr, c->T.off, c->T.count, c->T.first};
    std::vector<uint64_t> *host[4] = {&hdr, &off, &cnt, &fst};
    for (int f = 0; f < 4; f++) {
      if ((r = gather(fields[f], list[0], (uint32_t)n, 0, key[1], nullptr)) || (r = to_host(host[f]->data(), key[1], n))) return r;
    }
    return DCRX_OK;
  };
  rc = run();
  if (rc) return rc;
  uint64_t bytes = 0;
  for (uint64_t k = 0; k < n; k++) bytes += header_len(hdr[k]);
  *text_bytes = bytes;
  if (cap < n || text_cap < bytes || !v || !j || !vdel || !jdel || !count || !first || !ins_off || (bytes && !ins_text))
    return (int64_t)n;                                // (sizes only)
  std::vector<uint8_t> arena(st[ST_ARENA]);
  if ((rc = to_host(arena.data(), c->arena.get(), arena.size()))) return rc;
  uint64_t at = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint64_t h = hdr[k];
    v[k] = (uint16_t)(h & 0xFFFF); j[k] = (uint16_t)((h >> 16) & 0xFFFF);
    vdel[k] = (uint8_t)((h >> 32) & 0xFF); jdel[k] = (uint8_t)((h >> 40) & 0xFF);
    count[k] = cnt[k]; first[k] = fst[k];
    ins_off[k] = at;
    const uint32_t len = header_len(h);
    if (len) std::memcpy(ins_text + at, arena.data() + off[k], len);
    at += len;
  }
  ins_off[n] = at;
  return (int64_t)n;
} catch (const std::exception &e) {      // (the entry's one guard: the host copies of the table's columns and of the arena)
  return set_err(DCRX_E_NOMEM, e.what());
}

int64_t dcrx_format_counts(uint64_t n, const uint16_t *v, const uint16_t *j, const uint8_t *vdel, const uint8_t *jdel,
                           const uint64_t *count, const uint64_t *ins_off, const char *ins_text, const char *field_sep,
                           char *out, uint64_t out_cap) {
  if (n && (!v || !j || !vdel || !jdel || !count || !ins_off || !field_sep)) return set_err(DCRX_E_INVALID, "null argument");
  if (!field_sep) return 0;
  const uint64_t sl = std::strlen(field_sep);
  const uint64_t text = n ? ins_off[n] - ins_off[0] : 0;
  auto write = [&]() -> uint64_t {
    char *o = out;
    for (uint64_t k = 0; k < n; k++) {
      o = put_u64(o, v[k]); std::memcpy(o, field_sep, sl); o += sl;
      o = put_u64(o, j[k]); std::memcpy(o, field_sep, sl); o += sl;
      o = put_u64(o, vdel[k]); std::memcpy(o, field_sep, sl); o += sl;
      o = put_u64(o, jdel[k]); std::memcpy(o, field_sep, sl); o += sl;
      const uint64_t il = ins_off[k + 1] - ins_off[k];
      if (il) { std::memcpy(o, ins_text + ins_off[k], il); o += il; }
      std::memcpy(o, field_sep, sl); o += sl;
      o = put_u64(o, count[k]);
      *o++ = '\n';
    }
    return (uint64_t)(o - out);
  };
  // one pass when the buffer holds the longest text these lines can take (DCRX_COUNTS_LINE_BOUND per line), else the
  // exact size first
  if (out && out_cap >= n * (DCRX_COUNTS_LINE_BOUND + 5 * sl) + text) return (int64_t)write();
  uint64_t need = text;
  for (uint64_t k = 0; k < n; k++)
    need += digits(v[k]) + digits(j[k]) + digits(vdel[k]) + digits(jdel[k]) + digits(count[k]) + 5 * sl + 1;
  if (out && need <= out_cap) write();
  return (int64_t)need;
}

}  // extern "C"

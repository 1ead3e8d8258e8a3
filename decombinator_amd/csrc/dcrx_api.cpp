// dcrx_api.cpp — the C ABI declared in include/dcrx.h and include/dcrx_synth.h.
//
// Host side of the boundary: validates arguments, owns the table handle and its
// per-device workspace, launches the kernels of dcrx_kernels.hip.  There is no
// CPU implementation of the hot path in this library: every decombine entry
// point needs a GPU and fails with DCRX_E_NOGPU / DCRX_E_HIP without one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dcrx.h"
#include "../../include/dcrx_synth.h"
#include "dcrx_hip.h"
#include "dcrx_launch.h"
#include "dcrx_synth_core.h"
#include <cstdlib>
#include <thread>

#include "dcrx_merge_core.h"
#include "dcrx_tables.h"

namespace dcrx {
hipError_t launch_synth(const DevTables &T, const SynthParams &P, uint64_t first, uint64_t n, uint32_t stride,
                        uint8_t *d_packed, hipStream_t s);
// dcrx_count.hip: the host entries' count step over one chunk, and the figures a count settles once its stream is drained
int count_chunk(dcrx_counts_t *c, const dcrx_record_t *d_records, const dcrx_batch_t *d_batch, uint64_t first_index,
                const uint32_t *h_index, hipStream_t s);
int count_settle(dcrx_counts_t *c, hipStream_t s);
int merge_windows(dcrx_tables_t *t, const uint32_t **d_rows, uint32_t *n_v, uint32_t *n_j);
}

using namespace dcrx;

static thread_local std::string g_err;

static int set_err(int code, const std::string &m) { g_err = m; return code; }
namespace dcrx { int set_err(int code, const char *msg) { return ::set_err(code, std::string(msg)); } }
// reads per chunk of the host-buffer entry (dcrx_decombine): 80 MB in, 32 MB out at 150 nt
#ifndef DCRX_HOST_CHUNK
#define DCRX_HOST_CHUNK (2u << 20)
#endif

// memcpy over a few threads (a pinned staging buffer has to be filled faster than the link drains it)
static void par_memcpy(void *dst, const void *src, size_t n) {
  static const unsigned want = [] { const char *e = std::getenv("DCRX_HOST_THREADS"); unsigned k = e ? (unsigned)std::atoi(e) : std::min(12u, std::max(1u, std::thread::hardware_concurrency() / 2)); return std::max(1u, std::min(k, 16u)); }();
  const unsigned nt = n < (8u << 20) ? 1u : want;
  if (nt == 1) { std::memcpy(dst, src, n); return; }
  // (a worker that cannot be started — std::system_error, or no memory for the vector — leaves its slice to this thread:
  // nothing is thrown past the threads already running)
  std::thread th[16];
  const size_t per = ((n / nt) + 4095) & ~(size_t)4095;
  for (unsigned k = 1; k < nt; k++) {
    const size_t a = std::min(n, per * k), b = std::min(n, per * (k + 1));
    if (b <= a) continue;
    try { th[k] = std::thread([=] { std::memcpy((uint8_t *)dst + a, (const uint8_t *)src + a, b - a); }); }
    catch (...) { std::memcpy((uint8_t *)dst + a, (const uint8_t *)src + a, b - a); }
  }
  std::memcpy(dst, src, std::min(n, per));
  for (auto &x : th) if (x.joinable()) x.join();
}

// Everything a handle keeps on the device its tables were last used on.  All of it is owned here: a fresh DeviceState
// assigned over this one (with that device current) releases the lot.
struct DeviceState {
  int device = -1;
  DevBuf<uint8_t> blob;
  DevTables dev{};
  DevBuf<DevTables> d_dev;      // the same struct in device memory (what a kernel's rare paths read instead of holding it in registers)
  LaunchPlan plan{};            // (its pointers are copies of the owners below: fill_plan)
  DevBuf<uint32_t> exc_flag; uint64_t exc_flag_reads = 0;
  DevBuf<uint32_t> queue;       // [DCRX_QUEUE_HEADER work counters][exc_flag_reads rescue indices][exc_flag_reads general indices]
  // v2 kernels: the per-wave lists between scan and finishing
  DevBuf<uint4> v2_tail, v2_events, v2_slow;
  DevBuf<uint32_t> v2_counts;
  DevBuf<uint4> v2_left;        // the finishing launch's left list
  DevBuf<uint64_t> v2_acc;      // the v2 kernels' tallies of the call in flight (zero between calls)
  Stream v2_side, v2_side2;
  Event v2_ev_fork, v2_ev_join, v2_ev_join2;
  // staging for the host-buffer entry point: two sets of device buffers and pinned host buffers, three streams
  // (copies in, kernels, copies out) and the events that order them
  DevBuf<uint8_t> d_stage; size_t stage_bytes = 0;
  PinnedBuf<uint8_t> h_stage; size_t h_stage_bytes = 0;
  Stream hs_in, hs_run, hs_out;
  Event hev_in[2], hev_run[2], hev_out[2];
  V2Tune tune[2];               // the handle's timing of its own finishing launches (launch_v2), per frame
  // the kernels' side of the tuple sink
  DevBuf<V2SinkDev> sink; DevBuf<uint2> sink_items; DevBuf<uint32_t> sink_ctr;
  uint64_t sink_items_cap = 0; uint32_t sink_regions_cap = 0;
};

// the error merge's germline windows (dcrx_merge_core.h), on the device they were last asked for
struct MergeRows { int device = -1; DevBuf<uint32_t> rows; };

struct dcrx_tables {
  HostTables host;
  DeviceState state;
  bool ws_dirty = true;       // work counters / exception bitmap must be zeroed before the next launch
  uint32_t reserved_cus = 0;
  bool tune_may_wait = false;       // dcrx_set_tune_wait
  // the tail list (a third of the lists' bytes) exists only for handles whose calls keep the tail a role of the finishing launch:
  // set by the first route that needs it (ensure_device), and stays set
  bool want_tail = false;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;      // around the dominant kernel (the caller's: dcrx_set_timing_events)
  hipEvent_t ev_step_start = nullptr, ev_step_stop = nullptr;  // around every launch of a call (the caller's)
  // the tuple sink (dcrx_set_tuple_sink): where the next calls leave their message
  bool sink_on = false;
  dcrx_tuple_layout_t sink_layout{};
  uint8_t *sink_msg = nullptr; uint64_t sink_slots = 0; uint64_t *sink_total = nullptr;
  MergeRows merge;
};

static int layout_dev(dcrx_tables *t, const dcrx_tuple_layout_t *L, TupleLayoutDev *D);
static int compact_workspace(uint64_t n_reads, uint32_t **tc, uint64_t **to);

static void free_device_state(dcrx_tables *t) {
  DeviceGuard on(t->state.device);
  t->state = DeviceState{};
}

static void free_merge_rows(dcrx_tables *t) {
  DeviceGuard on(t->merge.device);
  t->merge = MergeRows{};
}

// dcrx_merge.hip: one window row per gene (V rows, then J rows) out of the handle's regions, on the current device
int dcrx::merge_windows(dcrx_tables_t *t, const uint32_t **d_rows, uint32_t *n_v, uint32_t *n_j) {
  int dev = -1;
  HIP_TRY(hipGetDevice(&dev));
  if (t->merge.device != dev) {
    free_merge_rows(t);
    const uint32_t nv = t->host.g[0].n, nj = t->host.g[1].n;
    std::vector<uint32_t> rows((size_t)(nv + nj) * dcrx_merge::WIN_WORDS + 1, 0u);
    for (int g = 0; g < 2; g++)
      for (uint32_t k = 0; k < t->host.g[g].n; k++) {
        const std::string &r = t->host.g[g].regions[k];
        dcrx_merge::make_window(r.data(), (uint32_t)r.size(), g == 0, rows.data() + (size_t)((g ? nv : 0) + k) * dcrx_merge::WIN_WORDS);
      }
    if (int rc = t->merge.rows.alloc(rows.size())) return rc;
    HIP_TRY(hipMemcpy(t->merge.rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    t->merge.device = dev;
  }
  *d_rows = t->merge.rows; *n_v = t->host.g[0].n; *n_j = t->host.g[1].n;
  return DCRX_OK;
}

extern "C" {

int dcrx_abi_version(void) { return DCRX_ABI_VERSION; }
const char *dcrx_last_error(void) { return g_err.c_str(); }
const char *dcrx_build_info(void) { return "dcrx hip kernels: gfx950; v2 scan block 1024 (16-bit pair table), finishing blocks 256; reads <= 511 nt on register shapes of 10 / 20 / 32 words per read, 512 .. 65535 nt one read per lane from memory"; }

int dcrx_tables_create(const dcrx_tagset_t *tagset, dcrx_tables_t **out) {
  if (!out) return set_err(DCRX_E_INVALID, "out is null");
  *out = nullptr;
  dcrx_tables *t = new (std::nothrow) dcrx_tables();
  if (!t) return set_err(DCRX_E_NOMEM, "out of memory");
  std::string err;
  int rc;
  try { rc = compile_tables(tagset, &t->host, &err); }
  catch (...) { rc = DCRX_E_NOMEM; err = "out of memory while compiling the tag tables"; }
  if (rc != DCRX_OK) { delete t; return set_err(rc, err); }
  *out = t;
  return DCRX_OK;
}

void dcrx_tables_destroy(dcrx_tables_t *t) {
  if (!t) return;
  free_merge_rows(t);
  free_device_state(t);
  delete t;
}

int dcrx_tables_info(const dcrx_tables_t *t, dcrx_tables_info_t *info) {
  if (!t || !info) return set_err(DCRX_E_INVALID, "null argument");
  std::memset(info, 0, sizeof *info);
  info->n_v = t->host.g[0].n; info->n_j = t->host.g[1].n;
  info->n_states = t->host.n_states; info->dfa_bytes = t->host.dfa_bytes;
  for (int c = 0; c < 6; c++) info->n_keywords[c] = t->host.n_keywords[c];
  info->max_tag_len = t->host.max_tag_len;
  info->tables_in_lds = t->host.rel.lds_image_bytes + 128 <= 120 * 1024;
  info->equal_len_per_automaton = t->host.equal_len_per_automaton ? 1 : 0;
  info->pair_scan_bytes = t->host.rel.dfa16_bytes;
  info->v2_tables = t->host.rel.v2_ok;
  for (int o = 0; o < 2; o++) { info->v2_states[o] = t->host.rel.v2[o].n_states; info->v2_scan_bytes[o] = t->host.rel.v2[o].trans_bytes; }
  info->max_read_len = DCRX_MAX_READ_LEN;
  return DCRX_OK;
}

// ---- device plumbing ------------------------------------------------------------
int dcrx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int dcrx_set_device(int device) { HIP_TRY(hipSetDevice(device)); return DCRX_OK; }
int dcrx_device_name(char *buf, size_t cap) {
  if (!buf || !cap) return set_err(DCRX_E_INVALID, "null buffer");
  int dev = 0; HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t p; HIP_TRY(hipGetDeviceProperties(&p, dev));
  std::snprintf(buf, cap, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
  return DCRX_OK;
}
int dcrx_malloc_device(void **ptr, size_t bytes) {
  if (!ptr) return set_err(DCRX_E_INVALID, "null ptr");
  HIP_TRY(hipMalloc(ptr, bytes ? bytes : 16)); return DCRX_OK;
}
int dcrx_free_device(void *ptr) { HIP_TRY(hipFree(ptr)); return DCRX_OK; }
int dcrx_malloc_host(void **ptr, size_t bytes) {
  if (!ptr) return set_err(DCRX_E_INVALID, "null argument");
  *ptr = nullptr;
  HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
  return DCRX_OK;
}
int dcrx_free_host(void *ptr) { if (ptr) HIP_TRY(hipHostFree(ptr)); return DCRX_OK; }
int dcrx_memcpy_h2d(void *d, const void *h, size_t bytes) { HIP_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); return DCRX_OK; }
int dcrx_memcpy_d2h(void *h, const void *d, size_t bytes) { HIP_TRY(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); return DCRX_OK; }
int dcrx_memset_device(void *d, int value, size_t bytes) { HIP_TRY(hipMemset(d, value, bytes)); return DCRX_OK; }
int dcrx_synchronize(void) { HIP_TRY(hipDeviceSynchronize()); return DCRX_OK; }
int dcrx_event_create(void **ev) {
  if (!ev) return set_err(DCRX_E_INVALID, "null event");
  hipEvent_t e; HIP_TRY(hipEventCreate(&e)); *ev = e; return DCRX_OK;
}
int dcrx_event_destroy(void *ev) { HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return DCRX_OK; }
int dcrx_event_record(void *ev, void *stream) { HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return DCRX_OK; }
int dcrx_event_elapsed_ms(void *a, void *b, float *ms) {
  if (!ms) return set_err(DCRX_E_INVALID, "null ms");
  HIP_TRY(hipEventSynchronize((hipEvent_t)b));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
  return DCRX_OK;
}

}  // extern "C"

// ---- per-device state -------------------------------------------------------------
// the tables on the current device and the launch plan of that device: what a handle's first use of a device builds
static int first_use(const dcrx_tables *t, int dev, DeviceState *out) {
  DeviceState N;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  int rc;
  if ((rc = N.blob.alloc(t->host.blob.size()))) return rc;
  HIP_TRY(hipMemcpy(N.blob, t->host.blob.data(), t->host.blob.size(), hipMemcpyHostToDevice));
  N.dev = t->host.resolve(N.blob);
  if ((rc = N.d_dev.alloc(1))) return rc;
  HIP_TRY(hipMemcpy(N.d_dev, &N.dev, sizeof(DevTables), hipMemcpyHostToDevice));
  // launch plan: persistent blocks of DCRX_BLOCK threads, the DFA resident in LDS
  const uint32_t lds_cap = 160 * 1024;
  const uint32_t want = t->host.rel.lds_image_bytes + DCRX_N_COUNTERS * 4;
  LaunchPlan &P = N.plan;
  P.n_cu = (uint32_t)prop.multiProcessorCount;
  P.table_in_lds = want <= 120 * 1024;
  P.lds_bytes = P.table_in_lds ? want : DCRX_N_COUNTERS * 4;
  const uint32_t side_bytes = t->host.rel.lds_image_bytes - t->host.rel.dfa_bytes;
  P.lds16_bytes = DCRX_N_COUNTERS * 4 + t->host.rel.dfa16_bytes + side_bytes;
  P.table16_in_lds = P.table_in_lds && t->host.rel.dfa16_bytes != 0 && P.lds16_bytes + 32768 <= lds_cap;  // + wq and tail buffers of the 1024-thread block
  uint32_t per_cu = std::min<uint32_t>(2048 / DCRX_BLOCK, std::max<uint32_t>(1, lds_cap / std::max<uint32_t>(P.lds_bytes, 1)));
  P.grid = (uint32_t)prop.multiProcessorCount * std::max<uint32_t>(per_cu, 1);  // upper bound for either fast kernel
  const uint32_t q_per_cu = std::min<uint32_t>(2048 / DCRX_QBLOCK, std::max<uint32_t>(1, lds_cap / std::max<uint32_t>(P.lds_bytes, 1)));
  P.qgrid = (uint32_t)prop.multiProcessorCount * q_per_cu;
  P.reserved_cus = t->reserved_cus;
  P.tune_may_wait = t->tune_may_wait;
  N.device = dev;
  *out = std::move(N);
  return DCRX_OK;
}

// the handle's tables and plan are on the caller's current device
static int use_device(dcrx_tables *t) {
  int dev = -1;
  HIP_TRY(hipGetDevice(&dev));
  if (t->state.device == dev) return DCRX_OK;
  free_device_state(t);       // tables move with the caller's current device
  // (built aside and committed whole: a first use that fails part-way leaves the handle empty, and what it had allocated is freed)
  return first_use(t, dev, &t->state);
}

// the handle's workspace on its device holds batches of up to max_reads reads of this stride, and the tail list where
// want_tail says so (sizes kept in the plan say what is allocated; a list that failed to grow is gone and its size is zero)
static int grow_workspace(dcrx_tables *t, uint64_t max_reads, uint32_t stride) {
  DeviceState &S = t->state;
  LaunchPlan &P = S.plan;
  int rc;
  if (max_reads < 4096) max_reads = 4096;  // workspace exists even for empty batches
  if (max_reads > S.exc_flag_reads) {
    S.exc_flag_reads = 0;
    S.exc_flag.reset(); S.queue.reset();
    if ((rc = S.exc_flag.alloc(((max_reads + 31) / 32) + 4))) return rc;
    if ((rc = S.queue.alloc(3 * max_reads + DCRX_QUEUE_HEADER))) return rc;  // [work counters][rescue queue][general list][its exception-list offsets]
    S.exc_flag_reads = max_reads;
    t->ws_dirty = true;
  }
  if (t->host.rel.v2_ok && stride <= DCRX_FAST_MAX_STRIDE) {
    // the lists between the v2 kernels: every wave of the scan kernel (16 per CU) owns a region of tail and of event
    // entries; an entry carries the read's packed words, so the size follows the stride
    uint64_t tr = 0, er = 0;
    v2_list_rows(max_reads, stride, P.n_cu, &tr, &er);
    if (t->want_tail && tr > P.v2_tail_rows) {
      P.v2_tail_rows = 0;
      if ((rc = S.v2_tail.alloc(tr))) return rc;
      P.v2_tail_rows = tr;
    }
    if (er > P.v2_event_rows || v2_slow_rows(max_reads, stride, P.n_cu) > P.v2_slow_rows) {
      P.v2_event_rows = P.v2_slow_rows = 0;
      S.v2_events.reset(); S.v2_counts.reset(); S.v2_slow.reset();
      const uint64_t sr = v2_slow_rows(max_reads, stride, P.n_cu);
      if ((rc = S.v2_events.alloc(er)) || (rc = S.v2_slow.alloc(sr)) || (rc = S.v2_counts.alloc((size_t)P.n_cu * 16 * 4))) return rc;
      HIP_TRY(hipMemset(S.v2_counts, 0, (size_t)P.n_cu * 16 * 16));      // (no hint yet of a region's last share of tail reads: scan2_kernel, V2_L_TWHINT)
      if (!S.v2_acc) {
        if ((rc = S.v2_acc.alloc(DCRX_N_COUNTERS))) return rc;
        t->ws_dirty = true;
      }
      if (!S.v2_left) {      // V2_LEFT_CAP entries of 32-word reads, and a valid word per entry (zero between launches)
        const size_t left_rows = (size_t)1024 * ((1 + 2 * DCRX_V2_NWLONG + 3) / 4) + 1024 / 4;
        DevBuf<uint4> left;
        if ((rc = left.alloc(left_rows))) return rc;
        HIP_TRY(hipMemset(left, 0, left_rows * 16));
        S.v2_left = std::move(left);
      }
      P.v2_event_rows = er; P.v2_slow_rows = sr;
      if (!S.v2_side) {     // the two side streams (tail kernel; general form over list X) and the events that fork them off the caller's stream and join them back
        // (a device that gives no more streams or events: the launches then do without the side streams)
        if (S.v2_side.create() || S.v2_side2.create() || S.v2_ev_fork.create(false) || S.v2_ev_join.create(false) || S.v2_ev_join2.create(false)) {
          S.v2_side.reset(); S.v2_side2.reset();
        }
      }
    }
  }
  return DCRX_OK;
}

// The one place the plan's pointers come from: the owners, as they stand after whatever grow_workspace did (or could not do).
static void fill_plan(DeviceState &S) {
  LaunchPlan &P = S.plan;
  P.dev_tables = S.d_dev;
  P.tune = S.tune;
  P.v2_tail = S.v2_tail; P.v2_events = S.v2_events; P.v2_slow = S.v2_slow; P.v2_counts = S.v2_counts;
  P.v2_left = S.v2_left; P.v2_acc = S.v2_acc;
  P.v2_side = S.v2_side; P.v2_side2 = S.v2_side2;
  P.v2_ev_fork = S.v2_ev_fork; P.v2_ev_join = S.v2_ev_join; P.v2_ev_join2 = S.v2_ev_join2;
}

// cfg, uniform: the call the workspace is for, whose route (dcrx_route.h) comes back in *route; no call in hand
// (dcrx_reserve_device, the host-buffer pipeline, entries that only need the tables): either frame might be asked for, no flags
static int ensure_device(dcrx_tables *t, uint64_t max_reads, uint32_t stride = 40, hipStream_t stream = nullptr, const dcrx_cfg_t *cfg = nullptr,
                         bool uniform = true, Route *route = nullptr) {
  int rc = use_device(t);
  if (!rc) {
    auto ask = [&](int orientation, uint32_t flags) { return route_of(route_facts(t->state.plan, t->state.dev, stride, uniform, max_reads, orientation, flags)); };
    const Route R = cfg ? ask(cfg->orientation, cfg->flags) : ask(DCRX_ORIENT_REVERSE, 0);
    if (R.needs_tail_list || (!cfg && ask(DCRX_ORIENT_FORWARD, 0).needs_tail_list)) t->want_tail = true;
    if (route) *route = R;
    rc = grow_workspace(t, max_reads, stride);
  }
  DeviceState &S = t->state;
  fill_plan(S);
  if (rc) return rc;
  if (t->ws_dirty) {
    // the kernels leave the work counters and the exception bitmap zeroed; they are zeroed here
    // only once per allocation, or after a launch that failed part-way
    // on the stream the kernels will run on (a non-blocking stream does not order against the null stream)
    HIP_TRY(hipMemsetAsync(S.exc_flag, 0, ((S.exc_flag_reads + 31) / 32) * 4 + 16, stream));
    HIP_TRY(hipMemsetAsync(S.queue, 0, DCRX_QUEUE_HEADER * 4, stream));
    if (S.v2_acc) HIP_TRY(hipMemsetAsync(S.v2_acc, 0, DCRX_N_COUNTERS * 8, stream));
    // dcrx_reserve_device and the host-buffer entry come here with the null stream: the fills must have landed before a
    // later call's kernels start on a non-blocking stream of the caller's, which nothing orders against the null stream
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    t->ws_dirty = false;
  }
  return DCRX_OK;
}

// The device side of the tuple sink for batches of up to max_reads reads: the regions' slabs of items, their counters and
// the descriptor the kernels read (allocated on the first call that needs them, grown by a larger batch: synchronises).
static int ensure_sink(dcrx_tables *t, uint64_t max_reads, hipStream_t stream) {
  DeviceState &S = t->state;
  const uint64_t want = v2_sink_items(std::max<uint64_t>(max_reads, 4096), S.plan.n_cu);
  const uint32_t regions = S.plan.n_cu;
  if (S.sink && want <= S.sink_items_cap && regions <= S.sink_regions_cap) return DCRX_OK;
  HIP_TRY(hipStreamSynchronize(stream));
  S.sink_items.reset(); S.sink_ctr.reset(); S.sink.reset();
  S.sink_items_cap = 0; S.sink_regions_cap = 0;
  int rc;
  if ((rc = S.sink_items.alloc(want)) || (rc = S.sink_ctr.alloc((size_t)2 * regions + 16))) return rc;
  HIP_TRY(hipMemset(S.sink_ctr, 0, ((size_t)2 * regions + 16) * 4));
  if ((rc = S.sink.alloc(1))) return rc;
  V2SinkDev D;
  D.late = S.sink_ctr + regions; D.ticket = S.sink_ctr + 2 * regions;      // (the regions' counts of decombined reads in front: V2SinkCall::hits)
  D.j_tag_len = S.dev.g[1].tag_len; D.j_jump = S.dev.g[1].jump;
  HIP_TRY(hipMemcpy(S.sink, &D, sizeof D, hipMemcpyHostToDevice));
  S.sink_items_cap = want; S.sink_regions_cap = regions;
  return DCRX_OK;
}

static int check_batch(const dcrx_batch_t *b) {
  if (!b) return set_err(DCRX_E_INVALID, "batch is null");
  if (b->n_reads >= (1ull << 32)) return set_err(DCRX_E_INVALID, "more than 2^32-1 reads in one call");
  if (b->stride == 0 || (b->stride & 7u)) return set_err(DCRX_E_INVALID, "stride must be a positive multiple of 8");
  if (b->stride > DCRX_MAX_STRIDE) return set_err(DCRX_E_UNSUPPORTED, "stride > 16384 bytes: reads longer than 65535 nt are not supported");
  if (!b->lens && b->read_len > DCRX_MAX_READ_LEN) return set_err(DCRX_E_UNSUPPORTED, "reads longer than 65535 nt are not supported");
  if (!b->lens && b->read_len > 4 * b->stride) return set_err(DCRX_E_INVALID, "read_len exceeds 4*stride");
  if (b->n_reads && !b->packed) return set_err(DCRX_E_INVALID, "packed is null");
  if (b->n_exc && (!b->exc_read || !b->exc_pos || !b->exc_chr)) return set_err(DCRX_E_INVALID, "exception arrays are null");
  if (b->n_exc >= (1ull << 32)) return set_err(DCRX_E_INVALID, "more than 2^32-1 exception entries in one call");
  return DCRX_OK;
}

extern "C" {

int dcrx_set_timing_events(dcrx_tables_t *t, void *start_event, void *stop_event) {
  if (!t) return set_err(DCRX_E_INVALID, "tables is null");
  t->ev_start = (hipEvent_t)start_event; t->ev_stop = (hipEvent_t)stop_event;
  return DCRX_OK;
}

int dcrx_set_step_events(dcrx_tables_t *t, void *start_event, void *stop_event) {
  if (!t) return set_err(DCRX_E_INVALID, "tables is null");
  t->ev_step_start = (hipEvent_t)start_event; t->ev_step_stop = (hipEvent_t)stop_event;
  return DCRX_OK;
}

int dcrx_reserve_device(dcrx_tables_t *t, uint64_t max_reads) {
  if (!t) return set_err(DCRX_E_INVALID, "tables is null");
  return ensure_device(t, max_reads);
}

int dcrx_decombine_device(dcrx_tables_t *t, const dcrx_cfg_t *cfg, const dcrx_batch_t *b, dcrx_record_t *d_records,
                          uint64_t *d_counters, void *stream) {
  if (!t || !cfg || !d_counters) return set_err(DCRX_E_INVALID, "null argument");
  int rc = check_batch(b);
  if (rc) return rc;
  if (b->n_reads && !d_records) return set_err(DCRX_E_INVALID, "d_records is null");
  if (cfg->orientation < 0 || cfg->orientation > 2) return set_err(DCRX_E_INVALID, "orientation must be 0, 1 or 2");
  if (cfg->flags & DCRX_F_PROFILE_MASK) {       // profiling switches: the records are then not results
    if (!dcrx_debug_flags_on()) return set_err(DCRX_E_INVALID, "cfg.flags holds a profiling switch (records would not be results): set DCRX_DEBUG_FLAGS=1 to allow it");
  }
  Route route;      // what the call will launch, before anything is: the workspace is sized for it, and launch_decombine runs it
  rc = ensure_device(t, b->n_reads, b->stride, (hipStream_t)stream, cfg, b->lens == nullptr, &route);
  if (rc) return rc;
  BatchDev B;
  B.packed = b->packed; B.stride = b->stride; B.read_len = b->read_len; B.lens = b->lens;
  B.n_reads = b->n_reads; B.n_exc = b->n_exc; B.exc_read = b->exc_read; B.exc_pos = b->exc_pos;
  B.exc_chr = b->exc_chr; B.exc_flag = t->state.exc_flag;
  CfgDev C{cfg->orientation, cfg->allow_ns, cfg->lenthreshold, cfg->flags};
  t->state.plan.ev_step_start = t->ev_step_start; t->state.plan.ev_step_stop = t->ev_step_stop;
  // the call's tuple sink: the kernels' own (tuples of up to 40 bits, the shipped launch shape: launch_v2), else a compaction
  // of the records behind the call, on the same stream
  bool sink_done = false;
  t->state.plan.sink = V2SinkJob{};
  TupleLayoutDev LD{};
  if (t->sink_on) {
    if (t->sink_slots < b->n_reads) return set_err(DCRX_E_INVALID, "tuple sink: the message holds fewer read slots than the batch has reads");
    rc = layout_dev(t, &t->sink_layout, &LD);
    if (rc) return rc;
    // (v_start and j_end travel in w_pos bits each: a batch whose reads can be longer than those bits hold would spill into the
    // neighbouring fields of every tuple)
    const uint64_t longest = b->lens ? (uint64_t)b->stride * 4u : (uint64_t)b->read_len;
    if (LD.w_pos < 32 && (longest >> LD.w_pos) != 0)
      return set_err(DCRX_E_INVALID, b->lens ? "tuple sink: a batch with per-read lengths is priced at the longest read its stride holds (4 * stride bases: the lengths "
                                                "live in device memory); give dcrx_tuple_layout a max_read_len of 4 * stride for such batches"
                                              : "tuple sink: the batch's reads are longer than the layout's position fields hold (dcrx_tuple_layout's max_read_len)");
    if (t->sink_layout.bits <= 40 && t->host.rel.v2_ok && b->stride <= DCRX_FAST_MAX_STRIDE) {
      rc = ensure_sink(t, b->n_reads, (hipStream_t)stream);
      if (rc) return rc;
      V2SinkJob &J = t->state.plan.sink;
      J.dev = t->state.sink; J.items = static_cast<uint2 *>(t->state.sink_items); J.hits = t->state.sink_ctr; J.items_cap = t->state.sink_items_cap; J.regions_cap = t->state.sink_regions_cap;
      J.wpack = LD.w_v | (LD.w_j << 5) | (LD.w_vdel << 10) | (LD.w_jdel << 15) | (LD.w_pos << 20);
      J.bytes = LD.bytes; J.msg = t->sink_msg; J.n_slots = t->sink_slots; J.d_total = t->sink_total; J.done = &sink_done;
    }
  }
  const hipError_t le = launch_decombine(route, t->state.plan, t->state.dev, B, C, d_records, t->state.queue + DCRX_QUEUE_HEADER,
                                         t->state.queue + DCRX_QUEUE_HEADER + t->state.exc_flag_reads, t->state.queue, d_counters,
                                         (hipStream_t)stream, t->ev_start, t->ev_stop);
  t->state.plan.sink = V2SinkJob{};
  if (le != hipSuccess) { t->ws_dirty = true; return hip_fail(le, "launch_decombine"); }
  if (t->sink_on && !sink_done) {
    uint32_t *tc = nullptr; uint64_t *to = nullptr;
    rc = compact_workspace(b->n_reads, &tc, &to);
    if (rc) return rc;
    HIP_TRY(launch_compact_narrow(d_records, b->n_reads, t->sink_msg, t->sink_slots, LD, t->sink_total, tc, to, (hipStream_t)stream));
  }
  return DCRX_OK;
}

}  // extern "C"

// ---- the host-buffer entries ------------------------------------------------------------------------------------------

// host-side validation of a host batch that the device entry cannot afford (after check_batch)
static int check_host_batch(const dcrx_batch_t *hb) {
  const uint64_t n = hb->n_reads;
  if (hb->lens) {
    for (uint64_t r = 0; r < n; r++) {
      if (hb->lens[r] > 4 * hb->stride) return set_err(DCRX_E_INVALID, "a read is longer than 4*stride");
      if (hb->lens[r] > DCRX_MAX_READ_LEN) return set_err(DCRX_E_UNSUPPORTED, "a read is longer than 65535 nt");
    }
  }
  for (uint64_t i = 0; i < hb->n_exc; i++) {
    const uint8_t c = hb->exc_chr[i];
    if (c == 'A' || c == 'C' || c == 'G' || c == 'T') return set_err(DCRX_E_INVALID, "exception byte is one of ACGT");
    if (hb->exc_read[i] >= n) return set_err(DCRX_E_INVALID, "exception read index out of range");
    if (i && (hb->exc_read[i] < hb->exc_read[i - 1] ||
              (hb->exc_read[i] == hb->exc_read[i - 1] && hb->exc_pos[i] <= hb->exc_pos[i - 1])))
      return set_err(DCRX_E_INVALID, "exceptions are not sorted by (read, pos)");
    const uint32_t len = hb->lens ? hb->lens[hb->exc_read[i]] : hb->read_len;
    if (hb->exc_pos[i] >= len) return set_err(DCRX_E_INVALID, "exception position beyond the read");
  }
  return DCRX_OK;
}

// One chunk's staging: the input set (packed | lens | exc_read | exc_pos | exc_chr) and the output set (records |
// counters), offsets inside each set.  (long reads: a chunk's packed bytes stay within what 2 M reads of 150 nt take)
struct HostLayout {
  uint64_t chunk = 0;
  size_t o_lens = 0, o_er = 0, o_ep = 0, o_ec = 0, in_bytes = 0;
  size_t o_cnt = 0, out_bytes = 0;
};
static HostLayout host_layout(const dcrx_batch_t *hb) {
  HostLayout L;
  const uint64_t n = hb->n_reads;
  L.chunk = std::min<uint64_t>(std::max<uint64_t>(n, 1), std::max<uint64_t>(1024, std::min<uint64_t>(DCRX_HOST_CHUNK, ((uint64_t)DCRX_HOST_CHUNK * 40) / hb->stride)));
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  uint64_t max_exc = 0;       // the most exception entries any chunk holds
  uint64_t e = 0;
  for (uint64_t c0 = 0; c0 < n; c0 += L.chunk) {
    const uint64_t e0 = e;
    while (e < hb->n_exc && hb->exc_read[e] < c0 + L.chunk) e++;
    max_exc = std::max(max_exc, e - e0);
  }
  L.o_lens = al(L.chunk * hb->stride + 16);
  L.o_er = L.o_lens + al(hb->lens ? L.chunk * 2 : 0);
  L.o_ep = L.o_er + al(max_exc * 4);
  L.o_ec = L.o_ep + al(max_exc * 2);
  L.in_bytes = L.o_ec + al(max_exc);
  L.o_cnt = al(L.chunk * sizeof(dcrx_record_t));
  L.out_bytes = L.o_cnt + al(DCRX_N_COUNTERS * 8);
  return L;
}

// the handle's staging buffers hold at least `bytes`, on the device and pinned on the host
static int ensure_staging(dcrx_tables *t, size_t bytes) {
  DeviceState &S = t->state;
  int rc;
  if (bytes > S.stage_bytes) {
    S.stage_bytes = 0;
    if ((rc = S.d_stage.alloc(bytes))) return rc;
    S.stage_bytes = bytes;
  }
  if (bytes > S.h_stage_bytes) {
    S.h_stage_bytes = 0;
    if ((rc = S.h_stage.alloc(bytes))) return rc;
    S.h_stage_bytes = bytes;
  }
  return DCRX_OK;
}

// the handle's host-entry streams that a call asks for (each made once), and the events that order them
static int ensure_host_streams(dcrx_tables *t, bool in, bool run, bool out) {
  DeviceState &S = t->state;
  int rc;
  if (in && !S.hs_in && (rc = S.hs_in.create())) return rc;
  if (run && !S.hs_run && (rc = S.hs_run.create())) return rc;
  if (out && !S.hs_out && (rc = S.hs_out.create())) return rc;
  for (Event *set : {S.hev_in, S.hev_run, S.hev_out})
    for (int k = 0; k < 2; k++)
      if (!set[k] && (rc = set[k].create(false))) return rc;
  return DCRX_OK;
}

// Buffers the caller has pinned (dcrx_malloc_host, hipHostMalloc, hipHostRegister) are copied from and to directly: the
// staging copies — half of a call's time from pageable memory — fall away for them.
static bool host_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

// The chunk pipeline of the host-buffer entries, over nc = 1 .. DCRX_MAX_CHAINS handles (arguments checked by host_entry);
// chain c fills records[c], or counts[c] (the chunks' records then stay on the device and feed it, only the counters come
// back).  The batch goes through in chunks of DCRX_HOST_CHUNK reads, three streams deep: while the kernels of chunk k run,
// chunk k + 1 is copied in and the records of chunk k - 1 are copied out (PCIe is full duplex: 40 bytes per read one way,
// 16 the other), through pinned staging buffers (a copy from pageable memory would not overlap anything).  Each chunk is
// copied in once, on T[0]'s copy-in stream, into the input sets of T[0]'s staging, in front of its output sets; every
// other handle's staging holds only its output sets.  Each chain's launches run on its handle's run stream.  The loop it
// stands for is the reference's read loop (decombine.py:963-1050).
static int host_pipeline(dcrx_tables *const *T, uint32_t nc, const dcrx_cfg_t *cfg, const dcrx_batch_t *hb,
                         dcrx_record_t *const *records, uint64_t *const *counters, dcrx_counts_t *const *counts,
                         uint64_t first_index, const uint32_t *index) {
  const uint64_t n = hb->n_reads;
  const HostLayout Lay = host_layout(hb);
  const uint64_t chunk = Lay.chunk;
  int rc;
  for (uint32_t c = 0; c < nc; c++) {
    rc = ensure_device(T[c], chunk, hb->stride);
    if (rc) return rc;
    rc = ensure_staging(T[c], (c == 0 ? 2 * Lay.in_bytes : 0) + 2 * Lay.out_bytes);
    if (rc) return rc;
    rc = ensure_host_streams(T[c], c == 0, true, nc == 1);
    if (rc) return rc;
    for (int k = 0; k < DCRX_N_COUNTERS; k++) counters[c][k] = 0;
  }
  hipStream_t s_in = T[0]->state.hs_in;
  auto out_at = [&](uint32_t c, int set) { return (c == 0 ? 2 * Lay.in_bytes : 0) + (size_t)set * Lay.out_bytes; };
  const bool in_direct = n && host_pinned(hb->packed) && host_pinned(hb->packed + (size_t)n * hb->stride - 1);
  bool out_direct[DCRX_MAX_CHAINS];
  for (uint32_t c = 0; c < nc; c++)
    out_direct[c] = n && !counts && host_pinned(records[c]) && host_pinned(reinterpret_cast<const uint8_t *>(records[c] + n) - 1);
  const uint64_t n_chunks = n ? (n + chunk - 1) / chunk : 1;
  uint64_t exc_at = 0;
  auto drain = [&](uint64_t k) -> int {       // chunk k's records and counters of every chain: pinned buffers to the caller's
    const int set = (int)(k & 1);
    const uint64_t c0 = k * chunk, cn = std::min<uint64_t>(chunk, n - c0);
    for (uint32_t c = 0; c < nc; c++) {
      HIP_TRY(hipEventSynchronize(T[c]->state.hev_out[set]));
      const uint8_t *h = T[c]->state.h_stage + out_at(c, set);
      if (cn && !out_direct[c] && !counts) par_memcpy(records[c] + c0, h, cn * sizeof(dcrx_record_t));
      const uint64_t *hc = reinterpret_cast<const uint64_t *>(h + Lay.o_cnt);
      for (int i = 0; i < DCRX_N_COUNTERS; i++) counters[c][i] += hc[i];
    }
    return DCRX_OK;
  };
  for (uint64_t k = 0; k < n_chunks; k++) {
    const int set = (int)(k & 1);
    const uint64_t c0 = k * chunk, cn = n ? std::min<uint64_t>(chunk, n - c0) : 0;
    uint8_t *h = T[0]->state.h_stage + (size_t)set * Lay.in_bytes, *d = T[0]->state.d_stage + (size_t)set * Lay.in_bytes;
    // chunk k - 2's records leave the pinned buffers on a helper thread while this thread fills the input set (several
    // threads: one memcpy does not keep up with the link; the input and output sets do not overlap), once the copy in of
    // chunk k - 2, which read the same bytes, is over
    int drc = DCRX_OK;
    std::thread helper;
    if (k >= 2) helper = std::thread([&, k] { drc = drain(k - 2); });
    struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join_helper{helper};
    if (k >= 2) HIP_TRY(hipEventSynchronize(T[0]->state.hev_in[set]));
    const uint64_t e0 = exc_at;
    while (exc_at < hb->n_exc && hb->exc_read[exc_at] < c0 + cn) exc_at++;
    const uint64_t ne = exc_at - e0;
    if (cn && !in_direct) par_memcpy(h, hb->packed + c0 * hb->stride, cn * hb->stride);
    if (hb->lens && cn) std::memcpy(h + Lay.o_lens, hb->lens + c0, cn * 2);
    uint32_t *her = reinterpret_cast<uint32_t *>(h + Lay.o_er);
    for (uint64_t i = 0; i < ne; i++) her[i] = hb->exc_read[e0 + i] - (uint32_t)c0;      // read indices inside the chunk
    if (ne) { std::memcpy(h + Lay.o_ep, hb->exc_pos + e0, ne * 2); std::memcpy(h + Lay.o_ec, hb->exc_chr + e0, ne); }
    if (helper.joinable()) helper.join();
    if (drc) return drc;
    // copy in, once every chain's kernels that read this input set (chunk k - 2) are over
    if (k >= 2)
      for (uint32_t c = 0; c < nc; c++) HIP_TRY(hipStreamWaitEvent(s_in, T[c]->state.hev_run[set], 0));
    if (in_direct) {
      HIP_TRY(hipMemcpyAsync(d, hb->packed + c0 * hb->stride, cn * hb->stride, hipMemcpyHostToDevice, s_in));
      if (Lay.in_bytes > Lay.o_lens) HIP_TRY(hipMemcpyAsync(d + Lay.o_lens, h + Lay.o_lens, Lay.in_bytes - Lay.o_lens, hipMemcpyHostToDevice, s_in));
    } else {
      HIP_TRY(hipMemcpyAsync(d, h, Lay.in_bytes, hipMemcpyHostToDevice, s_in));
    }
    HIP_TRY(hipEventRecord(T[0]->state.hev_in[set], s_in));
    dcrx_batch_t db = *hb;
    db.n_reads = cn;
    db.packed = d;
    db.lens = hb->lens ? reinterpret_cast<const uint16_t *>(d + Lay.o_lens) : nullptr;
    db.n_exc = ne;
    db.exc_read = reinterpret_cast<const uint32_t *>(d + Lay.o_er);
    db.exc_pos = reinterpret_cast<const uint16_t *>(d + Lay.o_ep);
    db.exc_chr = d + Lay.o_ec;
    // every chain: kernels, then its copy out
    for (uint32_t c = 0; c < nc; c++) {
      dcrx_tables *t = T[c];
      // (one chain: the handle's out stream, beside the next chunk's kernels; several: behind the chain's kernels)
      const hipStream_t s_out = nc == 1 ? t->state.hs_out : t->state.hs_run;
      uint8_t *od = t->state.d_stage + out_at(c, set), *oh = t->state.h_stage + out_at(c, set);
      HIP_TRY(hipStreamWaitEvent(t->state.hs_run, T[0]->state.hev_in[set], 0));
      // (the records of chunk k - 2 have left this output set: a copy out on the run stream itself is ordered already)
      if (k >= 2 && s_out != t->state.hs_run) HIP_TRY(hipStreamWaitEvent(t->state.hs_run, t->state.hev_out[set], 0));
      rc = dcrx_decombine_device(t, cfg, &db, reinterpret_cast<dcrx_record_t *>(od), reinterpret_cast<uint64_t *>(od + Lay.o_cnt), t->state.hs_run);
      if (rc) return rc;          // (host_entry drains the streams)
      if (counts && cn) {         // the count step reads the packed chunk too: it is among what the next refill of the set waits for
        rc = count_chunk(counts[c], reinterpret_cast<const dcrx_record_t *>(od), &db, index ? first_index : first_index + c0,
                         index ? index + c0 : nullptr, t->state.hs_run);
        if (rc) return rc;
      }
      HIP_TRY(hipEventRecord(t->state.hev_run[set], t->state.hs_run));
      if (s_out != t->state.hs_run) HIP_TRY(hipStreamWaitEvent(s_out, t->state.hev_run[set], 0));
      if (out_direct[c] || counts) {
        if (cn && !counts) HIP_TRY(hipMemcpyAsync(records[c] + c0, od, cn * sizeof(dcrx_record_t), hipMemcpyDeviceToHost, s_out));
        HIP_TRY(hipMemcpyAsync(oh + Lay.o_cnt, od + Lay.o_cnt, Lay.out_bytes - Lay.o_cnt, hipMemcpyDeviceToHost, s_out));
      } else {
        HIP_TRY(hipMemcpyAsync(oh, od, Lay.out_bytes, hipMemcpyDeviceToHost, s_out));
      }
      HIP_TRY(hipEventRecord(t->state.hev_out[set], s_out));
    }
  }
  for (uint64_t k = n_chunks >= 2 ? n_chunks - 2 : 0; k < n_chunks; k++) { rc = drain(k); if (rc) return rc; }
  // (include/dcrx_codes.h: a wave that gave up waiting for another says so in the call's counters — the records would not be
  // complete, and this entry, which has the counters in hand, does not return them as if they were)
  for (uint32_t c = 0; c < nc; c++)
    if (counters[c][DCRX_C_DEVICE_ERRORS]) return set_err(DCRX_E_HIP, "a device-side wait timed out (the fused scan's ring): the records of this call are incomplete");
  if (counts)
    for (uint32_t c = 0; c < nc; c++) { rc = count_settle(counts[c], T[c]->state.hs_run); if (rc) return rc; }
  return DCRX_OK;
}

// The one epilogue of the four host-buffer entries.  Whatever goes wrong inside the chunk pipeline — a HIP error, no memory,
// a helper thread that cannot be started — comes back as a code, and only after every stream of every handle has drained:
// their asynchronous copies may target the caller's own (pinned) `packed` and `records` buffers, which the caller is free to
// release once this returns.  (The tuple sink concerns the device entry: a chunked host call has no one message.)
static int host_entry(dcrx_tables_t *const *T, uint32_t nc, const dcrx_cfg_t *cfg, const dcrx_batch_t *hb,
                      dcrx_record_t *const *records, uint64_t *const *counters, dcrx_counts_t *const *counts,
                      uint64_t first_index, const uint32_t *index) {
  if (!T || !cfg || (!records && !counts) || !counters) return set_err(DCRX_E_INVALID, "null argument");
  if (nc == 0 || nc > DCRX_MAX_CHAINS) return set_err(DCRX_E_INVALID, "n_chains must be 1 .. DCRX_MAX_CHAINS");
  for (uint32_t c = 0; c < nc; c++) {
    if (!T[c]) return set_err(DCRX_E_INVALID, "tables[c] is null");
    for (uint32_t e = 0; e < c; e++)
      if (T[e] == T[c]) return set_err(DCRX_E_INVALID, "the same tables handle twice: every chain needs a handle (and a workspace) of its own");
  }
  if (counts)
    for (uint32_t c = 0; c < nc; c++) {
      if (!counts[c]) return set_err(DCRX_E_INVALID, "counts[c] is null");
      for (uint32_t e = 0; e < c; e++)
        if (counts[e] == counts[c]) return set_err(DCRX_E_INVALID, "the same counts handle twice: every chain needs a table of its own");
    }
  int rc = check_batch(hb);
  if (rc) return rc;
  for (uint32_t c = 0; c < nc; c++) {
    if (!counters[c]) return set_err(DCRX_E_INVALID, "counters[c] is null");
    if (hb->n_reads && !counts && !records[c]) return set_err(DCRX_E_INVALID, "records[c] is null");
  }
  rc = check_host_batch(hb);
  if (rc) return rc;
  bool sink_was_on[DCRX_MAX_CHAINS];
  for (uint32_t c = 0; c < nc; c++) { sink_was_on[c] = T[c]->sink_on; T[c]->sink_on = false; }
  try { rc = host_pipeline(T, nc, cfg, hb, records, counters, counts, first_index, index); }
  catch (const std::bad_alloc &) { rc = set_err(DCRX_E_NOMEM, "out of host memory in the host-buffer entry"); }
  catch (const std::exception &e) { rc = set_err(DCRX_E_NOMEM, std::string("host-buffer entry: ") + e.what()); }
  catch (...) { rc = set_err(DCRX_E_NOMEM, "host-buffer entry: unexpected exception"); }
  if (rc != DCRX_OK) {
    const std::string keep = g_err;       // (the synchronising calls must not replace the message of what failed)
    for (uint32_t c = 0; c < nc; c++) {
      dcrx_tables *t = T[c];
      if (t->state.hs_in) (void)hipStreamSynchronize(t->state.hs_in);
      if (t->state.hs_run) (void)hipStreamSynchronize(t->state.hs_run);
      if (t->state.hs_out) (void)hipStreamSynchronize(t->state.hs_out);
      t->ws_dirty = true;
    }
    (void)hipGetLastError();
    g_err = keep;
  }
  for (uint32_t c = 0; c < nc; c++) T[c]->sink_on = sink_was_on[c];
  return rc;
}

extern "C" {

int dcrx_decombine(dcrx_tables_t *t, const dcrx_cfg_t *cfg, const dcrx_batch_t *hb, dcrx_record_t *records,
                   uint64_t *counters) {
  if (!t || !cfg || !counters) return set_err(DCRX_E_INVALID, "null argument");
  return host_entry(&t, 1, cfg, hb, &records, &counters, nullptr, 0, nullptr);
}

int dcrx_decombine_count(dcrx_tables_t *t, const dcrx_cfg_t *cfg, const dcrx_batch_t *hb, dcrx_counts_t *counts,
                         uint64_t first_index, const uint32_t *index, uint64_t *counters) {
  if (!counts) return set_err(DCRX_E_INVALID, "counts is null");
  if (!t || !cfg || !counters) return set_err(DCRX_E_INVALID, "null argument");
  return host_entry(&t, 1, cfg, hb, nullptr, &counters, &counts, first_index, index);
}

int dcrx_decombine_chains(dcrx_tables_t *const *tables, uint32_t n_chains, const dcrx_cfg_t *cfg,
                          const dcrx_batch_t *hb, dcrx_record_t *const *records, uint64_t *const *counters) {
  if (!records) return set_err(DCRX_E_INVALID, "null argument");
  return host_entry(tables, n_chains, cfg, hb, records, counters, nullptr, 0, nullptr);
}

int dcrx_decombine_chains_count(dcrx_tables_t *const *tables, uint32_t n_chains, const dcrx_cfg_t *cfg,
                                const dcrx_batch_t *hb, dcrx_counts_t *const *counts, uint64_t first_index,
                                const uint32_t *index, uint64_t *const *counters) {
  if (!counts) return set_err(DCRX_E_INVALID, "null argument");
  return host_entry(tables, n_chains, cfg, hb, nullptr, counters, counts, first_index, index);
}

}  // extern "C"

// tile counts and offsets of a compaction: a process-wide slot keyed by device (compaction does not need tables)
static int compact_workspace(uint64_t n_reads, uint32_t **tc, uint64_t **to) {
  struct Slot { int dev = -1; DevBuf<uint32_t> tc; DevBuf<uint64_t> to; uint64_t cap = 0; };
  // One slot per thread, on the heap and never deleted: a thread_local (or static) Slot would run hipFree from a thread-exit
  // or process-exit destructor, when the HIP runtime may already be gone.  What a thread's last slot holds goes with the process.
  static thread_local Slot *const slot = new (std::nothrow) Slot;
  if (!slot) return set_err(DCRX_E_NOMEM, "out of memory");
  Slot &ws = *slot;
  int dev = -1; HIP_TRY(hipGetDevice(&dev));
  if (ws.dev != dev || n_reads > ws.cap) {
    { DeviceGuard on(ws.dev); ws = Slot{}; }
    const size_t tiles = compact_tiles(n_reads) + 1024;
    Slot N;
    int rc;
    if ((rc = N.tc.alloc(tiles)) || (rc = N.to.alloc(tiles))) return rc;
    N.dev = dev; N.cap = n_reads;
    ws = std::move(N);
  }
  *tc = ws.tc; *to = ws.to;
  return DCRX_OK;
}

static int compact_hits(const dcrx_record_t *d_records, uint64_t n_reads, uint64_t first_index, dcrx_record_t *d_hits,
                        uint64_t *d_hit_index, uint64_t *d_ok_bitmap, int packed12, uint64_t *d_n_hits, void *stream) {
  if (!d_n_hits || (n_reads && (!d_records || !d_hits || (!d_hit_index && !d_ok_bitmap)))) return set_err(DCRX_E_INVALID, "null argument");
  uint32_t *tc = nullptr; uint64_t *to = nullptr;
  int rc = compact_workspace(n_reads, &tc, &to);
  if (rc) return rc;
  HIP_TRY(launch_compact(d_records, n_reads, first_index, d_hits, d_hit_index, d_ok_bitmap, packed12, d_n_hits, tc, to,
                         (hipStream_t)stream));
  return DCRX_OK;
}

extern "C" {

int dcrx_compact_hits_device(const dcrx_record_t *d_records, uint64_t n_reads, uint64_t first_index,
                             dcrx_record_t *d_hits, uint64_t *d_hit_index, uint64_t *d_n_hits, void *stream) {
  if (n_reads && !d_hit_index) return set_err(DCRX_E_INVALID, "null argument");
  return compact_hits(d_records, n_reads, first_index, d_hits, d_hit_index, nullptr, 0, d_n_hits, stream);
}

int dcrx_compact_hits_bitmap_device(const dcrx_record_t *d_records, uint64_t n_reads, dcrx_record_t *d_hits,
                                    uint64_t *d_ok_bitmap, uint64_t *d_n_hits, void *stream) {
  if (n_reads && !d_ok_bitmap) return set_err(DCRX_E_INVALID, "null argument");
  return compact_hits(d_records, n_reads, 0, d_hits, nullptr, d_ok_bitmap, 0, d_n_hits, stream);
}

int dcrx_compact_hits_packed_device(const dcrx_record_t *d_records, uint64_t n_reads, void *d_tuples12,
                                    uint64_t *d_ok_bitmap, uint64_t *d_n_hits, void *stream) {
  if (n_reads && !d_ok_bitmap) return set_err(DCRX_E_INVALID, "null argument");
  return compact_hits(d_records, n_reads, 0, reinterpret_cast<dcrx_record_t *>(d_tuples12), nullptr, d_ok_bitmap, 1, d_n_hits, stream);
}

int dcrx_compact_hits_packed8_device(const dcrx_record_t *d_records, uint64_t n_reads, void *d_tuples8,
                                     uint64_t *d_ok_bitmap, uint64_t *d_n_hits, void *stream) {
  if (n_reads && !d_ok_bitmap) return set_err(DCRX_E_INVALID, "null argument");
  return compact_hits(d_records, n_reads, 0, reinterpret_cast<dcrx_record_t *>(d_tuples8), nullptr, d_ok_bitmap, 2, d_n_hits, stream);
}

static uint8_t bits_of(uint64_t x) { uint8_t b = 1; while (b < 64 && (x >> b)) b++; return b; }   // bits that hold 0..x (at least one)

int dcrx_tuple_layout(const dcrx_tables_t *t, uint32_t max_read_len, dcrx_tuple_layout_t *L) {
  if (!t || !L) return set_err(DCRX_E_INVALID, "null argument");
  std::memset(L, 0, sizeof *L);
  const GeneHost &V = t->host.g[0], &J = t->host.g[1];
  int64_t max_vdel = 0, max_jdel = 0;
  for (uint32_t k = 0; k < V.n; k++) max_vdel = std::max<int64_t>(max_vdel, (int64_t)V.jumps[k] - (int64_t)V.tags[k].size());
  for (uint32_t k = 0; k < J.n; k++) max_jdel = std::max<int64_t>(max_jdel, (int64_t)J.jumps[k]);
  // (a record's vdel / jdel are bytes: deletions beyond 255 never reach a record)
  L->w_v = bits_of(V.n ? V.n - 1 : 0); L->w_j = bits_of(J.n ? J.n - 1 : 0);
  L->w_vdel = bits_of((uint64_t)std::min<int64_t>(max_vdel, 255)); L->w_jdel = bits_of((uint64_t)std::min<int64_t>(max_jdel, 255));
  L->w_pos = bits_of(max_read_len);
  const uint32_t bits = L->w_v + L->w_j + L->w_vdel + L->w_jdel + 2u * L->w_pos + 2u;
  L->max_read_len = max_read_len;
  if (bits > 64) return set_err(DCRX_E_UNSUPPORTED, "narrow tuple wider than 64 bits");
  L->bits = (uint8_t)bits;
  L->bytes = (uint8_t)std::max<uint32_t>(4, (bits + 7) / 8);
  return DCRX_OK;
}

uint64_t dcrx_tuple_message_bytes(const dcrx_tuple_layout_t *L, uint64_t n_reads, uint64_t n_hits) {
  if (!L) return 0;
  return ((n_reads + 63) / 64) * 8 + n_hits * L->bytes;
}

// the layout as a caller handed it back: what dcrx_tuple_layout would say for these tables
static int layout_dev(dcrx_tables *t, const dcrx_tuple_layout_t *L, TupleLayoutDev *D) {
  dcrx_tuple_layout_t want;
  int rc = dcrx_tuple_layout(t, L->max_read_len, &want);
  if (rc) return rc;
  if (std::memcmp(&want, L, sizeof want) != 0) return set_err(DCRX_E_INVALID, "tuple layout does not belong to these tables");
  D->w_v = L->w_v; D->w_j = L->w_j; D->w_vdel = L->w_vdel; D->w_jdel = L->w_jdel; D->w_pos = L->w_pos; D->bytes = L->bytes;
  D->j_tag_len = t->state.dev.g[1].tag_len; D->j_jump = t->state.dev.g[1].jump;
  return DCRX_OK;
}

int dcrx_compact_hits_narrow_device(dcrx_tables_t *t, const dcrx_tuple_layout_t *L, const dcrx_record_t *d_records,
                                    uint64_t n_reads, uint64_t n_slots, void *d_message, uint64_t *d_n_hits, void *stream) {
  if (!t || !L || !d_n_hits || (n_reads && !d_records) || (n_slots && !d_message)) return set_err(DCRX_E_INVALID, "null argument");
  if (n_slots < n_reads) return set_err(DCRX_E_INVALID, "n_slots < n_reads");
  try {
    int rc = ensure_device(t, 0, 40, (hipStream_t)stream);
    if (rc) return rc;
    TupleLayoutDev D;
    rc = layout_dev(t, L, &D);
    if (rc) return rc;
    uint32_t *tc = nullptr; uint64_t *to = nullptr;
    rc = compact_workspace(n_reads, &tc, &to);
    if (rc) return rc;
    HIP_TRY(launch_compact_narrow(d_records, n_reads, static_cast<uint8_t *>(d_message), n_slots, D, d_n_hits, tc, to, (hipStream_t)stream));
  } catch (const std::exception &e) {
    return set_err(DCRX_E_NOMEM, e.what());
  }
  return DCRX_OK;
}

int dcrx_set_tuple_sink(dcrx_tables_t *t, const dcrx_tuple_layout_t *L, void *d_message, uint64_t n_slots, uint64_t *d_n_hits) {
  if (!t) return set_err(DCRX_E_INVALID, "tables is null");
  if (!L) { t->sink_on = false; t->sink_msg = nullptr; t->sink_slots = 0; t->sink_total = nullptr; return DCRX_OK; }
  if (!d_message || !d_n_hits || !n_slots) return set_err(DCRX_E_INVALID, "null argument");
  dcrx_tuple_layout_t want;
  int rc = dcrx_tuple_layout(t, L->max_read_len, &want);
  if (rc) return rc;
  if (std::memcmp(&want, L, sizeof want) != 0) return set_err(DCRX_E_INVALID, "tuple layout does not belong to these tables");
  t->sink_on = true; t->sink_layout = *L;
  t->sink_msg = static_cast<uint8_t *>(d_message); t->sink_slots = n_slots; t->sink_total = d_n_hits;
  return DCRX_OK;
}

int dcrx_tune_state(const dcrx_tables_t *t, int orientation, uint64_t n_reads, dcrx_tune_state_t *out) {
  if (!t || !out) return set_err(DCRX_E_INVALID, "null argument");
  *out = dcrx_tune_state_t{0u, 0u, 0.f, 0.f, 0u, 0u};
  const V2Tune &F = t->state.tune[orientation == DCRX_ORIENT_FORWARD ? 0 : 1];
  out->launch_form = F.last_form;
  uint32_t first, second;
  V2Tune::candidates(n_reads, first, second);
  out->candidates = first | (second << 16);
  const int k = V2Tune::size_class(n_reads);
  if (k < 0) return DCRX_OK;
  const V2TuneSlot &U = F.slot[k];
  out->rescue_waves = U.choice; out->launches = (uint32_t)U.launches; out->us_first = U.us[0]; out->us_second = U.us[1];
  return DCRX_OK;
}

int dcrx_set_tune_wait(dcrx_tables_t *t, int allow) {
  if (!t) return set_err(DCRX_E_INVALID, "tables is null");
  t->tune_may_wait = allow != 0;
  t->state.plan.tune_may_wait = t->tune_may_wait;
  return DCRX_OK;
}

int dcrx_set_reserved_cus(dcrx_tables_t *t, uint32_t n_cus) {
  if (!t) return set_err(DCRX_E_INVALID, "tables is null");
  t->reserved_cus = n_cus;
  t->state.plan.reserved_cus = n_cus;
  return DCRX_OK;
}

// ---- host-side packing --------------------------------------------------------------
extern "C++" {
// Packs one read: 16 bases per step through a byte table whose top bit marks a byte that is
// not one of "ACGT"; such a word is redone base by base to record the exception entries.
namespace {
struct PackCode {
  uint8_t t[256];
  PackCode() {
    for (int c = 0; c < 256; c++) t[c] = 0x80;
    t[(int)'A'] = 0; t[(int)'C'] = 1; t[(int)'G'] = 2; t[(int)'T'] = 3;
  }
};
const PackCode g_pack_code;

struct ExcEntry { uint32_t read; uint16_t pos; uint8_t chr; };

inline void pack_one(const uint8_t *s, uint32_t len, uint8_t *out, uint32_t stride, uint32_t r, std::vector<ExcEntry> &exc) {
  const uint8_t *t = g_pack_code.t;
  uint32_t *ow = reinterpret_cast<uint32_t *>(out);
  const uint32_t nwords = stride / 4, full = len / 16;
  uint32_t k = 0;
  for (; k < full; k++) {
    const uint8_t *b = s + 16 * k;
    uint32_t w = 0, bad = 0;
    for (int i = 0; i < 16; i++) { const uint32_t c = t[b[i]]; bad |= c; w |= (c & 3u) << (2 * i); }
    if (bad & 0x80u)
      for (int i = 0; i < 16; i++)
        if (t[b[i]] & 0x80u) exc.push_back(ExcEntry{r, (uint16_t)(16 * k + i), b[i]});
    ow[k] = w;
  }
  if (len & 15u) {
    const uint8_t *b = s + 16 * k;
    uint32_t w = 0;
    for (uint32_t i = 0; i < (len & 15u); i++) {
      const uint32_t c = t[b[i]];
      if (c & 0x80u) exc.push_back(ExcEntry{r, (uint16_t)(16 * k + i), b[i]});
      w |= (c & 3u) << (2 * i);
    }
    ow[k++] = w;
  }
  for (; k < nwords; k++) ow[k] = 0;
}

// start/len accessors differ between the two entry points; everything else is shared.  Reads are
// split into contiguous ranges over a few threads; the ranges' exception lists are concatenated
// in range order, which keeps the list sorted by read.
template <class Span>
int64_t pack_all(const char *ascii, const Span &span, uint64_t n_reads, uint32_t stride, uint8_t *packed, uint16_t *lens,
                 uint32_t *exc_read, uint16_t *exc_pos, uint8_t *exc_chr, uint64_t exc_cap) {
  if ((n_reads && (!ascii || !packed)) || stride == 0 || (stride & 7u)) return set_err(DCRX_E_INVALID, "bad argument to the read packer");
  if (n_reads > 0xFFFFFFFFull) return set_err(DCRX_E_INVALID, "more than 2^32-1 reads in one batch");
  unsigned nt = 1;
  if (n_reads >= (1u << 16)) {
    nt = std::thread::hardware_concurrency();
    if (const char *e = std::getenv("DCRX_HOST_THREADS")) nt = (unsigned)std::atoi(e);
    if (nt < 1) nt = 1;
    if (nt > 16) nt = 16;
  }
  std::vector<std::vector<ExcEntry>> exc(nt);
  std::vector<int> bad(nt, 0);
  auto work = [&](unsigned k) {
    const uint64_t lo = n_reads * k / nt, hi = n_reads * (k + 1) / nt;
    for (uint64_t r = lo; r < hi; r++) {
      const uint64_t len = span.len(r);
      if (len > 4ull * stride || len > 65535) { bad[k] = 1; return; }
      if (lens) lens[r] = (uint16_t)len;
      pack_one(reinterpret_cast<const uint8_t *>(ascii) + span.start(r), (uint32_t)len, packed + r * (uint64_t)stride, stride,
               (uint32_t)r, exc[k]);
    }
  };
  if (nt == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; k++) th.emplace_back(work, k);
    for (auto &x : th) x.join();
  }
  for (unsigned k = 0; k < nt; k++) if (bad[k]) return set_err(DCRX_E_INVALID, "read longer than 4*stride");
  uint64_t n_exc = 0;
  for (unsigned k = 0; k < nt; k++)
    for (const ExcEntry &e : exc[k]) {
      if (n_exc < exc_cap && exc_read) { exc_read[n_exc] = e.read; exc_pos[n_exc] = e.pos; exc_chr[n_exc] = e.chr; }
      n_exc++;
    }
  return (int64_t)n_exc;
}
struct SpanOffsets { const uint64_t *o; uint64_t start(uint64_t r) const { return o[r]; } uint64_t len(uint64_t r) const { return o[r + 1] - o[r]; } };
struct SpanStartLen { const uint64_t *s; const uint32_t *l; uint64_t start(uint64_t r) const { return s[r]; } uint64_t len(uint64_t r) const { return l[r]; } };
}  // namespace

}  // extern "C++"

int64_t dcrx_pack_reads(const char *ascii, const uint64_t *offsets, uint64_t n_reads, uint32_t stride,
                        uint8_t *packed, uint16_t *lens, uint32_t *exc_read, uint16_t *exc_pos, uint8_t *exc_chr,
                        uint64_t exc_cap) {
  if (n_reads && !offsets) return set_err(DCRX_E_INVALID, "bad argument to dcrx_pack_reads");
  try {
    return pack_all(ascii, SpanOffsets{offsets}, n_reads, stride, packed, lens, exc_read, exc_pos, exc_chr, exc_cap);
  } catch (...) { return set_err(DCRX_E_NOMEM, "out of memory in dcrx_pack_reads"); }
}

int64_t dcrx_pack_reads_span(const char *ascii, const uint64_t *start, const uint32_t *len, uint64_t n_reads, uint32_t stride,
                             uint8_t *packed, uint16_t *lens, uint32_t *exc_read, uint16_t *exc_pos, uint8_t *exc_chr,
                             uint64_t exc_cap) {
  if (n_reads && (!start || !len)) return set_err(DCRX_E_INVALID, "bad argument to dcrx_pack_reads_span");
  try {
    return pack_all(ascii, SpanStartLen{start, len}, n_reads, stride, packed, lens, exc_read, exc_pos, exc_chr, exc_cap);
  } catch (...) { return set_err(DCRX_E_NOMEM, "out of memory in dcrx_pack_reads_span"); }
}

int dcrx_unpack_reads(const dcrx_batch_t *b, const uint64_t *offsets, char *ascii) {
  if (!b || !offsets || !ascii) return set_err(DCRX_E_INVALID, "null argument");
  for (uint64_t r = 0; r < b->n_reads; r++) {
    const uint32_t len = b->lens ? b->lens[r] : b->read_len;
    const uint8_t *in = b->packed + r * (uint64_t)b->stride;
    char *o = ascii + offsets[r];
    for (uint32_t i = 0; i < len; i++) o[i] = "ACGT"[(in[i >> 2] >> (2 * (i & 3))) & 3];
  }
  for (uint64_t i = 0; i < b->n_exc; i++) ascii[offsets[b->exc_read[i]] + b->exc_pos[i]] = (char)b->exc_chr[i];
  return DCRX_OK;
}

// ---- synthetic reads ------------------------------------------------------------------
static SynthParams synth_params(const dcrx_synth_cfg_t *c) {
  SynthParams P;
  P.seed = c->seed; P.read_len = c->read_len;
  auto clamp01 = [](double x) { return x < 0 ? 0.0 : (x > 1 ? 1.0 : x); };
  P.p_rearr_u16 = (uint32_t)(clamp01(c->p_rearranged) * 65536.0 + 0.5);
  P.sub_u16 = (uint32_t)(clamp01(c->sub_rate) * 65536.0 + 0.5);
  double nr = clamp01(c->n_rate) * 4294967296.0;
  P.n_u32 = nr >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(nr + 0.5);
  return P;
}

static int check_synth(const dcrx_tables_t *t, const dcrx_synth_cfg_t *c, uint32_t stride) {
  if (!t || !c) return set_err(DCRX_E_INVALID, "null argument");
  if (stride == 0 || (stride & 7u) || c->read_len > 4 * stride) return set_err(DCRX_E_INVALID, "bad stride for read_len");
  if (c->read_len > 65535) return set_err(DCRX_E_INVALID, "read_len too large");
  return DCRX_OK;
}

int dcrx_synth_reads_host(const dcrx_tables_t *t, const dcrx_synth_cfg_t *c, uint64_t first, uint64_t n,
                          uint32_t stride, uint8_t *packed) {
  int rc = check_synth(t, c, stride);
  if (rc) return rc;
  if (n && !packed) return set_err(DCRX_E_INVALID, "packed is null");
  const DevTables T = t->host.resolve(t->host.blob.data());
  const SynthParams P = synth_params(c);
  for (uint64_t i = 0; i < n; i++)
    synth_read(T.g[0], T.g[1], P, first + i, reinterpret_cast<uint32_t *>(packed + i * (uint64_t)stride), stride / 4);
  return DCRX_OK;
}

int64_t dcrx_synth_exceptions_host(const dcrx_tables_t *t, const dcrx_synth_cfg_t *c, uint64_t first, uint64_t n,
                                   uint32_t *exc_read, uint16_t *exc_pos, uint8_t *exc_chr, uint64_t cap) {
  if (!t || !c) return set_err(DCRX_E_INVALID, "null argument");
  const SynthParams P = synth_params(c);
  uint64_t cnt = 0;
  if (P.n_u32 == 0 || P.read_len == 0) return 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t key = synth_mix64(P.seed ^ synth_mix64(first + i));
    const uint64_t dn = synth_draw(key, 8);
    if ((uint32_t)(dn & 0xFFFFFFFFu) < P.n_u32) {
      if (cnt < cap && exc_read) {
        exc_read[cnt] = (uint32_t)i; exc_pos[cnt] = (uint16_t)((dn >> 32) % (uint64_t)P.read_len); exc_chr[cnt] = 'N';
      }
      cnt++;
    }
  }
  return (int64_t)cnt;
}

int dcrx_synth_reads_device(dcrx_tables_t *t, const dcrx_synth_cfg_t *c, uint64_t first, uint64_t n, uint32_t stride,
                            uint8_t *d_packed, void *stream) {
  int rc = check_synth(t, c, stride);
  if (rc) return rc;
  if (n && !d_packed) return set_err(DCRX_E_INVALID, "d_packed is null");
  rc = ensure_device(t, 0);
  if (rc) return rc;
  HIP_TRY(launch_synth(t->state.dev, synth_params(c), first, n, stride, d_packed, (hipStream_t)stream));
  return DCRX_OK;
}

}  // extern "C"

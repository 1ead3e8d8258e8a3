// dcrx_launch.h — what dcrx_api.cpp (host) and dcrx_kernels.hip share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dcrx.h"
#include "dcrx_device.h"
#include "dcrx_hip.h"

#include "dcrx_launch_types.h"
#include "dcrx_route.h"
#include "dcrx_tune.h"

namespace dcrx {

// the narrow tuple (include/dcrx.h, dcrx_tuple_layout) as the kernels take it
struct TupleLayoutDev {
  uint32_t w_v, w_j, w_vdel, w_jdel, w_pos, bytes;
  const uint8_t *j_tag_len;    // len(j_seqs[k])
  const int32_t *j_jump;       // jump_to_start_j[k]
};
// The tuple sink of a handle (dcrx_sink_device.h).  V2SinkDev lives in device memory and stays as it is while the sink is on;
// V2SinkCall travels with a launch (dev == nullptr: no sink).
struct V2SinkDev {
  uint32_t *late;              // [regions] items of the late section (zero between calls)
  uint32_t *ticket;            // blocks of the place kernel that have read the counts (zero between calls)
  const uint8_t *j_tag_len;
  const int32_t *j_jump;
};
struct V2SinkCall {
  const V2SinkDev *dev;
  uint2 *items;                // [regions][stride]: the tuple's low word | the read's index inside its region (24 bits; V2_SINK_EMPTY: no tuple) and the tuple's bits 32-39
  uint32_t *hits;              // [regions] decombined reads (zero between calls)
  uint32_t stride;             // items of a region's slab: sections tail (at 0), E, C, late
  uint32_t e_off, c_off, late_off, late_cap;
  uint32_t per_block;          // reads of a region
  uint32_t wpack;              // w_v | w_j << 5 | w_vdel << 10 | w_jdel << 15 | w_pos << 20
};
// what a launch is asked to leave in the sink, and whether it did (else the caller compacts the records)
struct V2SinkJob {
  const V2SinkDev *dev = nullptr;
  uint2 *items = nullptr; uint32_t *hits = nullptr;
  uint64_t items_cap = 0;      // items allocated
  uint32_t regions_cap = 0;    // regions the counters hold
  uint32_t wpack = 0, bytes = 0;
  uint8_t *msg = nullptr; uint64_t n_slots = 0; uint64_t *d_total = nullptr;
  bool *done = nullptr;
};

// The clock of a handle's own timing (dcrx_tune.h) in production: HIP events, read without waiting.  (A query that finds an
// event not complete leaves hipErrorNotReady behind: launch_v2 clears it.)
struct HipTuneClock {
  using Event = dcrx::Event;
  using Counts = PinnedBuf<uint32_t>;
  bool create(Event &e, bool timing) { return e.create(timing) == DCRX_OK; }
  bool done(const Event &e) { return hipEventQuery(e) == hipSuccess; }
  bool elapsed_ms(const Event &a, const Event &b, float &ms) { return hipEventElapsedTime(&ms, a, b) == hipSuccess; }
  void wait(const Event &e) { (void)hipEventSynchronize(e); }
};
using V2TuneSlot = V2TuneSlotT<HipTuneClock>;
using V2Tune = V2TuneT<HipTuneClock>;

// a kernel and the dynamic LDS its launches may ask for (set_lds_ceilings, dcrx_kernels.hip)
struct KernelLds {
  const void *kernel;
  int bytes;
  bool no_static_lds;      // the kernel addresses its table from LDS address 0: static LDS in front of the dynamic segment is refused (hipErrorNotSupported)
};
bool first_use_on_device(bool (&seen)[64]);
hipError_t set_lds_ceilings(bool (&seen)[64], const KernelLds *list, int n);

struct LaunchPlan {
  uint32_t n_cu;
  uint32_t grid;   // fast kernel (upper bound; capped by measured occupancy at launch)
  uint32_t qgrid;  // list kernel
  uint32_t lds_bytes;
  bool table_in_lds;
  bool table16_in_lds;       // the two-bases-per-step table + side tables fit beside the fast kernel's buffers
  uint32_t lds16_bytes;      // counters + that table + side tables
  uint32_t reserved_cus = 0; // compute units the persistent grids leave free (dcrx_set_reserved_cus)
  const DevTables *dev_tables = nullptr;   // DevTables in device memory
  // v2 kernels: the per-wave lists between the scan and the finishing kernel (device memory of the tables handle)
  uint4 *v2_tail = nullptr; uint4 *v2_events = nullptr; uint32_t *v2_counts = nullptr;
  uint4 *v2_slow = nullptr;
  uint4 *v2_left = nullptr;             // the finishing launch's left list (V2_LEFT_CAP event entries of the longest shape)
  uint64_t *v2_acc = nullptr;           // the call's tallies (uint64[DCRX_N_COUNTERS]): zero between calls, handed to the caller by the list kernel
  uint64_t v2_tail_rows = 0, v2_event_rows = 0, v2_slow_rows = 0;       // 16-byte rows allocated for each list
  hipStream_t v2_side = nullptr, v2_side2 = nullptr;  // the tail kernel / the general form over the reads with exception bytes run here, beside the rescue kernel
  hipEvent_t v2_ev_fork = nullptr, v2_ev_join = nullptr, v2_ev_join2 = nullptr;
  // optional, set per call (dcrx_set_step_events): start of the first and end of the last kernel of the call.  Attached to
  // those kernels' own dispatches (hipExtLaunchKernelGGL): a separate event record costs the stream ~10 us of gap each
  hipEvent_t ev_step_start = nullptr, ev_step_stop = nullptr;
  V2SinkJob sink;              // set per call while a tuple sink is on (dcrx_set_tuple_sink)
  V2Tune *tune = nullptr;      // [2]: per frame (the handle owns them, and with them the events and pinned counts launch_v2 makes in their slots)
  bool tune_may_wait = false;  // dcrx_set_tune_wait: the fourth call of a big-batch size class may wait for the third's finishing launch, once
};

// compute units the persistent grids may fill (reserved_cus: left to other streams — an RCCL gather running beside the scan)
inline uint32_t free_cus(const LaunchPlan &P) { return P.n_cu > P.reserved_cus ? P.n_cu - P.reserved_cus : 1u; }

// The facts a call's route follows from (dcrx_route.h), and the launches of that route: what route_of() said of these facts
// is what launch_decombine runs — dcrx_api.cpp asks first and sizes the workspace by the answer.
RouteFacts route_facts(const LaunchPlan &P, const DevTables &T, uint32_t stride, bool uniform, uint64_t n_reads, int orientation, uint32_t flags);
hipError_t launch_decombine(const Route &R, const LaunchPlan &P, const DevTables &T, const BatchDev &B, const CfgDev &cfg,
                            dcrx_record_t *rec, uint32_t *queue, uint32_t *gqueue, uint32_t *queue_count,
                            uint64_t *d_counters, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// dcrx_kernels_v2.hip
void v2_list_rows(uint64_t max_reads, uint32_t stride, uint32_t n_cu, uint64_t *tail_rows, uint64_t *event_rows);
uint64_t v2_slow_rows(uint64_t max_reads, uint32_t stride, uint32_t n_cu);
void v2_route_facts(const DevTables &T, uint32_t stride, RouteFacts &F);      // the v2 kernels' share of route_facts
// what a v2 launch that serves the call's tuple sink leaves for the list kernel and the place kernel behind it
struct V2SinkLaunch { V2SinkCall S{}; uint32_t n_regions = 0, tcap = 0, ecap = 0, ccap = 0, fused = 0; const uint32_t *counts = nullptr; };
hipError_t launch_v2_any(const LaunchPlan &P, const DevTables &T, const BatchDev &B, const CfgDev &cfg, dcrx_record_t *rec,
                         uint32_t *queue, uint32_t *gqueue, uint32_t qcap, uint32_t *queue_count, unsigned long long *d_counters,
                         hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, const Route::Pass &pass, uint32_t retry = 0, V2SinkLaunch *sink = nullptr);
hipError_t launch_v2_place(const LaunchPlan &P, const V2SinkLaunch &K, uint64_t n_reads, hipStream_t s, hipEvent_t ev_stop);
uint64_t v2_sink_items(uint64_t max_reads, uint32_t n_cu);      // items a handle's sink needs for batches of up to max_reads reads
hipError_t launch_compact(const dcrx_record_t *rec, uint64_t n, uint64_t first_index, dcrx_record_t *hits,
                          uint64_t *hit_index, uint64_t *ok_bitmap, int packed12, uint64_t *d_total, uint32_t *tile_count,
                          uint64_t *tile_off, hipStream_t s);
hipError_t launch_compact_narrow(const dcrx_record_t *rec, uint64_t n, uint8_t *msg, uint64_t n_slots, const TupleLayoutDev &L, uint64_t *d_total,
                                 uint32_t *tile_count, uint64_t *tile_off, hipStream_t s);
uint32_t compact_tiles(uint64_t n);

}  // namespace dcrx

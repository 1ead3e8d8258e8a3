// dcrx_route.h — which launches a decombine call consists of, decided once per call from plain facts.  Plain C++, no HIP: the
// launchers fill RouteFacts from the handle's plan, the tables, the batch, the cfg and the debug knobs (route_facts,
// dcrx_kernels.hip), dcrx_api.cpp asks route_of() before it sizes the workspace and launches, and tests/host_route prints the
// route of facts given on a command line.
#pragma once

#include <cstdint>

#include "../../include/dcrx_codes.h"
#include "dcrx_launch_types.h"

namespace dcrx {

constexpr uint32_t DCRX_LDS_CU = 160u * 1024u;             // LDS of a compute unit: what one block may take
constexpr uint32_t DCRX_V2_FINISH_LDS_MAX = 64u * 1024u;   // ... and a block of the v2 finishing launch

// index of a frame's tables, tuners and kernels: 0 forward, 1 reverse (`both` on the three-launch form counts as 1)
inline int route_frame(const int orientation) { return orientation == DCRX_ORIENT_FORWARD ? 0 : 1; }

struct RouteFacts {
  uint32_t stride = 0;
  bool uniform = true;               // one length for all reads (no per-read lengths)
  uint64_t n_reads = 0;
  int orientation = DCRX_ORIENT_REVERSE;
  uint32_t flags = 0;
  bool table_in_lds = false, table16_in_lds = false;      // the one-base table / the pair table of the three-launch form fit LDS
  uint32_t lds16_bytes = 0, rescue_lds_extra = 0;         // counters + pair table + side tables; what a rescue block adds to them
  bool pair_rescue = false;          // the tables serve the rescue kernel
  bool v2_ok = false;                // the tables express the v2 kernels' form
  struct Frame {
    uint32_t trans_bytes = 0;        // the v2 pair table
    uint32_t scan_lds = 0;           // a scan block's LDS with that table (no ring)
    uint32_t finish_lds = 0;         // a finishing block's LDS at this stride's register shape
    uint32_t bucket_bytes = 0;       // the keyword buckets (in the scan block's LDS beside a ring)
    bool narrow = false;             // 16-bit entries suffice (one of the A/B shapes exists for these only)
  } frame[2];
  uint32_t side_bytes = 0;           // the side tables (beside a ring as well)
  uint32_t ring_batch_bytes = 0;     // LDS of one batch of the tail ring
  uint32_t fuse_limit = 0, ring_max = 0, ring_min = 0;      // knobs: largest pair table that fuses; the rings tried, halving
};

enum class RouteForm { LONG, THREE_LAUNCH, V2, V2_BOTH };

struct Route {
  RouteForm form = RouteForm::LONG;
  // the three-launch form: prologue -> fast kernel -> rescue kernel or list kernel
  bool pair_scan = false;            // two bases per step (else one)
  int nw = DCRX_NWMAX;               // words of a read in registers: 10 or DCRX_NWMAX
  bool all_general = false;          // no fast kernel: every read through the list kernel
  bool rescue_kernel = false;        // the rescue kernel takes the rescue queue and is the last launch (else the list kernel)
  // the v2 kernels: per pass scan -> finishing launch -> list kernel
  struct Pass {
    int frame = 1;
    int reads_per_lane = 2;
    bool prefetch = true;
    uint32_t ring_batches = 0;       // the tail inside the scan through a ring of so many batches; 0: a role or a launch of its own
  } pass[2];
  int n_passes = 0;
  bool needs_tail_list = false;      // a pass keeps the tail out of the scan: the handle must hold the tail list
  uint32_t last_form = 0;            // what dcrx_tune_state reports for the call's frame until a v2 pass refines it: 1, 2 (0: the long form reports nothing)
  bool v2() const { return form == RouteForm::V2 || form == RouteForm::V2_BOTH; }
};

// The launch shape of a v2 pass: DCRX_F_V2_SHAPE(k), 0 = two reads per lane where the registers allow (150-nt shapes), else one;
// 1 = four per lane without prefetch (uniform 150-nt batches on narrow tables; elsewhere two); the longest reads always one.
inline void route_v2_shape(const RouteFacts &F, Route::Pass &p) {
  const bool nw10 = F.stride <= 40;
  uint32_t shape = (F.flags >> 8) & 3u;
  if (shape == 0) shape = nw10 ? 2 : 3;
  p.reads_per_lane = 2; p.prefetch = true;
  if (F.stride > 4 * DCRX_NWMAX) { p.reads_per_lane = 1; p.prefetch = false; }
  else if (shape == 3) p.reads_per_lane = 1;
  else if (shape == 1 && nw10 && F.uniform && F.frame[p.frame].narrow) { p.reads_per_lane = 4; p.prefetch = false; }
}

// Batches of the tail ring of a pass (the fused form: the tail inside the scan kernel, through a ring in LDS): the 150-nt
// two-reads-per-lane shape, a pair table of up to fuse_limit, no A/B form or profiling switch that keeps the tail a launch of
// its own, and the largest ring from ring_max down to ring_min that fits beside the table, the side tables and the buckets.
inline uint32_t route_tail_ring(const RouteFacts &F, const Route::Pass &p) {
  const RouteFacts::Frame &f = F.frame[p.frame];
  if (F.stride > 40 || p.reads_per_lane != 2 || !p.prefetch || f.trans_bytes > F.fuse_limit) return 0u;
  if (F.flags & (DCRX_F_V2_NO_FUSE | DCRX_F_V2_SIDE_STREAMS | DCRX_F_V2_LEAN_SERIAL | DCRX_F_V2_NO_LEAN_RESCUE | (DCRX_F_PROFILE_MASK & ~DCRX_F_PROFILE_TAIL_STREAM_ONLY)))
    return 0u;
  const uint32_t fixed = f.scan_lds + F.side_bytes + f.bucket_bytes;
  for (uint32_t nb = F.ring_max; nb && nb >= F.ring_min; nb >>= 1)
    if (fixed + nb * F.ring_batch_bytes <= DCRX_LDS_CU) return nb;
  return 0u;
}

inline Route route_of(const RouteFacts &F) {
  Route R;
  if (F.stride > DCRX_FAST_MAX_STRIDE) return R;      // reads of 512 nt and more: the long form
  const bool both = F.orientation == DCRX_ORIENT_BOTH;
  // The v2 kernels serve one frame per pass — `both` is the reverse frame and then the forward frame for the reads it did not
  // decombine —; the A/B switches of the three-launch form and the forced slow reader keep that form, and so do tables that
  // leave a scan or a finishing block no room (a `both` call needs both frames' to fit, and takes no profiling switch).  An
  // entry keeps two flags above a 30-bit read index.
  auto fits = [&](const int o) { return F.frame[o].scan_lds <= DCRX_LDS_CU && F.frame[o].finish_lds <= DCRX_V2_FINISH_LDS_MAX; };
  const bool v2 = F.v2_ok && F.n_reads < (1ull << 30) &&
                  !(F.flags & (DCRX_F_V1_KERNELS | DCRX_F_FORCE_SLOW_READER | DCRX_F_ONE_BASE_SCAN | DCRX_F_LIST_RESCUE | DCRX_F_PROFILE_LIST_SCAN_ONLY)) &&
                  (both ? fits(0) && fits(1) && !(F.flags & DCRX_F_PROFILE_MASK) : fits(route_frame(F.orientation)));
  if (v2) {
    R.form = both ? RouteForm::V2_BOTH : RouteForm::V2;
    R.n_passes = both ? 2 : 1;
    R.pass[0].frame = both ? 1 : route_frame(F.orientation);
    R.pass[1].frame = 0;
    for (int k = 0; k < R.n_passes; k++) {
      route_v2_shape(F, R.pass[k]);
      R.pass[k].ring_batches = route_tail_ring(F, R.pass[k]);
      if (!R.pass[k].ring_batches) R.needs_tail_list = true;
    }
    R.last_form = 2;
    return R;
  }
  R.form = RouteForm::THREE_LAUNCH;
  R.last_form = 1;
  R.nw = F.stride <= 40 ? 10 : DCRX_NWMAX;      // 150-nt reads: ten words in registers
  R.pair_scan = F.table_in_lds && F.table16_in_lds && !(F.flags & DCRX_F_ONE_BASE_SCAN);
  // (the fast kernel holds 320 nt in registers: longer reads all go through the list kernel, as `both` and the forced slow reader do)
  R.all_general = both || (F.flags & DCRX_F_FORCE_SLOW_READER) || F.stride > 4 * DCRX_NWMAX;
  R.rescue_kernel = R.pair_scan && F.pair_rescue && !(F.flags & DCRX_F_LIST_RESCUE) && F.lds16_bytes + F.rescue_lds_extra <= DCRX_LDS_CU && !R.all_general;
  return R;
}

}  // namespace dcrx

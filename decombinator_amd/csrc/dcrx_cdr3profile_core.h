// dcrx_cdr3profile_core.h — the bin of a distance in a radius profile (include/dcrx.h "profile, weighted"), shared by the kernel
// (dcrx_cdr3walk.h: the Profile sink of cdr3_walk_kernel) and a plain host build (tests/host_cdr3profile).
//
// A profile has `bins` bins of `step` each: bin 0 holds distance 0 alone, bin b the distances (b - 1) * step < d <= b * step,
// which is ceil(d / step).  The ladder's top is R = step * (bins - 1) <= 65535, and the walk hands over distances d <= R only.
#pragma once
#include <stdint.h>

#include "dcrx_cdr3w_core.h"

namespace dcrx_cdr3profile {

using namespace dcrx_cdr3w;

constexpr uint32_t MAX_BINS = 32, MAX_STEP = 65535;

// ceil(d / step) for d in 0 .. 65535 and step in 1 .. 65535, by a true division: exact by definition.  Both operands are cut
// to the 16 bits the contract leaves them, so the dividend stays below 2^17 and the compiler may take its short (24-bit)
// division on the device.
DCRX_CDR3NET_HD uint32_t bin_of(uint32_t d, uint32_t step) {
  const uint32_t s = step & 0xFFFFu;
  return ((d & 0xFFFFu) + s - 1u) / s;
}

// what the entries refuse of (step, bins), as a message; null: the ladder stands
DCRX_CDR3NET_HD const char *refuse_ladder(uint32_t step, uint32_t bins) {
  if (step < 1 || step > MAX_STEP) return "the step is 1 .. 65535";
  if (bins < 1 || bins > MAX_BINS) return "the bins are 1 .. 32";
  if ((uint64_t)step * (bins - 1) > MAX_RADIUS) return "step * (bins - 1) is above 65535";
  return nullptr;
}

}  // namespace dcrx_cdr3profile

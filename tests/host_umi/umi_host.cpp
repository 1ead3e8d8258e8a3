// Test-only: the kernel's per-pair function (dcrx_umi_core.h) built by g++, for a check against a plain DP on the host.
#include "../../decombinator_amd/csrc/dcrx_umi_core.h"

extern "C" int umi_host_pair_distance(const uint32_t *a, const uint32_t *b, int32_t k) { return dcrx_umi::pair_distance(a, b, k); }

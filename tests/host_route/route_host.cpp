// Test-only host build of the call route (decombinator_amd/csrc/dcrx_route.h): prints the route of the facts given on the
// command line, one key=value line on stdout.
//
//   route_host key=value ...
//
// Facts not given are those of a tag set like config 2's on 150-nt reads: everything fits, both frames fuse.  Per-frame
// keys end in 0 (forward) or 1 (reverse): trans0, scan0, finish0, bucket0, narrow0, ...  `flags` takes names joined by `+`
// (V1_KERNELS, V2_NO_FUSE, SHAPE1 .. SHAPE3, PROFILE_SCAN_ONLY, ...) or a number; `orientation` reverse, forward or both.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../decombinator_amd/csrc/dcrx_route.h"

namespace {

const std::map<std::string, uint32_t> FLAGS = {
    {"FORCE_SLOW_READER", DCRX_F_FORCE_SLOW_READER}, {"PROFILE_SCAN_ONLY", DCRX_F_PROFILE_SCAN_ONLY}, {"ONE_BASE_SCAN", DCRX_F_ONE_BASE_SCAN},
    {"PROFILE_LIST_SCAN_ONLY", DCRX_F_PROFILE_LIST_SCAN_ONLY}, {"LIST_RESCUE", DCRX_F_LIST_RESCUE}, {"PROFILE_RESCUE_HITS_ONLY", DCRX_F_PROFILE_RESCUE_HITS_ONLY},
    {"V1_KERNELS", DCRX_F_V1_KERNELS}, {"PROFILE_NO_FINISH", DCRX_F_PROFILE_NO_FINISH}, {"PROFILE_NO_EVENTS", DCRX_F_PROFILE_NO_EVENTS},
    {"PROFILE_NO_TAIL", DCRX_F_PROFILE_NO_TAIL}, {"V2_NO_LEAN_RESCUE", DCRX_F_V2_NO_LEAN_RESCUE}, {"PROFILE_TAIL_STREAM_ONLY", DCRX_F_PROFILE_TAIL_STREAM_ONLY},
    {"V2_LEAN_SERIAL", DCRX_F_V2_LEAN_SERIAL}, {"V2_SIDE_STREAMS", DCRX_F_V2_SIDE_STREAMS}, {"V2_NO_FUSE", DCRX_F_V2_NO_FUSE},
    {"SHAPE1", DCRX_F_V2_SHAPE(1)}, {"SHAPE2", DCRX_F_V2_SHAPE(2)}, {"SHAPE3", DCRX_F_V2_SHAPE(3)}};

bool parse_flags(const std::string &v, uint32_t &out) {
  out = 0;
  if (v.empty() || (v[0] >= '0' && v[0] <= '9')) { out = (uint32_t)strtoul(v.c_str(), nullptr, 0); return true; }
  size_t at = 0;
  while (at <= v.size()) {
    const size_t plus = v.find('+', at);
    const std::string name = v.substr(at, plus == std::string::npos ? std::string::npos : plus - at);
    const auto it = FLAGS.find(name);
    if (it == FLAGS.end()) { fprintf(stderr, "route_host: unknown flag %s\n", name.c_str()); return false; }
    out |= it->second;
    if (plus == std::string::npos) break;
    at = plus + 1;
  }
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  dcrx::RouteFacts F;
  F.stride = 40; F.uniform = true; F.n_reads = 5000;
  F.table_in_lds = F.table16_in_lds = true;
  F.lds16_bytes = 100u * 1024u; F.rescue_lds_extra = 36928u;
  F.pair_rescue = F.v2_ok = true;
  for (int o = 0; o < 2; o++) {
    F.frame[o].trans_bytes = 56u * 1024u; F.frame[o].scan_lds = 56u * 1024u + 512u; F.frame[o].finish_lds = 40u * 1024u;
    F.frame[o].bucket_bytes = 2048u; F.frame[o].narrow = true;
  }
  F.side_bytes = 8192u; F.ring_batch_bytes = 3840u;
  F.fuse_limit = 64u * 1024u; F.ring_max = 16; F.ring_min = 8;
  for (int i = 1; i < argc; i++) {
    const char *eq = strchr(argv[i], '=');
    if (!eq) { fprintf(stderr, "route_host: %s is not key=value\n", argv[i]); return 2; }
    std::string k(argv[i], eq - argv[i]);
    const std::string v(eq + 1);
    const unsigned long long n = strtoull(v.c_str(), nullptr, 0);
    if (k == "flags") { if (!parse_flags(v, F.flags)) return 2; continue; }
    if (k == "orientation") {
      if (v == "reverse") F.orientation = DCRX_ORIENT_REVERSE;
      else if (v == "forward") F.orientation = DCRX_ORIENT_FORWARD;
      else if (v == "both") F.orientation = DCRX_ORIENT_BOTH;
      else { fprintf(stderr, "route_host: orientation %s\n", v.c_str()); return 2; }
      continue;
    }
    if (k == "stride") F.stride = (uint32_t)n;
    else if (k == "uniform") F.uniform = n != 0;
    else if (k == "n_reads") F.n_reads = n;
    else if (k == "table_in_lds") F.table_in_lds = n != 0;
    else if (k == "table16_in_lds") F.table16_in_lds = n != 0;
    else if (k == "lds16_bytes") F.lds16_bytes = (uint32_t)n;
    else if (k == "rescue_lds_extra") F.rescue_lds_extra = (uint32_t)n;
    else if (k == "pair_rescue") F.pair_rescue = n != 0;
    else if (k == "v2_ok") F.v2_ok = n != 0;
    else if (k == "side") F.side_bytes = (uint32_t)n;
    else if (k == "ring_batch") F.ring_batch_bytes = (uint32_t)n;
    else if (k == "fuse_limit") F.fuse_limit = (uint32_t)n;
    else if (k == "ring_max") F.ring_max = (uint32_t)n;
    else if (k == "ring_min") F.ring_min = (uint32_t)n;
    else {
      const char last = k.empty() ? 0 : k.back();
      if (last != '0' && last != '1') { fprintf(stderr, "route_host: unknown key %s\n", k.c_str()); return 2; }
      dcrx::RouteFacts::Frame &f = F.frame[last - '0'];
      k.pop_back();
      if (k == "trans") f.trans_bytes = (uint32_t)n;
      else if (k == "scan") f.scan_lds = (uint32_t)n;
      else if (k == "finish") f.finish_lds = (uint32_t)n;
      else if (k == "bucket") f.bucket_bytes = (uint32_t)n;
      else if (k == "narrow") f.narrow = n != 0;
      else { fprintf(stderr, "route_host: unknown key %s%c\n", k.c_str(), last); return 2; }
    }
  }
  const dcrx::Route R = dcrx::route_of(F);
  static const char *const FORM[] = {"long", "three", "v2", "v2_both"};
  printf("form=%s last_form=%u needs_tail_list=%d", FORM[(int)R.form], R.last_form, R.needs_tail_list ? 1 : 0);
  if (R.form == dcrx::RouteForm::THREE_LAUNCH)
    printf(" scan=%s nw=%d all_general=%d rescue_kernel=%d last=%s", R.pair_scan ? "pair" : "one_base", R.nw, R.all_general ? 1 : 0, R.rescue_kernel ? 1 : 0,
           R.rescue_kernel ? "rescue" : "list");
  printf(" passes=%d", R.n_passes);
  for (int k = 0; k < R.n_passes; k++)
    printf(" frame%d=%d rpl%d=%d prefetch%d=%d ring%d=%u", k, R.pass[k].frame, k, R.pass[k].reads_per_lane, k, R.pass[k].prefetch ? 1 : 0, k, R.pass[k].ring_batches);
  printf("\n");
  return 0;
}

// Test-only host build of a handle's launch tuners (decombinator_amd/csrc/dcrx_tune.h) and of the debug knobs' reader
// (dcrx_debug_flags.h), with a scripted clock in place of HIP events.  One line per simulated launch on stdout.
//
//   tune_host rescue key=value ... script=eeEi...   one character per launch: e an eligible launch of `reads` reads, E one of
//                                                    `reads2` reads (another size class), i an ineligible one (the launcher
//                                                    leaves the slot alone)
//   tune_host liste key=value ... script=ffbf...    f a launch the tuner may time, b one that carries the caller's events or a sink
//   tune_host knob NAME lo hi fallback              what dcrx_debug_int reads from the environment
//
// The clock: an event recorded by launch n has completed from launch n + lag on (lag_at=k:v: launch k's events take v launches);
// create number fail_create (counted from 0) fails; a timed launch takes t1 / t2 ms on the first / second setting.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../decombinator_amd/csrc/dcrx_debug_flags.h"
#include "../../decombinator_amd/csrc/dcrx_tune.h"

namespace {

struct FakeEvent {
  bool made = false;
  mutable bool recorded = false;
  mutable int recorded_at = 0, ready_at = 0;
  mutable float at_ms = 0.f;      // the device's time when it passed
  explicit operator bool() const { return made; }
};
struct FakeClock {
  using Event = FakeEvent;
  using Counts = int;
  int now = 0, creates = 0, fail_create = -1, queries = 0, waits = 0;
  int synced = -1;      // what launches up to this one recorded has completed (a wait: the stream runs in order)
  bool create(Event &e, bool) { if (creates++ == fail_create) return false; e.made = true; return true; }
  bool done(const Event &e) { queries++; return e.recorded && (now >= e.ready_at || e.recorded_at <= synced); }
  bool elapsed_ms(const Event &a, const Event &b, float &ms) { ms = b.at_ms - a.at_ms; return true; }
  void wait(const Event &e) { waits++; if (e.recorded && e.recorded_at > synced) synced = e.recorded_at; }
  void record(const Event &start, const Event &stop, float ms, int lag) const {
    start.recorded = stop.recorded = true; start.recorded_at = stop.recorded_at = now; start.ready_at = stop.ready_at = now + lag; start.at_ms = 100.f; stop.at_ms = 100.f + ms;
  }
};
using Slot = dcrx::V2TuneSlotT<FakeClock>;
using Tune = dcrx::V2TuneT<FakeClock>;

struct Args {
  std::map<std::string, std::string> kv;
  Args(int argc, char **argv) {
    for (int i = 2; i < argc; i++) {
      const char *eq = strchr(argv[i], '=');
      if (eq) kv[std::string(argv[i], eq - argv[i])] = eq + 1;
    }
  }
  double num(const char *k, double d) const { auto it = kv.find(k); return it == kv.end() ? d : atof(it->second.c_str()); }
  std::string str(const char *k) const { auto it = kv.find(k); return it == kv.end() ? "" : it->second; }
  int lag(int launch) const {      // lag_at=k:v overrides lag for launch k
    const std::string s = str("lag_at");
    int k = -1, v = 0;
    if (!s.empty() && sscanf(s.c_str(), "%d:%d", &k, &v) == 2 && k == launch) return v;
    return (int)num("lag", 1);
  }
};

int run_rescue(const Args &a) {
  FakeClock x;
  x.fail_create = (int)a.num("fail_create", -1);
  Tune F;
  const uint64_t reads[2] = {(uint64_t)a.num("reads", 3000000), (uint64_t)a.num("reads2", 1500000)};
  const bool may_wait = a.num("may_wait", 0) != 0;
  const float t[2] = {(float)a.num("t1", 1.0), (float)a.num("t2", 1.0)};
  const std::string script = a.str("script");
  for (size_t n = 0; n < script.size(); n++) {
    x.now = (int)n;
    const char c = script[n];
    if (c == 'i') { printf("launch=%zu class=-\n", n); continue; }
    const uint64_t nr = reads[c == 'E' ? 1 : 0];
    uint32_t first, second;
    Tune::candidates(nr, first, second);
    const int q0 = x.queries, w0 = x.waits;
    const dcrx::V2RescueStep<FakeClock> st = dcrx::tune_rescue_waves(F, x, nr, may_wait);
    if (st.start) x.record(*st.start, *st.stop, st.waves == first ? t[0] : t[1], a.lag((int)n));
    const Slot &U = F.slot[Tune::size_class(nr)];
    printf("launch=%zu class=%d waves=%u timed=%d queried=%d waited=%d choice=%u launches=%d us0=%.1f us1=%.1f\n", n, Tune::size_class(nr), st.waves, st.start ? 1 : 0,
           x.queries - q0, x.waits - w0, U.choice, U.launches, U.us[0], U.us[1]);
  }
  return 0;
}

int run_liste(const Args &a) {
  FakeClock x;
  x.fail_create = (int)a.num("fail_create", -1);
  Tune F;
  const uint64_t reads = (uint64_t)a.num("reads", 3000000), entries = (uint64_t)a.num("entries", 300000);
  const float max_share = (float)a.num("max_share", 0.25);
  const float t[2] = {(float)a.num("t1", 1.0), (float)a.num("t2", 1.0)};      // a role, fused
  const int settle_at = (int)a.num("settle_at", 0);      // the launch from which the rescue waves are settled
  const bool room = a.num("room", 1) != 0, copy_ok = a.num("copy_ok", 1) != 0;
  Slot &U = F.slot[Tune::size_class(reads)];
  const std::string script = a.str("script");
  for (size_t n = 0; n < script.size(); n++) {
    x.now = (int)n;
    if ((int)n >= settle_at && !U.choice) U.choice = 4096u;
    const int q0 = x.queries;
    // the launcher's order: the share (once the counts are in), the form of this launch, the scan, the counts behind the first scan
    dcrx::tune_e_share(U, x, max_share, [&] { return entries; });
    const dcrx::V2ListEStep<FakeClock> st = dcrx::tune_list_e(U, x, script[n] == 'f');
    bool fused = st.fused;
    if (fused && !room) { dcrx::tune_e_no_room(U); fused = false; }
    if (st.start) x.record(*st.start, *st.stop, fused ? t[1] : t[0], a.lag((int)n));
    int copies = 0;
    dcrx::tune_e_first_launch(U, 256u, reads, [&] {
      copies++;
      if (!copy_ok || !x.create(U.ev_counts, false)) return false;
      x.record(U.ev_counts, U.ev_counts, 0.f, a.lag((int)n));
      return true;
    });
    int pair = -1;
    for (int k = 0; k < 2 * Slot::E_PAIRS; k++) if (st.start == &U.ev_e[k][0]) pair = k;
    printf("launch=%zu fused=%d pair=%d copies=%d queried=%d state=%d phase=%d share=%.3f us0=%.1f us1=%.1f\n", n, fused ? 1 : 0, pair, copies, x.queries - q0, U.fuse_e, U.e_phase,
           U.e_share, U.us_e[0], U.us_e[1]);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 6 && !strcmp(argv[1], "knob")) {
    printf("%d\n", dcrx_debug_int(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "rescue")) return run_rescue(Args(argc, argv));
  if (argc >= 2 && !strcmp(argv[1], "liste")) return run_liste(Args(argc, argv));
  fprintf(stderr, "usage: tune_host rescue|liste key=value ... | knob NAME lo hi fallback\n");
  return 2;
}

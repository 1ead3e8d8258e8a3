// dcrx_tune.h — what a handle settles for its own v2 launches (launch_v2), as operations on a size class's slot.  Plain C++, no
// HIP: everything that touches an event goes through a clock X, which production fills with the HIP calls (dcrx_launch.h,
// HipTuneClock) and tests/host_tune with a scripted one.  X provides
//   typename X::Event                       an owner that is false in a condition until created
//   typename X::Counts                      where the first launch's list counts go (the launcher's business)
//   bool create(Event &, bool timing)       false: the event could not be created
//   bool done(const Event &)                has it completed?  (never waits)
//   bool elapsed_ms(const Event &start, const Event &stop, float &ms)
//   void wait(const Event &)
#pragma once

#include <cstdint>

namespace dcrx {

// A handle's own choice of the waves that share a region's list E in the finishing launch of the fused form (launch_v2): 16 per
// region suit some tag sets and 12 others by 1-4 % of the step, whatever the reads are, so a handle
// times its own launches: behind its first launch of a batch size one finishing launch on each setting carries a pair of
// events on its dispatch (no marker packets), later launches look (X::done: no waiting) whether the pairs have completed, and
// the second setting stays if its launches were at least 1.5 % shorter; else the first.  One per frame.
template <class X> struct V2TuneSlotT {
  using Event = typename X::Event;
  static constexpr int SAMPLES = 2;      // (one per setting — the two differ by a tenth of the launch, samples by a hundredth —: launches 1 and 2 of a size class, so that a caller's third or fourth launch finds them complete and runs on the choice)
  uint32_t choice = 0;               // rescue waves once settled (0: not yet)
  int launches = 0;                  // eligible launches seen in this size class until it settled
  Event ev[SAMPLES][2];              // (start, stop) of the finishing launch of sample k
  bool created = false;              // all of them exist
  // list E inside the scan kernel (FUSE_E) or a role of the finishing launch: decided once per size class from the share of the
  // reads that were list-E entries in the class's first launch (the regions' counts copied to pinned memory behind that launch,
  // read when the copy's event has passed: no wait)
  int fuse_e = -1;                   // -1 not known yet, -2 the share allows it: the two forms are being timed, 0 a role, 1 inside the scan
  static constexpr int E_PAIRS = 3, E_FIRST = 8;      // timed launches per form, from the class's E_FIRST-th eligible launch on (the clocks have come up by then)
  int e_phase = 0;                   // (fuse_e == -2) eligible launches seen: E_FIRST + k, k < E_PAIRS, runs as a role under pair k, E_FIRST + E_PAIRS fused and untimed, the next E_PAIRS fused under pairs E_PAIRS ..; then the events are read
  Event ev_e[2 * E_PAIRS][2];        // (start on the scan's dispatch, stop on the finishing launch's) per timed launch
  float us_e[2] = {0.f, 0.f};        // what the samples said: mean of the launches with list E a role / inside the scan
  bool e_sampling = false;
  Event ev_counts;
  typename X::Counts h_counts;       // V2_L_COUNTS words per region
  uint32_t e_regions = 0;
  uint64_t e_reads = 0;
  float e_share = -1.f;
  float us[2] = {0.f, 0.f};          // what the samples said: a finishing launch on the first / on the second candidate (dcrx_tune_state)
};
// ... per size class (batches of 2^(20 + k) .. 2^(21 + k) - 1 reads share a slot): a short last chunk of a host call, or the
// short last step of a shard, falls into another class and leaves the settled one alone.
template <class X> struct V2TuneT {
  static constexpr int SAMPLES = V2TuneSlotT<X>::SAMPLES;
  static constexpr int CLASSES = 12;
  static constexpr uint64_t BIG_BATCH = 1ull << 25;      // reads: from here a handle chooses between 8 192 and 4 096 rescue waves (below: 4 096 and 3 072)
  V2TuneSlotT<X> slot[CLASSES];
  uint32_t last_form = 0;            // the frame's last call: 0 none yet, 1 the three-launch form, 2 the v2 kernels (tail as a role), 3 v2 with the tail inside the scan, 4 with list E inside the scan as well
  static void candidates(uint64_t n_reads, uint32_t &first, uint32_t &second) {      // the rescue waves a handle chooses between
    const bool big = n_reads >= BIG_BATCH;
    first = big ? 8192u : 4096u; second = big ? 4096u : 3072u;
  }
  static int size_class(uint64_t n_reads) {      // -1: below a million reads (not tuned)
    if (n_reads < (1ull << 20)) return -1;
    int k = 0;
    while (k + 1 < CLASSES && (n_reads >> (21 + k)) != 0) k++;
    return k;
  }
};

// ---- the procedure both choices share: timed launches under a pair of events each, read without waiting; the second setting
// wins only if its launches were at least 1.5 % shorter in sum
struct V2Timing {
  bool ready = false;                // every stop event has completed
  bool ok = false;                   // ... and every pair gave a time
  float ms[2] = {0.f, 0.f};          // summed per setting
  bool second_wins() const { return ok && ms[1] < 0.985f * ms[0]; }
};
template <class X, class E> bool tune_create_pairs(X &x, E (*ev)[2], const int n) {      // all of them, or false at the first that fails
  for (int i = 0; i < n; i++)
    for (int b = 0; b < 2; b++)
      if (!x.create(ev[i][b], true)) return false;
  return true;
}
// setting_of(i): the setting (0, 1) pair i was timed on
template <class X, class E, class F> V2Timing tune_read_pairs(X &x, E (*ev)[2], const int n, F setting_of) {
  V2Timing t;
  for (int i = 0; i < n; i++)
    if (!x.done(ev[i][1])) return t;
  t.ready = t.ok = true;
  for (int i = 0; i < n && t.ok; i++) {
    float one = 0.f;
    t.ok = x.elapsed_ms(ev[i][0], ev[i][1], one);
    t.ms[setting_of(i)] += one;
  }
  return t;
}

// ---- rescue waves ----
// What an eligible launch (launch_v2 says which are) runs on, and the pair of the slot's events its finishing launch carries
// when it is a sample.  The class's first launch is not timed, launch 1 + k is sample k on candidate k & 1; later launches ask
// whether the samples have completed and settle when they have, running on the first candidate meanwhile.  Nothing waits, but
// for the launch right behind the last sample of a big batch where the caller allowed it (may_wait: dcrx_set_tune_wait).
// n_reads: a batch of a size class (V2TuneT::size_class >= 0).
template <class X> struct V2RescueStep {
  uint32_t waves;
  const typename X::Event *start = nullptr, *stop = nullptr;
  bool read = false;                 // this launch read the samples (the slot's us[] say what they took)
};
template <class X> V2RescueStep<X> tune_rescue_waves(V2TuneT<X> &F, X &x, const uint64_t n_reads, const bool may_wait) {
  constexpr int N = V2TuneSlotT<X>::SAMPLES;
  V2TuneSlotT<X> &U = F.slot[V2TuneT<X>::size_class(n_reads)];
  uint32_t first, second;
  V2TuneT<X>::candidates(n_reads, first, second);
  V2RescueStep<X> r{first};
  if (U.choice) { r.waves = U.choice; return r; }
  const int k = U.launches - 1;      // sample index of this launch
  if (k >= 0 && k < N) {
    if (!U.created) {
      U.created = tune_create_pairs(x, U.ev, N);
      if (!U.created) U.choice = first;
    }
    if (U.created) { r.waves = (k & 1) ? second : first; r.start = &U.ev[k][0]; r.stop = &U.ev[k][1]; }
  } else if (k >= N && U.created) {
    if (may_wait && n_reads >= V2TuneT<X>::BIG_BATCH && k == N) x.wait(U.ev[N - 1][1]);
    const V2Timing t = tune_read_pairs(x, U.ev, N, [](int i) { return i & 1; });
    if (t.ready) {
      U.choice = t.second_wins() ? second : first;
      if (t.ok) { U.us[0] = 1e3f * t.ms[0] / (N / 2); U.us[1] = 1e3f * t.ms[1] / (N / 2); }
      r.waves = U.choice; r.read = true;
    }
  }
  U.launches++;
  return r;
}

// ---- list E inside the scan ----
// The class's first launch: `copy` sends the regions' list counts to the slot's pinned memory behind the scan and records
// ev_counts (false: it could not — a role it stays).
template <class X, class Copy> void tune_e_first_launch(V2TuneSlotT<X> &U, const uint32_t regions, const uint64_t reads, Copy copy) {
  if (U.fuse_e != -1 || U.e_sampling) return;
  if (copy()) { U.e_sampling = true; U.e_regions = regions; U.e_reads = reads; }
  else U.fuse_e = 0;
}
// A later launch, once that copy has completed: list E's share of the reads decides between "a role" and "to be timed"
// (`entries` sums list E's counts).  True: decided by this call.
template <class X, class Sum> bool tune_e_share(V2TuneSlotT<X> &U, X &x, const float max_share, Sum entries) {
  if (U.fuse_e != -1 || !U.e_sampling || !x.done(U.ev_counts)) return false;
  U.e_share = U.e_reads ? (float)((double)entries() / (double)U.e_reads) : 0.f;
  U.fuse_e = U.e_share <= max_share ? -2 : 0;
  U.e_sampling = false;
  return true;
}
// The scan block's LDS has no room for the event ring beside this table: a role it stays.
template <class X> void tune_e_no_room(V2TuneSlotT<X> &U) { U.fuse_e = 0; }
// Whether a launch runs with list E inside the scan, and the pair its scan (start) and finishing launch (stop) carry when it
// is timed.  While the two forms are being timed, launches that may be timed (`free`: the rescue waves are settled by then,
// the call carries none of the caller's events and serves no sink) run E_FIRST times untimed as a role, E_PAIRS times as a
// role under a pair each, once fused and untimed (the other kernel's code is cold, the blocks' hints are the role form's),
// E_PAIRS times fused under a pair each — timed in turns the two forms paid for each switch and read within 1 % of each other
// on a box where the fused form is 5 % faster in the steady state —, and fused from then on until the six have completed.
template <class X> struct V2ListEStep {
  bool fused;
  const typename X::Event *start = nullptr, *stop = nullptr;
  bool read = false;                 // this launch read the samples (the slot's us_e[] say what they took)
};
template <class X> V2ListEStep<X> tune_list_e(V2TuneSlotT<X> &U, X &x, const bool free) {
  constexpr int NP = V2TuneSlotT<X>::E_PAIRS, FIRST = V2TuneSlotT<X>::E_FIRST;
  V2ListEStep<X> r{U.fuse_e == 1};
  if (U.fuse_e != -2 || U.choice == 0u || !free) return r;
  if (!U.ev_e[0][0] && !tune_create_pairs(x, U.ev_e, 2 * NP)) { U.fuse_e = 0; return r; }      // (no events: a role it stays)
  const int k = U.e_phase - FIRST;      // index of this launch among the timed ones
  if (k <= 2 * NP) {
    const int pair = k < 0 || k == NP ? -1 : (k < NP ? k : k - 1);
    if (pair >= 0) { r.start = &U.ev_e[pair][0]; r.stop = &U.ev_e[pair][1]; }
    r.fused = k >= NP;
    U.e_phase++;
    return r;
  }
  r.fused = true;      // (the fused form runs on while its samples are read: one switch fewer if it stays)
  const V2Timing t = tune_read_pairs(x, U.ev_e, 2 * NP, [](int i) { return i < NP ? 0 : 1; });
  if (t.ready) {
    U.us_e[0] = 1e3f * t.ms[0] / NP; U.us_e[1] = 1e3f * t.ms[1] / NP;
    U.fuse_e = (t.second_wins() && t.ms[1] > 0.f) ? 1 : 0;
    r.fused = U.fuse_e == 1; r.read = true;
  }
  return r;
}

}  // namespace dcrx

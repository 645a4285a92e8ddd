// mre_policy.h -- the launch scheduler's rules (mre_sched.cpp, mre_api.cpp) as pure functions over plain arrays: no HIP
// call, no handle, integer arithmetic on what the kernels report.  Host only; compiles with a plain C++ compiler and
// runs without a GPU (tests/sched_policy/).
#pragma once
#include <algorithm>

#include "mre_dev.h"

namespace mre {
namespace policy {

// Capacity of a group's ring of unprocessed launches, and of its staged records (<= RING outstanding launches + the
// record being written).  The depth in use is mre_env::ring.
constexpr int RING = 4;
constexpr int NSTAGE = RING + 1;

// ---- an env's launch-info record (StepArgs::launch_info)
inline int info_duration(const int* li) { return li[0] < 0 ? 0 : (li[1] >> 16); }   // (not part of the launch: 0)

// An env whose high-water marks came within 1/8 of a compact capacity is moved to the large kernel at a launch boundary
// (no re-run).  Round 5 measured the one place where this rule looks wasteful: a closed grasp is EXACTLY 57 robot rows
// (7 equality rows, two limits, 2 pads x 2 boxes x 4 contact points x 3) of the 62 the compact kernel holds, and 7/8 of 62
// is 54 -- every grasping env moves to the large kernel (bench.py's pick_place leg: 1825 promotions per 4096-env pair, 38 %
// of the batch at 6 instead of 8 workgroups per CU through the close / lift / home phases).  Moving an env only when one
// more contact would no longer fit (hw_nrrow + 3 > NRROW_MAX) cut the promotions to 1150 but raised the re-runs from 24
// to 278 -- the swing home adds a finger-cube or cube-cube contact within one 50-tick launch -- and the leg ran 8 % SLOWER
// (20.4 M vs 22.3 M env-steps/s, profiles/NOTES.md): a re-run repeats a whole launch of 50 ticks on the large kernel
// behind the group's stream, residency on the large kernel costs a quarter of the slots of the envs that are on it.  The 7/8 rule stays.
inline int compact_nrrow_max(bool newton) { return newton ? NRROW_MAX_COMPACT_NEWTON : NRROW_MAX_COMPACT_PGS; }
inline bool near_compact_caps(bool newton, int hw_ncon, int hw_nefc, int hw_nrrow, int hw_npp) {
  return 8 * hw_ncon > 7 * NCON_MAX || 8 * hw_nefc > 7 * NEFC_MAX || 8 * hw_nrrow > 7 * compact_nrrow_max(newton) || 8 * hw_npp > 7 * NPP_MAX;
}
// ... and a large env whose marks all fell to 5/8 of the compact capacities goes back
inline bool far_below_compact_caps(bool newton, int hw_ncon, int hw_nefc, int hw_nrrow, int hw_npp) {
  return 8 * hw_ncon <= 5 * NCON_MAX && 8 * hw_nefc <= 5 * NEFC_MAX && 8 * hw_nrrow <= 5 * compact_nrrow_max(newton) && 8 * hw_npp <= 5 * NPP_MAX;
}

// What the host does with one env after a launch, from the env's record and the host's flag for it ("large").
enum Action {
  NONE,         // nothing
  RERUN,        // overflowed the COMPACT kernel: put back to its saved rows and re-run on the large kernel, flagged large
                // from now on (whatever the host's flag says by now: a promotion decided one launch ago takes effect one
                // launch later)
  PROMOTE,      // within 1/8 of a compact capacity: move over BEFORE it overflows -- a promotion at a launch boundary
                // costs nothing, an overflow costs a re-run of the whole launch (a scripted phase is one launch of 2000 steps)
  DEMOTE,       // back below 5/8: to the compact kernel again
  HANDED_OVER,  // moved to the large kernel inside a queue launch: it finished the launch there, and stays
};
// The one rule, for pipelined, queue and synchronous launches alike.  A synchronous launch needs less of it: there the
// flags the kernels read ARE the host's flags (mre_sched.cpp uploads h_large whenever d_large_stale says the pipelined
// path changed it, and every other writer of h_large uploads at once), so an unflagged env ran on the compact kernel and
// reports only -1, 0 or 1, a flagged one ran on the large kernel and reports only -1, 0 or 2, and bit 2 -- "moved", set
// by queue launches only -- is never set.  On exactly those records this rule is the one the synchronous path used to
// carry (unflagged and > 0: re-run; flagged and 0: maybe demote); the records on which the two differed (unflagged 2, 4,
// 6; flagged 1) need device flags that differ from the host's or a queue launch (tests/test_sched_policy.py lists them).
inline Action decide(const int* li, bool large, bool newton, bool compact_only, bool large_only) {
  if (li[0] < 0) return NONE;   // not part of the launch, or skipped while it waited for a re-run
  const int hw_ncon = li[1] & 0xFFFF, hw_nefc = li[2], hw_nrrow = li[3] & 0xFFFF, hw_npp = li[3] >> 16;
  if ((li[0] & 4) != 0 && !large) return HANDED_OVER;
  if (li[0] == 1) return RERUN;
  if (!large) return !compact_only && near_compact_caps(newton, hw_ncon, hw_nefc, hw_nrrow, hw_npp) ? PROMOTE : NONE;
  return !large_only && li[0] == 0 && far_below_compact_caps(newton, hw_ncon, hw_nefc, hw_nrrow, hw_npp) ? DEMOTE : NONE;
}
inline bool flag_after(Action a, bool large) { return a == NONE ? large : a != DEMOTE; }

// Dispatch order for the next launch: a launch ends with its slowest wavefront, and the hardware hands
// workgroups to free slots in index order, so the envs that took longest in this launch (the kernel
// reports each env's own duration, s_memtime ticks >> 10) go first in the next one -- longest
// processing time first.  Counting sort over 256 duration buckets, stable; results do not depend on it.
// Orders the envs [lo, lo + n) by the duration in info[env][4] into order[lo .. lo + n) and returns the longest
// duration; 0 = no env of the range reported one, and `order` is left as it was (what then: the caller's).
inline int sort_longest_first(const int* info, int lo, int n, int* order) {
  int kmax = 0;
  for (int i = lo; i < lo + n; i++) kmax = std::max(kmax, info_duration(info + 4 * (size_t)i));
  if (kmax == 0) return 0;
  int count[258] = {0};
  auto bucket = [&](int i) { return (int)((long long)info_duration(info + 4 * (size_t)i) * 255 / kmax); };
  for (int i = lo; i < lo + n; i++) count[255 - bucket(i) + 1]++;
  for (int k = 1; k <= 256; k++) count[k] += count[k - 1];
  for (int i = lo; i < lo + n; i++) order[lo + count[255 - bucket(i)]++] = i;
  return kmax;
}

// Spread of one tick's durations over the envs [lo, lo + n) that took part: p99 env / mean env (mre_env::tick_tail).
// False (nothing reported) with fewer than 256 samples.  `scratch` holds n ints.
inline bool tick_tail_ratio(const int* info, int lo, int n, int* scratch, float* ratio) {
  size_t m = 0;
  long long sum = 0;
  for (int i = lo; i < lo + n; i++) {
    const int* li = info + 4 * (size_t)i;
    if (li[0] >= 0) { scratch[m++] = li[1] >> 16; sum += li[1] >> 16; }
  }
  if (m < 256 || sum <= 0) return false;
  const size_t k = m - 1 - m / 100;
  std::nth_element(scratch, scratch + k, scratch + m);
  *ratio = (float)scratch[k] * (float)m / (float)sum;
  return true;
}

// A staged record nobody reads: not the current one, not one of the `nyounger` outstanding launches behind the one
// being processed (at most RING - 1 of them, so one of the NSTAGE is always free).
inline int free_stage(int cur, const int* younger_stages, int nyounger) {
  bool used[NSTAGE] = {false};
  used[cur] = true;
  for (int k = 0; k < nyounger; k++) used[younger_stages[k]] = true;
  int fs = 0;
  while (used[fs]) fs++;
  return fs;
}

// Spare waves of the large kernel's WAITING launch (queue_large_waves below: `spare_large`), by need.  Each spare wave
// holds 26.5 KB of LDS on its compute unit for the whole launch (room for six compact waves there instead of eight) and
// is of use only when a compact wave hands an env over.  A launch that follows one without a hand-over keeps ONE; a
// launch that follows hand-overs keeps the 8 measured in mre_env.h.  MRE_QUEUE_SPARE_LARGE (`forced` >= 0) overrides
// both.  Results never depend on the count: whatever the waiting launch leaves is done by the large launch behind the
// compact kernel (mre_sched.cpp); only WHERE a hand-over waits does.
constexpr int QUEUE_SPARE_LARGE_QUIET = 1, QUEUE_SPARE_LARGE_BUSY = 8;
inline int queue_spare_large(int last_handovers, int forced) {
  if (forced >= 0) return forced;
  return last_handovers > 0 ? QUEUE_SPARE_LARGE_BUSY : QUEUE_SPARE_LARGE_QUIET;
}

// Waves of the large kernel's WAITING launch in a queue launch over the envs [lo, lo + n), `nl` of them flagged large
// (`large`: the flags the kernels will read; `info_last`: every env's latest record).
// A wave per env that is large already and some for those that come over (the spare waves, or as many as the launch
// processed last handed over) -- up to the share of the compute units'
// LDS that the large envs' share of the work asks for: with x large and y compact waves per unit (26.5 x + 20.4 y =
// 160 KB) both kinds finish together when (work of the large envs) / x = (work of the compact envs) / y.  A fixed cap
// of two per unit was right for the benchmark (a dozen large envs) and starved the whole-episode run at tuned gains,
// where 44 % of 8192 envs grasp at once: 25.8 -> 14.7 M env-steps/s inside step().  Never so many that a unit has no
// room for compact waves (x < 6 by construction): large waves wait for the compact ones to finish.
inline int queue_large_waves(const int* info_last, const uint8_t* large, int lo, int n, int nl, int last_handovers,
                             int spare_large, int large_waves_max /* 2 per compute unit */) {
  int lw = nl + std::max(last_handovers, spare_large);
  // (the two kinds' work from the envs' own latest durations where there are any: the large envs are the
  //  contact-rich ones, their ticks cost 1.3 .. 2.5 compact ticks depending on the phase)
  double wl = 0, wc = 0;
  for (int i = lo; i < lo + n; i++) {
    const double d = (double)info_duration(info_last + 4 * (size_t)i);
    if (large[i]) wl += d; else wc += d;
  }
  const double ncomp = (double)(n - nl);
  const double r = (wl > 0 && wc > 0) ? wl / wc : (ncomp > 0 ? 1.3 * (double)nl / ncomp : 1e9);
  const double x = r * 160.0 / (26.5 * r + 20.4);   // large waves per compute unit at balance
  const int bal = std::max((int)(x * (double)(large_waves_max / 2)), large_waves_max / 4);
  return std::max(std::min(lw, bal), 1);
}

// A batch that exceeds the GPU's wave slots (queue_waves: what the GPU holds of the queue kernel) can take queue launches
inline bool queue_fits(bool queue_ok, int queue_waves, int N) { return queue_ok && queue_waves > 0 && N > queue_waves; }
// ... and a window of `nticks` control ticks wants them from queue_min_ticks on (mre_env::queue_min_ticks), and from 8 ticks
// on unless the per-tick launches have measured a spread of a tick's durations below queue_tail_min (mre_env::tick_tail)
inline bool window_wants_queue(int nticks, int queue_min_ticks, bool tick_tail_valid, float tick_tail, float queue_tail_min) {
  return nticks >= queue_min_ticks || (nticks >= 8 && !(tick_tail_valid && tick_tail < queue_tail_min));
}

// At most ring - 1 launches stay unprocessed behind the one being enqueued -- and none behind a long one: a launch of many
// ticks (a chunk of mre_run_controller: 50 ticks) makes the 0.1 ms the host costs the chain irrelevant, while an env
// that overflows would have to be re-run for two such launches instead of one
inline int ring_keep(int nsteps, int ring) { return nsteps <= 50 ? ring - 1 : 0; }

}  // namespace policy
}  // namespace mre

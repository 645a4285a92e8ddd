// mre_env.h -- the handle behind the C ABI (struct mre_env) and what the two host units that work on it share: the
// four functions through which a handle comes to own a buffer, an event or a stream, the drain of pending launches that
// every entry point starts with, and the scheduler's three entry points (mre_sched.cpp); error reporting comes with
// mre_host.h.  Private to csrc/: mre_api.cpp and mre_sched.cpp include it, nothing else does.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mre.h"
#include "mre_dev.h"
#include "mre_host.h"
#include "mre_policy.h"

struct mre_env {
  int N = 0, device = 0;
  // Everything the handle has created on its device, recorded where it is created (alloc_dev, alloc_host, new_event,
  // new_stream below): mre_destroy walks these four records and names no buffer, event or stream.  The members further
  // down are views of them, for the code that launches.
  struct Owned {
    std::vector<void*> dev, host;   // hipMalloc / hipHostMalloc
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;
  } owned;
  hipStream_t stream = nullptr;
  mre::DevModel* dM = nullptr;
  mre::DevModel hM;
  int solver = MRE_SOLVER_PGS;   // mjtSolver (0 = PGS, 2 = Newton): selects the kernel instantiation (mre_set_solver)
  float *qpos = nullptr, *qvel = nullptr, *qacc_ws = nullptr, *ctrl = nullptr;
  float* qfine = nullptr;   // [N][QFINE_ROW] low-order words of the state: robot joints, then cube poses and velocities (StepArgs::qfine)
  int *nstep = nullptr, *sv_nstep = nullptr;   // [N] physics steps since the last reset (physics.data.time)
  int* nprops = nullptr;
  float* prop_size = nullptr;
  float* osc_target = nullptr;
  uint8_t* grip_closed = nullptr;
  uint8_t* converged = nullptr;
  uint8_t* mask = nullptr;
  float* sites = nullptr;
  uint32_t* status = nullptr;
  int* stats = nullptr;
  mre::OscConfig osc;
  mre::OscConfig* d_osc = nullptr;
  mre::OscConfig* d_osc_env = nullptr;   // [N] per-env controller parameters (mre_osc_configure_env) or null
  float* geoms = nullptr;        // [N][NG][16] geom poses for the renderer (allocated on first use)
  // cached image of the static geoms (ground, table) for the last camera: depth | rgb | seg
  float* bg_depth = nullptr; uint8_t* bg_rgb = nullptr; uint8_t* bg_seg = nullptr;
  float bg_key[16] = {0}; int bg_h = 0, bg_w = 0; bool bg_valid = false;
  uint8_t* prop_rgb = nullptr;   // [N][NPROP][3]
  float geom_rgb[mre::NG][3];   // albedo of every geom but the cubes (mre_set_render_colours)
  float* trace = nullptr;
  int trace_nenv = 0, trace_max = 0, trace_pos = 0;
  long long env_id_offset = 0;
  std::vector<long long> env_ids;  // explicit global ids (mre_set_env_ids) or empty = offset + index
  int* order = nullptr;       // dispatch permutation (heavy-first), device
  bool use_order = false;     // caller-supplied permutation (mre_set_env_order)
  int* auto_order = nullptr;  // permutation maintained by launch_step: longest Gauss-Seidel schedule first
  int* h_auto_order = nullptr;  // pinned host staging
  bool have_auto_order = false;
  bool profiling = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  size_t events_used = 0;
  // ---- capacity fallback (see launch_step): per-env kernel choice, pre-launch state copies
  bool fallback = true;
  unsigned base_flags = 0;    // StepFlags of every launch (F_CLIP_ALWAYS under MRE_NARROW_GENERIC=1, F_NW_ALL_TILES under MRE_NEWTON_GENERIC=1)
  bool large_only = false;    // mre_set_fallback(2): every env on the large kernel (reference run for the fallback)
  bool compact_only = false;  // mre_set_fallback(0): every env on the compact kernel
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_order = nullptr;
  uint8_t *d_large = nullptr, *mask_r = nullptr;
  float *sv_qpos = nullptr, *sv_qvel = nullptr, *sv_qacc_ws = nullptr, *sv_ctrl = nullptr, *sv_qfine = nullptr;
  uint32_t* sv_status = nullptr;
  uint8_t* sv_converged = nullptr;
  float* contacts = nullptr;     // device [N][1 + 3 * CONTACT_EXPORT] (detect launches), allocated on first use
  float* contacts_full = nullptr;  // device [N][CONTACT_EXPORT][12] (mre_get_contacts_full), allocated on first use
  int* settle_steps = nullptr;   // device [N]
  // Launch info and the per-launch inputs the host decides (dispatch order, large flags) live in MAPPED pinned host
  // memory that the step kernels store to / load from directly: no copy command sits in a group's launch chain
  // (round 3: one shader blit of 16 KB behind every group launch, 0.08 .. 3.9 ms each behind 2048 resident waves, and
  // two more in front of the next one).  d_* = the device-side address of the same bytes.
  int* h_launch_info = nullptr;  // [RING][N][4]: a group's launches in flight write one buffer each (ring slot)
  int* d_launch_info = nullptr;
  int* h_info_last = nullptr;    // the buffer (one of the two, per group region) that holds each env's latest record
  uint8_t* d_pending = nullptr;  // device [N]: env overflowed the compact kernel, waits for its re-run (StepArgs::pending)
  uint8_t* h_large_stage = nullptr;  // mapped [NSTAGE][N]: the large flags a pipelined launch reads (Group::cur)
  uint8_t* d_large_stage = nullptr;
  bool d_large_stale = false;        // the pipelined path changed h_large: d_large (synchronous launches) is behind
  std::vector<uint8_t> h_large, h_rerun;
  int n_large = 0;
  long long* d_env_ids = nullptr; // device copy of env_ids (pose search), null = offset + index
  // pose-search / sort_colours scratch (device, allocated on first use)
  int *ps_attempts = nullptr, *ps_prop = nullptr, *ps_tick = nullptr, *ps_which = nullptr;
  double *ps_bounds = nullptr, *ps_pose = nullptr, *ps_zones = nullptr, *ps_pick = nullptr;
  int last_settle_max = 0;
  long long n_reruns = 0, n_promotions = 0, n_demotions = 0;
  // ---- pipelined env groups (launch_step): the envs are cut into contiguous groups, each with its own stream
  // pair; a stepping call enqueues every group's launch and returns.  The tail of one group's launch (its slowest
  // envs) then overlaps the other groups' next launches instead of leaving the GPU idle.
  // A group's launch info is read -- and its fallback decisions taken -- LATE: with the default ring of two, launch
  // t + 1 of a group is enqueued behind launch t without the host in between (reading t's info first put the read-back,
  // the host's wake-up and the enqueue, 100 - 200 us, between every two launches of a chain whose launches last 800 us:
  // the kernel trace of the Newton bench), and t's info is processed when launch t + 2 is issued (or at the next call
  // that touches the state: drain()).  An env that overflows the compact kernel in launch t is therefore skipped by the
  // launches already enqueued behind it on the device (StepArgs::pending) and re-run for every one of them on the large
  // kernel (process_oldest).  MRE_RING = 3 / 4 keeps up to two / three launches enqueued behind the one being read.
  struct Group {
    int lo = 0, n = 0;
    hipStream_t st = nullptr, st2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    struct Out {           // a launch whose info has not been processed yet
      mre::StepArgs args;       // (a re-run uses them)
      hipEvent_t ev_info = nullptr;
      int stage = 0;       // the staged record (order + large flags) the launch reads
    } out[mre::policy::RING];   // ring of RING entries: out[head] is the oldest one
    int head = 0, nout = 0;
    int cur = 0;           // staged record new launches read: the latest complete one of NSTAGE
                           // (a record is rewritten only when no outstanding launch reads it)
    int* h_order = nullptr;  // mapped [NSTAGE][N] (entries [lo, lo + n) are the group's): its envs slowest first
    int* d_order = nullptr;
  };
  std::vector<Group> groups;
  int* h_grp_order = nullptr;   // mapped [NSTAGE][N]: per group, its envs slowest first (Group::h_order of `groups`)
  int* d_grp_order = nullptr;
  // Queue launches (StepArgs::q_head, k_step_queue): a rollout of several control ticks over more envs than the GPU holds
  // waves.  The groups above give every env a wave of its own per launch, and a group's next launch waits for the
  // group's slowest env: measured on the benchmark (tests/diagnostics/duration_trace.py, schedule_sim.py) the mean env
  // takes 0.35 - 0.39 ms per tick, the slowest env OF A TICK 0.86 - 1.0 ms (a different env every tick: an impact, a few
  // more Newton iterations), and the tick period sits at that maximum, 25 % above what the wave slots could deliver.
  // A queue launch has no per-tick barrier: all envs form one group (`qgroup`), the launch covers queue_ticks control
  // ticks, and its persistent waves take the env that is furthest behind -- a slow tick of one env delays nobody else.
  // The ring, the staged records, the capacity fallback and the re-runs are those of a group.  Per-tick callers
  // (mre_step, one-tick rollouts) keep the groups; the two never have launches outstanding at the same time.
  Group qgroup;
  bool queue_ok = true;         // MRE_QUEUE=0: never
  int queue_ticks = 200;        // control ticks per queue launch at most when the cut is the library's (MRE_QUEUE_TICKS, <= QUEUE_TICKS_MAX):
                                // measured 50 / 100 / 200 on the benchmark: 25.0 / 25.6 / 26.1 M env-steps/s (a launch ends with idle slots once)
  int queue_waves = 0;          // waves the GPU holds of the queue kernel (CUs x workgroups per CU; the smaller of the two solvers' kernels)
  int queue_shards = 16;        // ready lists per launch (MRE_QUEUE_SHARDS, <= QUEUE_SHARDS_MAX): see queue_pop
  int queue_lshards = 8;        // ... of the large kernel (MRE_QUEUE_LSHARDS, <= QUEUE_LSHARDS_MAX)
  bool queue_test_serial = false;
  // waves of the large kernel beyond the envs flagged large (MRE_QUEUE_SPARE_LARGE): they wait for hand-overs, and each
  // holds the LDS of 1.3 compact waves while it does -- measured on the benchmark (2 hand-overs per 200 ticks): 8 / 32 / 96
  // spare waves = 26.3 / 25.9 / 24.8 M env-steps/s.  Hand-overs beyond the spare waves queue up behind them.
  // < 0 (MRE_QUEUE_SPARE_LARGE not set): by need -- 1 after a launch without hand-overs, 8 after one with
  // (policy::queue_spare_large)
  int queue_spare_large = -1;
  // mre_run_controller's queue launches are shorter than a rollout's: a scripted phase moves hundreds of envs towards
  // the compact capacities at once (the grasp closes), and the host's 7/8 rule moves them at launch boundaries, before
  // they overflow -- measured on bench.py's pick_place leg: 50 / 100 / 200 ticks = 24.7 / 25.0 / 22.8 M (no queue: 21.8 M)
  int queue_run_ticks = 100;
  // A window shorter than this is stepped the old way when the cut is the library's (MRE_QUEUE_MIN_TICKS).  A queue launch
  // pays ~0.8 ms once (set-up, the ragged end of its last tick) and 7.6 us per item (take + acquire 4.1, release + list
  // 3.5: measured with s_memtime stamps) and wins by not waiting for each tick's slowest env.  On the driver's window
  // (20 ticks after 5, the lightest regime: a tick's slowest env is 1.5x the mean, against 2.5-3x later) the two cancel:
  // 30.3 M env-steps/s as one queue launch, 31.3 M as per-tick launches, same run; from ~30 ticks on the queue wins
  // everywhere measured (+19 % over 200 ticks).  A caller that asks for launches of k >= 2 ticks gets queue launches of k.
  int queue_min_ticks = 32;
  // ... and between 8 ticks and that, by what the per-tick launches themselves have measured: the spread of a tick's
  // durations (p99 env / mean env of one-tick group launches, smoothed; 1.28 in the lightest regime, 1.9-2.0 with the arms
  // on the table).  Below queue_tail_min the per-tick launches lose little to their slowest env and the window stays with
  // them; above it, or when nothing has been measured since the last reset, a window of >= 8 ticks is a queue launch (20
  // ticks in the heavy regime: 19.5 M env-steps/s against 16.1 M per tick).
  float tick_tail = 0.f;
  bool tick_tail_valid = false;
  float queue_tail_min = 1.45f;
  unsigned tail_samples = 0;
  std::vector<int> tail_scratch;
  int queue_large_waves_max = 0;  // 2 per compute unit (the unit of the balance in policy::queue_large_waves; no longer a cap)
  int* h_qlist = nullptr;       // pinned [RING + 1][N + 32]: counts per large shard [16], then the shards' lists of envs flagged large (+ 1)
  int* q_ws = nullptr;          // device: q_head[48][256] q_tail[48][256] q_done[16] q_acc[N][4] q_buf[QUEUE_TICKS_MAX][stride] (StepArgs)
  int* q_gen = nullptr;         // device, one word: StepArgs::q_gen
  int* h_q_err = nullptr;       // mapped: StepArgs::q_err
  int* h_qgrp_order = nullptr;  // mapped [NSTAGE][N]: qgroup's own staged dispatch orders
  long n_queue_launches = 0;
  long long n_handovers = 0;    // envs a queue launch moved to the large kernel itself
  int queue_last_handovers = 0; // ... in the launch processed last (the next launch keeps that many spare large waves)
  // Depth of a group's ring of unprocessed launches: capacity RING = 4, depth in use `ring` = 2 (MRE_RING = 2 .. 4).
  // Rounds 3 / 4 ran two with one library call per tick: a group that finished early sat idle until Python came back and
  // the host had served the slower groups (rocprofv3 kernel trace of the round-4 bench: 167 / 106 us between a launch's
  // end and the next start on the two high-priority streams, all four groups in flight 56 % of the span).  Round 5: the
  // caller hands over all the ticks of a window in ONE call (mre_rollout_ticks) and the loop that enqueues them runs
  // here.  A ring of four was built and measured with it: all four groups in flight 81 % of the span, idle gap 17 - 23 us
  // -- and 1.5 - 2 % SLOWER than a ring of two under the same single call (21.6 vs 22.0 M env-steps/s default, 19.1 vs
  // 19.4 M in the heavy regime, three runs each on one box): what a launch reads from the host -- its longest-first
  // dispatch order above all -- is as many launches old as the ring is deep, and the fresher order is worth more than
  // the shorter gap.  Two stays the default.
  static constexpr int RING = mre::policy::RING;
  int ring = 2;
  static constexpr int NSTAGE = mre::policy::NSTAGE;
  hipEvent_t ev_main = nullptr; // orders the group streams after the handle's stream
  float* seq_copy[RING + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // own copies of the last RING + 1 ctrl_seq arguments (re-runs read them later)
  size_t seq_cap = 0;
  unsigned seq_calls = 0;
  double dbg_wait_s = 0, dbg_call_s = 0; long dbg_calls = 0;   // MRE_DEBUG_TIMING
  // a caller that reads or writes the state after EVERY stepping call (a per-tick loop with host-side targets)
  // gains nothing from the groups and pays their launches: after two such calls in a row the stepping calls
  // go back to one launch of the whole batch, until two stepping calls arrive back to back again
  int calls_since_drain = 0, sync_streak = 0;
  // a pipelined launch failed half-way (a HIP error between the enqueue of a group's kernels and the record of its
  // event): launches of the group that were in flight may have skipped envs waiting for a re-run, and their saved rows
  // are gone -- the state is no longer the state of any rollout.  Every later call says so instead of stepping on.
  bool broken = false;
};

namespace mre {
// ---- the launch scheduler (mre_sched.cpp)
// the env groups, the queue state and their streams and events (from create_buffers; the handle owns them)
int sched_create(mre_env* e);
// One stepping launch of `a` over the batch: synchronous, pipelined over the env groups, or a queue launch.
int launch_step(mre_env* e, const StepArgs& a, bool settle = false, bool pipeline_ok = true, bool allow_queue = false);
// Complete every pending group launch: every entry point that reads or writes device state starts here.
int drain(mre_env* e, bool api_call = false);
}  // namespace mre

// ---- What a handle owns.  Each of the four selects the handle's device first (the HIP current device is per thread, and
// a caller with two handles may have moved it) and records what it made in mre_env::owned at once, so a failure half-way
// through mre_create or a first use leaks nothing: mre_destroy releases exactly what exists.
// A device buffer behind *p; a no-op when *p is set, so a buffer of first use is one call where it is needed.
template <class T> int alloc_dev(mre_env* e, T** p, size_t bytes) {
  if (*p) return MRE_OK;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMalloc((void**)p, bytes));
  e->owned.dev.push_back(*p);
  return MRE_OK;
}
// Pinned (hipHostMallocDefault) or mapped host memory; dev_alias: where the kernels see mapped bytes.
template <class T> int alloc_host(mre_env* e, T** p, size_t bytes, unsigned flags, T** dev_alias = nullptr) {
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipHostMalloc((void**)p, bytes, flags));
  e->owned.host.push_back(*p);
  if (dev_alias) HIPCHK(hipHostGetDevicePointer((void**)dev_alias, *p, 0));
  return MRE_OK;
}
inline int new_event(mre_env* e, hipEvent_t* ev, unsigned flags = hipEventDisableTiming) {
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipEventCreateWithFlags(ev, flags));
  e->owned.events.push_back(*ev);
  return MRE_OK;
}
// A non-blocking stream, of the default priority unless one is named.
inline int new_stream(mre_env* e, hipStream_t* s, const int* priority = nullptr) {
  HIPCHK(hipSetDevice(e->device));
  if (priority) HIPCHK(hipStreamCreateWithPriority(s, hipStreamNonBlocking, *priority));
  else HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  e->owned.streams.push_back(*s);
  return MRE_OK;
}
// A device buffer that is about to be replaced or dropped: freed, forgotten and nulled, so that whatever happens next
// the member and the record agree.  The caller has completed the work that reads it.
template <class T> void release(mre_env* e, T** p) {
  if (!*p) return;
  (void)hipFree(*p);
  auto& v = e->owned.dev;
  v.erase(std::remove(v.begin(), v.end(), (void*)*p), v.end());
  *p = nullptr;
}

// Where the low-order word of coordinate k of a qpos row (k < NQ) / of a qvel row (k < NV) sits in the env's qfine row:
// the robot's joints first, angles then velocities, then the cubes' poses, then their velocities.
constexpr int qfine_of_q(int k) { return k < mre::NRV ? k : mre::QFINE_CUBE_Q + (k - mre::NRV); }
constexpr int qfine_of_v(int k) { return k < mre::NRV ? mre::QFINE / 2 + k : mre::QFINE_CUBE_V + (k - mre::NRV); }

#define DRAIN(e) do { int rc_ = mre::drain(e, true); if (rc_) return rc_; } while (0)
#define DRAIN_PENDING(e) do { int rc_ = mre::drain(e, false); if (rc_) return rc_; } while (0)

// The HIP event pair that brackets a launch when the handle is profiling (mre_profile_enable), else two nulls.
inline int profile_events(mre_env* e, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!e->profiling) return MRE_OK;
  if (e->events_used == e->events.size()) {
    hipEvent_t x, y;
    int rc = new_event(e, &x, hipEventDefault);   // (timing enabled)
    if (!rc) rc = new_event(e, &y, hipEventDefault);
    if (rc) return rc;
    e->events.emplace_back(x, y);
  }
  *e0 = e->events[e->events_used].first; *e1 = e->events[e->events_used].second;
  e->events_used++;
  return MRE_OK;
}

// mre_api.cpp -- host side of the C ABI declared in include/mre.h.
// Owns the device buffers and the HIP stream of a batch of environments,
// uploads the fp32 DevModel that mre_model.cpp builds from the model blob, and
// enqueues kernels.  No torch types; plain pointers and sizes only.
#include <hip/hip_runtime.h>
#include <chrono>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/mre.h"
#include "mre_dev.h"
#include "mre_model.h"
#include "mre_records.h"

using namespace mre;

extern "C" void mre_launch_step(const StepArgs* args, hipStream_t stream);
extern "C" void mre_launch_settle(const StepArgs* args, hipStream_t stream);
extern "C" void mre_launch_step_large(const StepArgs* args, hipStream_t stream);
extern "C" void mre_launch_step_newton(const StepArgs* args, hipStream_t stream);
extern "C" void mre_launch_settle_newton(const StepArgs* args, hipStream_t stream);
extern "C" void mre_launch_step_queue(const StepArgs* args, int nwaves, hipStream_t stream);
extern "C" void mre_launch_step_queue_newton(const StepArgs* args, int nwaves, hipStream_t stream);
extern "C" void mre_launch_step_queue_large(const StepArgs* args, int nwaves, hipStream_t stream);
extern "C" void mre_launch_step_queue_large_newton(const StepArgs* args, int nwaves, hipStream_t stream);
extern "C" int mre_queue_waves_per_cu(void);
extern "C" int mre_queue_waves_per_cu_newton(void);
extern "C" void mre_launch_step_large_newton(const StepArgs* args, hipStream_t stream);
extern "C" void mre_launch_render(const RenderArgs* args, int row_groups, hipStream_t stream);
extern "C" void mre_launch_pack_final(int N, const float* qpos, const float* qvel, const uint32_t* status, float* out,
                                      hipStream_t stream);
extern "C" void mre_launch_restore_rows(const uint8_t* sel, int env0, int N, float* qpos, const float* sv_qpos, float* qvel,
                                        const float* sv_qvel, float* qacc_ws, const float* sv_qacc_ws, float* qfine,
                                        const float* sv_qfine, float* ctrl, const float* sv_ctrl, int* nstep,
                                        const int* sv_nstep, uint32_t* status, const uint32_t* sv_status,
                                        uint8_t* converged, const uint8_t* sv_converged, uint8_t* pending,
                                        hipStream_t stream);
extern "C" void mre_launch_pose_search(const SearchArgs* args, hipStream_t stream);
extern "C" void mre_launch_sort_select(const SortArgs* args, hipStream_t stream);
extern "C" void mre_launch_reset(const DevModel* M, int N, float* qpos, float* qvel, float* qacc_ws, float* qfine,
                                 float* ctrl, uint32_t* status, int* nstep, const uint8_t* mask,
                                 hipStream_t stream);


static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                       \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess)                                                               \
      return fail(MRE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));         \
  } while (0)

struct mre_env {
  int N = 0, device = 0;
  hipStream_t stream = nullptr;
  DevModel* dM = nullptr;
  DevModel hM;
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
  OscConfig osc;
  OscConfig* d_osc = nullptr;
  OscConfig* d_osc_env = nullptr;
  float* geoms = nullptr;        // [N][NG][16] geom poses for the renderer (allocated on first use)
  // cached image of the static geoms (ground, table) for the last camera: depth | rgb | seg
  float* bg_depth = nullptr; uint8_t* bg_rgb = nullptr; uint8_t* bg_seg = nullptr;
  float bg_key[16] = {0}; int bg_h = 0, bg_w = 0; bool bg_valid = false;
  uint8_t* prop_rgb = nullptr;   // [N][NPROP][3]
  float geom_rgb[NG][3];  // [N] per-env controller parameters (mre_osc_configure_env) or null
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
  bool large_only = false;
  bool compact_only = false;  // mre_set_fallback(0)  // mre_set_fallback(2): every env on the large kernel (reference run for the fallback)
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
      StepArgs args;       // (a re-run uses them)
      hipEvent_t ev_info = nullptr;
      int stage = 0;       // the staged record (order + large flags) the launch reads
    } out[4];              // ring of RING entries: out[head] is the oldest one
    int head = 0, nout = 0;
    int cur = 0;           // staged record new launches read: the latest complete one of NSTAGE
                           // (a record is rewritten only when no outstanding launch reads it)
    hipEvent_t p0 = nullptr, p1 = nullptr;   // profiling bracket of the launch being enqueued
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
  int queue_spare_large = 8;
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
  int queue_large_waves_max = 0;  // 2 per compute unit (the unit of the balance in launch_group_enqueue; no longer a cap)
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
  static constexpr int RING = 4;
  int ring = 2;
  static constexpr int NSTAGE = RING + 1;   // <= RING outstanding launches + the record being written
  static_assert(sizeof(Group::out) / sizeof(Group::Out) == RING, "Group::out is the ring");
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

// solver-specific instantiations of the step kernel (opt_solver of the model, mre_set_solver)
static void launch_compact(const mre_env* e, const StepArgs& a, hipStream_t st, bool settle = false) {
  const bool newton = e->solver == MRE_SOLVER_NEWTON;
  if (settle) { if (newton) mre_launch_settle_newton(&a, st); else mre_launch_settle(&a, st); }
  else { if (newton) mre_launch_step_newton(&a, st); else mre_launch_step(&a, st); }
}
static void launch_large(const mre_env* e, const StepArgs& a, hipStream_t st) {
  if (e->solver == MRE_SOLVER_NEWTON) mre_launch_step_large_newton(&a, st); else mre_launch_step_large(&a, st);
}

// Launch the step kernel, optionally bracketed by HIP events on the handle's stream.
//
// Capacity fallback.  The compact kernel (8 workgroups/CU) holds at most NCON_MAX / NEFC_MAX /
// NRROW_MAX / NPP_MAX constraints per env; a grasp or a pile needs more.  Every launch therefore
//   1. has every env copy its state rows (qpos, qvel, warm start, finger low words, ctrl, status) aside as
//      the step kernel loads them (StepArgs::sv_*),
//   2. runs the envs currently marked "large" on the large-capacity kernel (second stream; an env takes
//      part in the kernel that matches its flag, StepArgs::large / want_large) next to the compact kernel
//      for all others,
//   3. reads back per-env launch info (overflow flag + high-water marks of the launch),
//   4. restores the envs that overflowed on the compact kernel to their saved rows, marks them
//      large and runs them again on the large kernel -- so no result ever depends on the compact
//      capacities; it also moves envs whose high-water marks came within 1/8 of a compact capacity
//      (no re-run needed at a launch boundary) and demotes large envs that fell below 5/8.
// Only an overflow of the LARGE capacities is reported (MRE_ST_CONTACT_OVERFLOW).
static int profile_events(mre_env* e, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!e->profiling) return MRE_OK;
  if (e->events_used == e->events.size()) {
    hipEvent_t x, y;
    HIPCHK(hipEventCreate(&x)); HIPCHK(hipEventCreate(&y));
    e->events.emplace_back(x, y);
  }
  *e0 = e->events[e->events_used].first; *e1 = e->events[e->events_used].second;
  e->events_used++;
  return MRE_OK;
}

// An env whose high-water marks came within 1/8 of a compact capacity is moved to the large kernel at a launch boundary
// (no re-run).  Round 5 measured the one place where this rule looks wasteful: a closed grasp is EXACTLY 57 robot rows
// (7 equality rows, two limits, 2 pads x 2 boxes x 4 contact points x 3) of the 62 the compact kernel holds, and 7/8 of 62
// is 54 -- every grasping env moves to the large kernel (bench.py's pick_place leg: 1825 promotions per 4096-env pair, 38 %
// of the batch at 6 instead of 8 workgroups per CU through the close / lift / home phases).  Moving an env only when one
// more contact would no longer fit (hw_nrrow + 3 > NRROW_MAX) cut the promotions to 1150 but raised the re-runs from 24
// to 278 -- the swing home adds a finger-cube or cube-cube contact within one 50-tick launch -- and the leg ran 8 % SLOWER
// (20.4 M vs 22.3 M env-steps/s, profiles/NOTES.md): a re-run repeats a whole launch of 50 ticks on the large kernel
// behind the group's stream, residency on the large kernel costs a quarter of the slots of the envs that are on it.  The 7/8 rule stays.
static inline int compact_nrrow_max(const mre_env* e) {
  return e->solver == MRE_SOLVER_NEWTON ? NRROW_MAX_COMPACT_NEWTON : NRROW_MAX_COMPACT_PGS;
}
static inline bool near_compact_caps(const mre_env* e, int hw_ncon, int hw_nefc, int hw_nrrow, int hw_npp) {
  return 8 * hw_ncon > 7 * NCON_MAX || 8 * hw_nefc > 7 * NEFC_MAX || 8 * hw_nrrow > 7 * compact_nrrow_max(e) || 8 * hw_npp > 7 * NPP_MAX;
}

// Dispatch order of a group: its envs by the duration in their launch-info record, longest first (counting sort over 256
// buckets, stable; results do not depend on it).
static void sort_longest_first(const mre_env::Group& G, const int* info, int kmax, int* order_stage) {
  int count[258] = {0};
  auto bucket = [&](int i) {
    const int* li = info + 4 * (size_t)i;
    return (int)((long long)(li[0] < 0 ? 0 : (li[1] >> 16)) * 255 / kmax);
  };
  for (int i = G.lo; i < G.lo + G.n; i++) count[255 - bucket(i) + 1]++;
  for (int k = 1; k <= 256; k++) count[k] += count[k - 1];
  for (int i = G.lo; i < G.lo + G.n; i++) order_stage[G.lo + count[255 - bucket(i)]++] = i;
}

// Read the launch info of a group's OLDEST outstanding launch and act on it (see launch_step): promotions /
// demotions, dispatch order of the group's next launch, re-run of the envs that overflowed the compact kernel --
// for that launch and for the younger outstanding one, which skipped them.
static int process_oldest(mre_env* e, mre_env::Group& G) {
  if (G.nout == 0) return MRE_OK;
  const int slot = G.head;
  mre_env::Group::Out& O = G.out[slot];
  {
    const auto w0 = std::chrono::steady_clock::now();
    HIPCHK(hipEventSynchronize(O.ev_info));
    e->dbg_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
  }
  if (e->h_q_err && *e->h_q_err != 0) {
    e->broken = true;
    return fail(MRE_ERR_HIP, "queue launch: an env listed as ready never arrived (internal error)");
  }
  const int* const info = e->h_launch_info + (size_t)slot * 4 * (size_t)e->N;
  // a staged record nobody reads: not the current one, not the younger outstanding launch's
  int fs = 0;
  {
    bool used[mre_env::NSTAGE] = {false};
    used[G.cur] = true;
    for (int k = 1; k < G.nout; k++) used[G.out[(slot + k) % mre_env::RING].stage] = true;   // the younger outstanding launches'
    while (used[fs]) fs++;
  }
  int* const order_stage = G.h_order + (size_t)fs * (size_t)e->N;
  int nrerun = 0;
  bool changed = false;
  int kmax = 0;
  const long long handovers0 = e->n_handovers;
  for (int i = G.lo; i < G.lo + G.n; i++) {
    const int* li = info + 4 * (size_t)i;
    e->h_rerun[i] = 0;
    if (li[0] < 0) continue;   // not part of the launch, or skipped while it waited for a re-run
    const int hw_ncon = li[1] & 0xFFFF, hw_nefc = li[2], hw_nrrow = li[3] & 0xFFFF, hw_npp = li[3] >> 16;
    if ((li[1] >> 16) > kmax) kmax = li[1] >> 16;
    if ((li[0] & 4) != 0 && !e->h_large[i]) {
      // handed over to the large kernel inside a queue launch: it finished the launch there, and stays
      e->h_large[i] = 1; changed = true; e->n_large++; e->n_promotions++; e->n_handovers++;
    } else if (li[0] == 1) {
      // overflowed the COMPACT kernel (whatever the host's flag says by now: a promotion decided one launch ago
      // takes effect one launch later)
      e->h_rerun[i] = 1; nrerun++;
      if (!e->h_large[i]) { e->h_large[i] = 1; changed = true; e->n_large++; e->n_promotions++; }
    } else if (!e->h_large[i]) {
      if (!e->compact_only && near_compact_caps(e, hw_ncon, hw_nefc, hw_nrrow, hw_npp)) {
        e->h_large[i] = 1; changed = true; e->n_large++; e->n_promotions++;
      }
    } else if (!e->large_only && li[0] == 0 && 8 * hw_ncon <= 5 * NCON_MAX && 8 * hw_nefc <= 5 * NEFC_MAX &&
               8 * hw_nrrow <= 5 * compact_nrrow_max(e) && 8 * hw_npp <= 5 * NPP_MAX) {
      e->h_large[i] = 0; changed = true; e->n_large--; e->n_demotions++;
    }
  }
  if (&G == &e->qgroup) e->queue_last_handovers = (int)(e->n_handovers - handovers0);
  else if (O.args.nsteps == O.args.control_steps && (e->tail_samples++ & 3u) == 0u && G.n >= 256) {
    // spread of this tick's durations over the group's envs (mre_env::tick_tail)
    std::vector<int>& d = e->tail_scratch;
    d.clear();
    long long sum = 0;
    for (int i = G.lo; i < G.lo + G.n; i++) {
      const int* li = info + 4 * (size_t)i;
      if (li[0] >= 0) { d.push_back(li[1] >> 16); sum += li[1] >> 16; }
    }
    if (d.size() >= 256 && sum > 0) {
      const size_t k = d.size() - 1 - d.size() / 100;
      std::nth_element(d.begin(), d.begin() + k, d.end());
      const float ratio = (float)d[k] * (float)d.size() / (float)sum;
      e->tick_tail = e->tick_tail_valid ? 0.9f * e->tick_tail + 0.1f * ratio : ratio;
      e->tick_tail_valid = true;
    }
  }
  // (what is decided here takes effect with the NEXT launch enqueued for the group -- the one after the younger
  //  outstanding launch -- which reads the staged record straight from mapped host memory)
  if (kmax > 0) {   // longest processing time first within the group (counting sort, stable)
    sort_longest_first(G, info, kmax, order_stage);
  } else {
    memcpy(order_stage + G.lo, G.h_order + (size_t)G.cur * (size_t)e->N + G.lo, (size_t)G.n * 4);
  }
  if (nrerun > 0) {
    HIPCHK(hipMemcpyAsync(e->mask_r + G.lo, e->h_rerun.data() + G.lo, (size_t)G.n, hipMemcpyHostToDevice, G.st));
    mre_launch_restore_rows(e->mask_r, G.lo, G.n, e->qpos, e->sv_qpos, e->qvel, e->sv_qvel, e->qacc_ws, e->sv_qacc_ws,
                            e->qfine, e->sv_qfine, e->ctrl, e->sv_ctrl, e->nstep, e->sv_nstep, e->status, e->sv_status,
                            e->converged, e->sv_converged, e->d_pending, G.st);
    // the launch that overflowed, then the younger outstanding launches (which left these envs alone)
    for (int k = 0; k < G.nout; k++) {
      StepArgs ar = G.out[(slot + k) % mre_env::RING].args;
      ar.env_mask = e->mask_r; ar.launch_info = nullptr; ar.large = nullptr; ar.sv_qpos = nullptr; ar.pending = nullptr;
      ar.q_head = nullptr;   // (one wave per env for the whole launch, whatever the launch itself was)
      launch_large(e, ar, G.st);
      HIPCHK(hipGetLastError());
    }
    e->n_reruns += nrerun;
  }
  memcpy(e->h_large_stage + (size_t)fs * (size_t)e->N + G.lo, e->h_large.data() + G.lo, (size_t)G.n);
  G.cur = fs;
  if (changed) e->d_large_stale = true;
  if (nrerun > 0) HIPCHK(hipStreamSynchronize(G.st));   // (h_rerun is pageable: the staged bytes must outlive the upload)
  // the latest record of every env of the group (mre_get_launch_info)
  for (int i = G.lo; i < G.lo + G.n; i++) {
    const int* li = info + 4 * (size_t)i;
    if (li[0] != -2) memcpy(e->h_info_last + 4 * (size_t)i, li, 16);
  }
  G.head = (G.head + 1) % mre_env::RING;
  G.nout--;
  return MRE_OK;
}

static int drain_group(mre_env* e, mre_env::Group& G, bool sync_idle = false) {
  if (G.nout == 0 && !sync_idle) return MRE_OK;
  while (G.nout > 0) {
    int rc = process_oldest(e, G);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(G.st));
  return MRE_OK;
}
// Complete every pending group launch: every entry point that reads or writes device state starts here.
static int drain(mre_env* e, bool api_call = false) {
  if (e->broken) return fail(MRE_ERR_HIP, "an earlier stepping call failed while its launches were being enqueued: the "
                                          "state of this handle is undefined (mre_destroy it, create a new one)");
  if (api_call) {
    if (e->calls_since_drain == 1) e->sync_streak++;
    else if (e->calls_since_drain > 1) e->sync_streak = 0;
    e->calls_since_drain = 0;
  }
  bool any = e->qgroup.nout > 0;
  for (auto& G : e->groups) any = any || G.nout > 0;
  if (!any) return MRE_OK;
  HIPCHK(hipSetDevice(e->device));
  for (auto& G : e->groups) {
    int rc = drain_group(e, G, true);
    if (rc) return rc;
  }
  return drain_group(e, e->qgroup, true);
}
#define DRAIN(e) do { int rc_ = drain(e, true); if (rc_) return rc_; } while (0)
#define DRAIN_PENDING(e) do { int rc_ = drain(e, false); if (rc_) return rc_; } while (0)

// a launch under the capacity fallback: split by the envs' flags, state rows copied aside, launch info reported
static void guard_args(mre_env* e, StepArgs& a) {
  a.large = e->d_large; a.launch_info = e->d_launch_info;
  a.sv_qpos = e->sv_qpos; a.sv_qvel = e->sv_qvel; a.sv_qacc_ws = e->sv_qacc_ws; a.sv_qfine = e->sv_qfine;
  a.sv_ctrl = e->sv_ctrl; a.sv_status = e->sv_status; a.sv_converged = e->sv_converged; a.sv_nstep = e->sv_nstep;
}

// One group's part of a stepping call: finish its previous launch, enqueue the new one, do not wait.
static int launch_group_enqueue(mre_env* e, mre_env::Group& G, const StepArgs& a_full, bool queue);
static int launch_group(mre_env* e, mre_env::Group& G, const StepArgs& a_full, bool queue = false) {
  // at most ring - 1 launches stay unprocessed behind the one enqueued here -- and none behind a long one: a launch of many
  // ticks (a chunk of mre_run_controller: 50 ticks) makes the 0.1 ms the host costs the chain irrelevant, while an env
  // that overflows would have to be re-run for two such launches instead of one
  const int keep = a_full.nsteps <= 50 ? e->ring - 1 : 0;
  while (G.nout > keep) {
    int rc = process_oldest(e, G);
    if (rc) return rc;
  }
  int rc = launch_group_enqueue(e, G, a_full, queue);
  if (rc) {
    // something failed after part of the launch was enqueued: nothing may stay in flight behind an event that was
    // never recorded (a later drain() would wait for it)
    (void)hipStreamSynchronize(G.st);
    (void)hipStreamSynchronize(G.st2);
    G.nout = 0; G.head = 0;
    (void)hipMemset(e->d_pending + G.lo, 0, (size_t)G.n);
    e->broken = true;
  }
  return rc;
}
static int launch_group_enqueue(mre_env* e, mre_env::Group& G, const StepArgs& a_full, bool queue) {
  int rc;
  StepArgs a = a_full;
  const size_t N = (size_t)e->N;
  // first launch of a burst (nothing of the group in flight): other entry points may have changed the flags since --
  // and the envs' latest durations may come from launches of ANOTHER group (the queue's group covers all envs; the
  // per-tick groups a quarter each): the burst starts with the order they give, not with the one this group left behind
  // (measured: 20 per-tick launches after a queue window of 200 ticks, 15.7 -> 16.1 M env-steps/s)
  if (G.nout == 0) {
    memcpy(e->h_large_stage + (size_t)G.cur * N + G.lo, e->h_large.data() + G.lo, (size_t)G.n);
    int kmax = 0;
    for (int i = G.lo; i < G.lo + G.n; i++) {
      const int* li = e->h_info_last + 4 * (size_t)i;
      if (li[0] >= 0 && (li[1] >> 16) > kmax) kmax = li[1] >> 16;
    }
    if (kmax > 0) sort_longest_first(G, e->h_info_last, kmax, G.h_order + (size_t)G.cur * N);
  }
  a.N = G.n; a.env_order = G.d_order + (size_t)G.cur * N + G.lo; a.seq_stride = e->N;
  rc = profile_events(e, &G.p0, &G.p1);
  if (rc) return rc;
  HIPCHK(hipStreamWaitEvent(G.st, e->ev_main, 0));
  if (G.p0) HIPCHK(hipEventRecord(G.p0, G.st));
  guard_args(e, a);
  a.pending = e->d_pending;
  const int slot = (G.head + G.nout) % mre_env::RING;
  a.large = e->d_large_stage + (size_t)G.cur * N;
  a.launch_info = e->d_launch_info + (size_t)slot * 4 * N;
  StepArgs ac = a;
  ac.want_large = 0;
  bool run_large = false;
  const uint8_t* const fl = e->h_large_stage + (size_t)G.cur * N;   // (the very flags the kernels will read)
  if (queue) {
    // Queue launch: compact waves on G.st, the large kernel's waves next to them on G.st2 (capacity fallback inside the
    // launch: mre_kernels.hip, queue_pop).  Ready lists, per-env accumulators and the count of finished envs start at
    // zero (one block from the allocation's start, a multiple of 16 bytes); the envs flagged large are bucket 0 of the
    // large shard.
    const int nt = a.nsteps / a.control_steps, S = e->queue_shards, cap = (G.n + S - 1) / S;
    const int SL = e->queue_lshards, capl = (G.n + SL - 1) / SL;
    constexpr int QS = QUEUE_SHARDS_MAX + QUEUE_LSHARDS_MAX;
    const size_t ctl = 2 * (size_t)QS * QUEUE_TICKS_MAX + 16;
    const size_t stride = (size_t)S * cap + (size_t)SL * capl;
    const size_t words = ctl + 4 * N + (size_t)nt * stride;
    ac.sv_qpos = nullptr;   // (nothing is re-run: no rows to put back)
    ac.q_head = e->q_ws; ac.q_tail = ac.q_head + QS * QUEUE_TICKS_MAX;
    ac.q_done = ac.q_tail + QS * QUEUE_TICKS_MAX; ac.q_started = ac.q_done + 1; ac.q_acc = ac.q_done + 16;
    ac.q_buf = ac.q_acc + 4 * N; ac.q_err = e->h_q_err; ac.q_nticks = nt; ac.q_shards = S; ac.q_cap = cap; ac.q_stride = (int)stride;
    ac.q_lshards = SL; ac.q_capl = capl;
    ac.q_gen = e->q_gen; ac.q_gen_expect = (int)(e->n_queue_launches + 1);
    // the envs flagged large, per large shard (env e: shard e % SL, in env order): counts in hl[0 .. SL), lists from hl[16]
    int* const hl = e->h_qlist + (size_t)(e->n_queue_launches % (mre_env::RING + 1)) * (N + 32);
    int nl = 0;
    for (int j = 0; j < SL; j++) hl[j] = 0;
    memset(hl + 16, 0, (size_t)SL * capl * 4);
    for (int i = G.lo; i < G.lo + G.n; i++)
      if (fl[i]) { const int j = i % SL; hl[16 + (size_t)j * capl + hl[j]++] = i + 1; nl++; }   // (the queue's group is all envs: lo = 0)
    run_large = true;
    // 1. the large kernel's waiting launch, first: see step_body (q_gen)
    StepArgs al = ac;
    al.want_large = 1; al.q_wait = 1;
    // A wave per env that is large already and some for those that come over -- up to the share of the compute units'
    // LDS that the large envs' share of the work asks for: with x large and y compact waves per unit (26.5 x + 20.4 y =
    // 160 KB) both kinds finish together when (work of the large envs) / x = (work of the compact envs) / y.  A fixed cap
    // of two per unit was right for the benchmark (a dozen large envs) and starved the whole-episode run at tuned gains,
    // where 44 % of 8192 envs grasp at once: 25.8 -> 14.7 M env-steps/s inside step().  Never so many that a unit has no
    // room for compact waves (x < 6 by construction): large waves wait for the compact ones to finish.
    int lw = nl + (e->queue_last_handovers > e->queue_spare_large ? e->queue_last_handovers : e->queue_spare_large);
    {
      // (the two kinds' work from the envs' own latest durations where there are any: the large envs are the
      //  contact-rich ones, their ticks cost 1.3 .. 2.5 compact ticks depending on the phase)
      double wl = 0, wc = 0;
      for (int i = G.lo; i < G.lo + G.n; i++) {
        const int* li = e->h_info_last + 4 * (size_t)i;
        const double d = li[0] >= 0 ? (double)(li[1] >> 16) : 0.0;
        if (fl[i]) wl += d; else wc += d;
      }
      const double ncomp = (double)(G.n - nl);
      const double r = (wl > 0 && wc > 0) ? wl / wc : (ncomp > 0 ? 1.3 * (double)nl / ncomp : 1e9);
      const double x = r * 160.0 / (26.5 * r + 20.4);   // large waves per compute unit at balance
      int bal = (int)(x * (double)(e->queue_large_waves_max / 2));   // (queue_large_waves_max = 2 per unit)
      if (bal < e->queue_large_waves_max / 4) bal = e->queue_large_waves_max / 4;
      if (lw > bal) lw = bal;
    }
    if (lw < 1) lw = 1;
    // (test knob MRE_QUEUE_TEST_SERIAL=1: on the compact kernel's own stream, i.e. strictly before it -- what a profiler
    //  that serialises dispatches makes of the two streams; the launch then leaves after its bounded wait and the one
    //  behind the compact kernel does the large kernel's whole share)
    hipStream_t const st_large = e->queue_test_serial ? G.st : G.st2;
    if (e->solver == MRE_SOLVER_NEWTON) mre_launch_step_queue_large_newton(&al, lw, st_large);
    else mre_launch_step_queue_large(&al, lw, st_large);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(G.ev_join, st_large));
    // 2. the lists, then the launch's number
    HIPCHK(hipMemsetAsync(e->q_ws, 0, ((words * 4 + 15) / 16) * 16, G.st));
    if (nl > 0) {
      HIPCHK(hipMemcpyAsync(ac.q_buf + (size_t)S * cap, hl + 16, (size_t)SL * capl * 4, hipMemcpyHostToDevice, G.st));
      // (bucket 0's tail word of every large shard: one word per row of QUEUE_TICKS_MAX)
      HIPCHK(hipMemcpy2DAsync(ac.q_tail + S * QUEUE_TICKS_MAX, (size_t)QUEUE_TICKS_MAX * 4, hl, 4, 4, (size_t)SL, hipMemcpyHostToDevice, G.st));
    }
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->q_gen, ac.q_gen_expect, 1, G.st));
    // 3. the compact kernel
    const int nwaves = G.n < e->queue_waves ? G.n : e->queue_waves;
    if (e->solver == MRE_SOLVER_NEWTON) mre_launch_step_queue_newton(&ac, nwaves, G.st);
    else mre_launch_step_queue(&ac, nwaves, G.st);
    HIPCHK(hipGetLastError());
    // Behind the compact kernel, the large kernel once more, not waiting: nothing to do when the two ran side by side
    // (a few microseconds), the rest of the job when they did not -- results never depend on how the GPU overlaps them.
    // (as many waves as the GPU holds of the large kernel: when a scripted phase closes hundreds of grasps inside one
    //  launch, the hand-overs outnumber the waiting launch's spare waves and pile up behind them -- here, with the compact
    //  kernel gone, they all run at once)
    al.q_wait = 0;
    const int sweep = G.n < 3 * e->queue_large_waves_max ? G.n : 3 * e->queue_large_waves_max;
    if (e->solver == MRE_SOLVER_NEWTON) mre_launch_step_queue_large_newton(&al, sweep, G.st);
    else mre_launch_step_queue_large(&al, sweep, G.st);
    e->n_queue_launches++;
  } else {
    for (int i = G.lo; i < G.lo + G.n && !run_large; i++) run_large = fl[i] != 0;
    if (run_large) {
      HIPCHK(hipEventRecord(G.ev_fork, G.st));
      HIPCHK(hipStreamWaitEvent(G.st2, G.ev_fork, 0));
      StepArgs al = a;
      al.want_large = 1;
      launch_large(e, al, G.st2);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(G.ev_join, G.st2));
    }
    launch_compact(e, ac, G.st, false);
  }
  HIPCHK(hipGetLastError());
  if (run_large) HIPCHK(hipStreamWaitEvent(G.st, G.ev_join, 0));
  if (G.p1) HIPCHK(hipEventRecord(G.p1, G.st));
  // (the kernels stored their 16 B of launch info per env into mapped host memory: the event is all that follows)
  HIPCHK(hipEventRecord(G.out[slot].ev_info, G.st));
  G.out[slot].args = a;
  G.out[slot].stage = G.cur;
  G.nout++;
  return MRE_OK;
}

static int launch_step(mre_env* e, const StepArgs& a, bool settle = false, bool pipeline_ok = true, bool allow_queue = false) {
  if (e->broken) return drain(e);   // (reports the failure)
  HIPCHK(hipSetDevice(e->device));  // the HIP current device is per thread; callers may have moved it
  {
    const bool guarded_ = e->fallback && a.nsteps > 0 && (a.flags & F_NO_CONSTRAINTS) == 0;
    if (++e->calls_since_drain >= 2) e->sync_streak = 0;
    const bool pipelined = pipeline_ok && e->sync_streak < 2 && e->groups.size() > 1 && guarded_ && !settle && a.env_mask == nullptr && !e->use_order &&
                           a.trace == nullptr && a.contacts == nullptr && a.settle_steps == nullptr && a.geoms == nullptr &&
                           (a.flags & (F_DETECT | F_SETTLE_EXIT | F_OSC_EVAL)) == 0;
    // a rollout of several ticks over more envs than the GPU holds waves: one queue launch of all envs (mre_env::qgroup)
    const bool queue = allow_queue && e->queue_ok && pipeline_ok && guarded_ && !e->compact_only && !e->large_only && !settle && (a.mode == CTRL_SEQ || a.mode == CTRL_OSC) && a.env_mask == nullptr && !e->use_order &&
                       a.contacts == nullptr && a.settle_steps == nullptr && a.geoms == nullptr &&
                       (a.flags & (F_DETECT | F_SETTLE_EXIT | F_OSC_EVAL)) == 0 && a.control_steps > 0 &&
                       a.nsteps % a.control_steps == 0 && a.nsteps >= 2 * a.control_steps &&
                       a.nsteps <= QUEUE_TICKS_MAX * a.control_steps && e->queue_waves > 0 && e->N > e->queue_waves;
    if (queue) {
      for (auto& G : e->groups) { int rc = drain_group(e, G); if (rc) return rc; }
      HIPCHK(hipEventRecord(e->ev_main, e->stream));
      int rc = launch_group(e, e->qgroup, a, true);
      // (a caller with a trace buffer reads it when the call returns: stepping calls with a trace have always completed first)
      if (!rc && a.trace != nullptr) rc = drain_group(e, e->qgroup);
      return rc;
    }
    { int rc = drain_group(e, e->qgroup); if (rc) return rc; }
    if (pipelined) {
      struct Timer { mre_env* e; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                     ~Timer() { e->dbg_call_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); e->dbg_calls++; } } timer_{e};
      HIPCHK(hipEventRecord(e->ev_main, e->stream));
      // serve the groups in the order their previous launches complete
      const size_t ng = e->groups.size();
      bool done[8] = {false, false, false, false, false, false, false, false};
      for (size_t left = ng; left > 0;) {
        size_t pick = ng;
        for (size_t g = 0; g < ng && pick == ng; g++)
          if (!done[g] && (e->groups[g].nout <= (a.nsteps <= 50 ? e->ring - 1 : 0) ||   // (launch_group's `keep`: nothing to wait for)
                           hipEventQuery(e->groups[g].out[e->groups[g].head].ev_info) == hipSuccess)) pick = g;
        (void)hipGetLastError();   // (hipErrorNotReady of a query is not an error)
        if (pick == ng) {          // none ready: wait for the first outstanding one
          for (size_t g = 0; g < ng && pick == ng; g++) if (!done[g]) pick = g;
        }
        int rc = launch_group(e, e->groups[pick], a);
        if (rc) return rc;
        done[pick] = true; left--;
      }
      return MRE_OK;
    }
    DRAIN_PENDING(e);
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (e->profiling) {
    if (e->events_used == e->events.size()) {
      hipEvent_t x, y;
      HIPCHK(hipEventCreate(&x)); HIPCHK(hipEventCreate(&y));
      e->events.emplace_back(x, y);
    }
    e0 = e->events[e->events_used].first; e1 = e->events[e->events_used].second;
    e->events_used++;
    HIPCHK(hipEventRecord(e0, e->stream));
  }
  const bool guarded = e->fallback && a.nsteps > 0 && (a.flags & F_NO_CONSTRAINTS) == 0;
  if (!guarded) {
    launch_compact(e, a, e->stream, settle);
    HIPCHK(hipGetLastError());
  } else {
    const size_t N = (size_t)e->N;
    if (e->d_large_stale) {   // promotions / demotions decided by the pipelined path since the last synchronous launch
      HIPCHK(hipMemcpyAsync(e->d_large, e->h_large.data(), N, hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      e->d_large_stale = false;
    }
    StepArgs ac = a;
    guard_args(e, ac);
    ac.want_large = 0;
    // (recounted from the flags every launch: an env flagged large is masked out of the compact
    // kernel, so the large kernel MUST run whenever a flag is set)
    e->n_large = 0;
    for (size_t i = 0; i < N; i++) e->n_large += e->h_large[i];
    const bool run_large = e->n_large > 0;
    if (run_large) {
      HIPCHK(hipEventRecord(e->ev_fork, e->stream));
      HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
      StepArgs al = ac;
      al.want_large = 1;
      launch_large(e, al, e->stream2);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(e->ev_join, e->stream2));
    }
    launch_compact(e, ac, e->stream, settle);
    HIPCHK(hipGetLastError());
    if (run_large) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    HIPCHK(hipStreamSynchronize(e->stream));   // (launch info: stored to mapped host memory by the kernels)
    memcpy(e->h_info_last, e->h_launch_info, N * 16);
    int nrerun = 0;
    bool changed = false;
    for (size_t i = 0; i < N; i++) {
      const int* li = e->h_launch_info + 4 * i;
      e->h_rerun[i] = 0;
      if (li[0] < 0) continue;
      const int hw_ncon = li[1] & 0xFFFF, hw_nefc = li[2], hw_nrrow = li[3] & 0xFFFF, hw_npp = li[3] >> 16;
      if (!e->h_large[i]) {
        if (li[0] > 0) {  // overflowed the compact kernel: re-run this launch on the large one
          e->h_rerun[i] = 1; e->h_large[i] = 1; nrerun++; changed = true; e->n_large++; e->n_promotions++;
        } else if (!e->compact_only && near_compact_caps(e, hw_ncon, hw_nefc, hw_nrrow, hw_npp)) {
          // within 1/8 of a compact capacity: move over BEFORE it overflows -- a promotion at a launch
          // boundary costs nothing, an overflow costs a re-run of the whole launch (a scripted phase
          // is one launch of 2000 steps)
          e->h_large[i] = 1; changed = true; e->n_large++; e->n_promotions++;
        }
      } else if (!e->large_only && li[0] == 0 && 8 * hw_ncon <= 5 * NCON_MAX && 8 * hw_nefc <= 5 * NEFC_MAX &&
                 8 * hw_nrrow <= 5 * compact_nrrow_max(e) && 8 * hw_npp <= 5 * NPP_MAX) {
        e->h_large[i] = 0; changed = true; e->n_large--; e->n_demotions++;  // back below 5/8: demote
      }
    }
    // Dispatch order for the next launch: a launch ends with its slowest wavefront, and the hardware hands
    // workgroups to free slots in index order, so the envs that took longest in this launch (the kernel
    // reports each env's own duration, s_memtime ticks >> 10) go first in the next one -- longest
    // processing time first.  Counting sort over 256 duration buckets, stable; results do not depend on it.
    if (!e->use_order) {
      int kmax = 0;
      for (size_t i = 0; i < N; i++)
        if (e->h_launch_info[4 * i] >= 0) { const int k = e->h_launch_info[4 * i + 1] >> 16; if (k > kmax) kmax = k; }
      if (kmax > 0) {
        int count[258] = {0};
        auto bucket = [&](size_t i) {
          const int k = e->h_launch_info[4 * i] < 0 ? 0 : (e->h_launch_info[4 * i + 1] >> 16);
          return (int)((long long)k * 255 / kmax);
        };
        for (size_t i = 0; i < N; i++) count[255 - bucket(i) + 1]++;
        for (int k = 1; k <= 256; k++) count[k] += count[k - 1];
        for (size_t i = 0; i < N; i++) e->h_auto_order[count[255 - bucket(i)]++] = (int)i;
        // (the pinned staging buffer is rewritten only after the next launch's read-back sync)
        HIPCHK(hipMemcpyAsync(e->auto_order, e->h_auto_order, N * 4, hipMemcpyHostToDevice, e->stream));
        e->have_auto_order = true;
      } else {
        e->have_auto_order = false;
      }
    }
    if (nrerun > 0) {
      HIPCHK(hipMemcpyAsync(e->mask_r, e->h_rerun.data(), N, hipMemcpyHostToDevice, e->stream));
      mre_launch_restore_rows(e->mask_r, 0, e->N, e->qpos, e->sv_qpos, e->qvel, e->sv_qvel, e->qacc_ws, e->sv_qacc_ws,
                              e->qfine, e->sv_qfine, e->ctrl, e->sv_ctrl, e->nstep, e->sv_nstep, e->status,
                              e->sv_status, e->converged, e->sv_converged, nullptr, e->stream);
      StepArgs ar = a;
      ar.env_mask = e->mask_r; ar.launch_info = nullptr;
      launch_large(e, ar, e->stream);
      HIPCHK(hipGetLastError());
      e->n_reruns += nrerun;
    }
    if (changed) {
      // the staged copy must outlive the async upload: h_large is only touched after a stream sync
      HIPCHK(hipMemcpyAsync(e->d_large, e->h_large.data(), N, hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
  }
  if (e1) HIPCHK(hipEventRecord(e1, e->stream));
  return MRE_OK;
}

// ------------------------------------------------------------------- lifecycle
extern "C" const char* mre_last_error(void) { return g_err.c_str(); }

// allocation part of mre_create: on any failure the caller releases what exists via mre_destroy
static int create_buffers(mre_env* e, int num_envs, int device_id) {
  e->N = num_envs;
  e->device = device_id;
  HIPCHK(hipSetDevice(device_id));
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  const size_t N = (size_t)num_envs;
  HIPCHK(hipMalloc(&e->dM, sizeof(DevModel)));
  HIPCHK(hipMemcpy(e->dM, &e->hM, sizeof(DevModel), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&e->qpos, N * NQP * 4)); HIPCHK(hipMalloc(&e->qvel, N * NVP * 4));
  HIPCHK(hipMalloc(&e->qacc_ws, N * NVP * 4)); HIPCHK(hipMalloc(&e->ctrl, N * NU * 4));
  HIPCHK(hipMalloc(&e->qfine, N * QFINE_ROW * 4)); HIPCHK(hipMalloc(&e->sv_qfine, N * QFINE_ROW * 4));
  HIPCHK(hipMemsetAsync(e->qfine, 0, N * QFINE_ROW * 4, e->stream));
  HIPCHK(hipMalloc(&e->nstep, N * 4)); HIPCHK(hipMalloc(&e->sv_nstep, N * 4));
  HIPCHK(hipMemsetAsync(e->nstep, 0, N * 4, e->stream));
  HIPCHK(hipMalloc(&e->nprops, N * 4)); HIPCHK(hipMalloc(&e->prop_size, N * NPROP * 3 * 4));
  HIPCHK(hipMalloc(&e->osc_target, N * 16 * 4)); HIPCHK(hipMalloc(&e->grip_closed, N));
  HIPCHK(hipMalloc(&e->converged, N)); HIPCHK(hipMalloc(&e->mask, N));
  HIPCHK(hipMalloc(&e->sites, N * 16 * 4));
  HIPCHK(hipMalloc(&e->status, N * 4)); HIPCHK(hipMalloc(&e->stats, N * 4 * 4));
  HIPCHK(hipMalloc(&e->order, N * 4)); HIPCHK(hipMalloc(&e->auto_order, N * 4));
  HIPCHK(hipHostMalloc((void**)&e->h_auto_order, N * 4, hipHostMallocDefault));
  HIPCHK(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
  HIPCHK(hipMalloc(&e->d_large, N)); HIPCHK(hipMalloc(&e->mask_r, N));
  HIPCHK(hipMalloc(&e->sv_qpos, N * NQP * 4)); HIPCHK(hipMalloc(&e->sv_qvel, N * NVP * 4));
  HIPCHK(hipMalloc(&e->sv_qacc_ws, N * NVP * 4)); HIPCHK(hipMalloc(&e->sv_ctrl, N * NU * 4));
  HIPCHK(hipMalloc(&e->sv_status, N * 4));
  HIPCHK(hipMalloc(&e->sv_converged, N));
  HIPCHK(hipHostMalloc((void**)&e->h_launch_info, mre_env::RING * N * 16, hipHostMallocMapped | hipHostMallocCoherent));
  HIPCHK(hipHostGetDevicePointer((void**)&e->d_launch_info, e->h_launch_info, 0));
  memset(e->h_launch_info, 0xFF, mre_env::RING * N * 16);
  HIPCHK(hipHostMalloc((void**)&e->h_info_last, N * 16, hipHostMallocDefault));
  memset(e->h_info_last, 0xFF, N * 16);   // -1: no launch yet
  HIPCHK(hipHostMalloc((void**)&e->h_large_stage, mre_env::NSTAGE * N, hipHostMallocMapped | hipHostMallocCoherent));
  HIPCHK(hipHostGetDevicePointer((void**)&e->d_large_stage, e->h_large_stage, 0));
  memset(e->h_large_stage, 0, mre_env::NSTAGE * N);
  HIPCHK(hipMalloc(&e->d_pending, N));
  HIPCHK(hipMemsetAsync(e->d_pending, 0, N, e->stream));
  HIPCHK(hipMemsetAsync(e->d_large, 0, N, e->stream));
  e->h_large.assign(N, 0); e->h_rerun.assign(N, 0);
  {
    // env groups of the pipelined stepping path (MRE_GROUPS = 1: every call completes before it returns)
    int ng = 4, min_envs = 512;   // (measured on the bench: 2, 3 and 4 groups are within 1 % for Newton, 4 best for PGS)
    if (const char* g = getenv("MRE_GROUPS")) ng = atoi(g);
    if (const char* g = getenv("MRE_GROUP_MIN")) min_envs = atoi(g);   // test knob: smallest group worth a launch of its own
    if (ng < 1) ng = 1;
    if (ng > 8) ng = 8;
    if (const char* r = getenv("MRE_RING")) { e->ring = atoi(r); if (e->ring < 2) e->ring = 2; if (e->ring > mre_env::RING) e->ring = mre_env::RING; }
    while (ng > 1 && num_envs < min_envs * ng) ng--;
    HIPCHK(hipHostMalloc((void**)&e->h_grp_order, mre_env::NSTAGE * N * 4, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&e->d_grp_order, e->h_grp_order, 0));
    for (int k = 0; k < mre_env::NSTAGE; k++)
      for (int i = 0; i < num_envs; i++) e->h_grp_order[(size_t)k * N + i] = i;
    HIPCHK(hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming));
    e->groups.resize(ng);
    {
      // the queue's group: all envs, default stream priority
      auto& Q = e->qgroup;
      Q.lo = 0; Q.n = num_envs;
      HIPCHK(hipHostMalloc((void**)&e->h_qgrp_order, mre_env::NSTAGE * N * 4, hipHostMallocMapped | hipHostMallocCoherent));
      Q.h_order = e->h_qgrp_order;
      HIPCHK(hipHostGetDevicePointer((void**)&Q.d_order, Q.h_order, 0));
      for (int k = 0; k < mre_env::NSTAGE; k++)
        for (int i = 0; i < num_envs; i++) Q.h_order[(size_t)k * N + i] = i;
      {
        // the large kernel's waves on a stream of HIGHER priority: its own hardware queue (streams of one priority share a
        // few), and its few workgroups are placed before the compact kernel's 2048 fill the compute units' LDS
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&Q.st, hipStreamNonBlocking, least));
        HIPCHK(hipStreamCreateWithPriority(&Q.st2, hipStreamNonBlocking, greatest));
      }
      HIPCHK(hipEventCreateWithFlags(&Q.ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&Q.ev_join, hipEventDisableTiming));
      for (auto& o : Q.out) HIPCHK(hipEventCreateWithFlags(&o.ev_info, hipEventDisableTiming));
      if (const char* q = getenv("MRE_QUEUE")) e->queue_ok = atoi(q) != 0;
      if (const char* q = getenv("MRE_QUEUE_TICKS")) { const int v = atoi(q); if (v >= 2 && v <= QUEUE_TICKS_MAX) e->queue_ticks = v; }
      if (e->queue_run_ticks > e->queue_ticks) e->queue_run_ticks = e->queue_ticks;
      hipDeviceProp_t prop;
      HIPCHK(hipGetDeviceProperties(&prop, e->device));
      {
        const int a_ = mre_queue_waves_per_cu(), b_ = mre_queue_waves_per_cu_newton();
        e->queue_waves = prop.multiProcessorCount * (a_ < b_ ? a_ : b_);
      }
      if (const char* q = getenv("MRE_QUEUE_WAVES")) { const int v = atoi(q); if (v > 0) e->queue_waves = v; }   // test knob
      if (const char* q = getenv("MRE_QUEUE_SHARDS")) { const int v = atoi(q); if (v >= 1 && v <= QUEUE_SHARDS_MAX) e->queue_shards = v; }
      if (const char* q = getenv("MRE_QUEUE_MIN_TICKS")) { const int v = atoi(q); if (v >= 2) e->queue_min_ticks = v; }
      if (const char* q = getenv("MRE_QUEUE_TAIL_MIN")) { const float v = (float)atof(q); if (v > 0.f) e->queue_tail_min = v; }
      if (const char* q = getenv("MRE_QUEUE_TEST_SERIAL")) e->queue_test_serial = atoi(q) != 0;
      if (const char* q = getenv("MRE_QUEUE_SPARE_LARGE")) { const int v = atoi(q); if (v >= 0) e->queue_spare_large = v; }
      e->queue_large_waves_max = 2 * prop.multiProcessorCount;
      if (const char* q = getenv("MRE_QUEUE_LSHARDS")) { const int v = atoi(q); if (v >= 1 && v <= QUEUE_LSHARDS_MAX) e->queue_lshards = v; }
      HIPCHK(hipMalloc(&e->q_ws, ((2 * (size_t)(QUEUE_SHARDS_MAX + QUEUE_LSHARDS_MAX) * QUEUE_TICKS_MAX + 16 + 4 * N +
                                   (size_t)QUEUE_TICKS_MAX * (2 * N + QUEUE_SHARDS_MAX + QUEUE_LSHARDS_MAX)) * 4 + 15) / 16 * 16));
      HIPCHK(hipMalloc(&e->q_gen, 64));
      HIPCHK(hipMemsetAsync(e->q_gen, 0, 64, e->stream));
      HIPCHK(hipHostMalloc((void**)&e->h_qlist, (size_t)(mre_env::RING + 1) * (N + 32) * 4, hipHostMallocDefault));
      HIPCHK(hipHostMalloc((void**)&e->h_q_err, 64, hipHostMallocMapped | hipHostMallocCoherent));
      *e->h_q_err = 0;
    }
    for (int g = 0; g < ng; g++) {
      auto& G = e->groups[g];
      G.h_order = e->h_grp_order; G.d_order = e->d_grp_order;
      G.lo = (int)((long long)num_envs * g / ng);
      G.n = (int)((long long)num_envs * (g + 1) / ng) - G.lo;
      // descending stream priorities stagger the groups: the first group's workgroups are dispatched first and the
      // later groups fill the slots its slow envs leave idle (MRE_GROUP_PRIORITY=0: equal priorities)
      int pr = 0;
      {
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const char* gp = getenv("MRE_GROUP_PRIORITY");
        if (!(gp && atoi(gp) == 0)) { pr = greatest + g; if (pr > least) pr = least; }
        // tuning knob: one digit per group, 0 = highest priority level
        if (const char* map = getenv("MRE_GROUP_PRIO_MAP")) {
          if ((int)strlen(map) > g && map[g] >= '0' && map[g] <= '9') { pr = greatest + (map[g] - '0'); if (pr > least) pr = least; }
        }
      }
      HIPCHK(hipStreamCreateWithPriority(&G.st, hipStreamNonBlocking, pr));
      HIPCHK(hipStreamCreateWithPriority(&G.st2, hipStreamNonBlocking, pr));
      HIPCHK(hipEventCreateWithFlags(&G.ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&G.ev_join, hipEventDisableTiming));
      for (auto& o : G.out) HIPCHK(hipEventCreateWithFlags(&o.ev_info, hipEventDisableTiming));
    }
  }
  if (const char* fb = getenv("MRE_NO_FALLBACK")) e->fallback = atoi(fb) == 0;  // profiling knob only
  if (const char* fl = getenv("MRE_FORCE_LARGE")) {  // profiling knob only: start every env on the large kernel
    if (atoi(fl) != 0) {
      e->h_large.assign(N, 1); e->n_large = num_envs;
      HIPCHK(hipMemsetAsync(e->d_large, 1, N, e->stream));
    }
  }
  HIPCHK(hipMemsetAsync(e->status, 0, N * 4, e->stream)); HIPCHK(hipMemsetAsync(e->stats, 0, N * 16, e->stream));
  HIPCHK(hipMemsetAsync(e->grip_closed, 0, N, e->stream)); HIPCHK(hipMemsetAsync(e->osc_target, 0, N * 64, e->stream));
  HIPCHK(hipMemsetAsync(e->sites, 0, N * 64, e->stream));
  // defaults: 4 cubes of half size 0.0155
  std::vector<int> np(N, NPROP);
  std::vector<float> ps(N * NPROP * 3, 0.0155f);
  HIPCHK(hipMemcpy(e->nprops, np.data(), N * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->prop_size, ps.data(), ps.size() * 4, hipMemcpyHostToDevice));
  // OSC defaults (osc.yaml:5-22)
  e->osc = OscConfig{350.f, 20.f, 500.f, 100.f, 200.f, 30.f, {0.f, -0.785f, 0.f, -2.356f, 0.f, 1.571f, 0.785f},
                     5e-3f, 68e-3f, 0};
  HIPCHK(hipMalloc(&e->d_osc, sizeof(OscConfig)));
  HIPCHK(hipMemcpy(e->d_osc, &e->osc, sizeof(OscConfig), hipMemcpyHostToDevice));
  // (device memsets above are enqueued on the handle's stream: a hipMemset on the null stream is
  // asynchronous and is NOT ordered against a non-blocking stream)
  HIPCHK(hipStreamSynchronize(e->stream));
  int rc = mre_reset(e, nullptr);
  if (rc != MRE_OK) return rc;
  return mre_sync(e);
}

extern "C" int mre_create(const void* blob, size_t nbytes, int num_envs, int device_id, mre_env** out) {
  if (!blob || !out || num_envs <= 0) return fail(MRE_ERR_ARG, "mre_create: bad argument");
  *out = nullptr;
  mre_env* e = new mre_env();
  const std::string err = build_model(blob, nbytes, e->hM, e->solver);
  if (!err.empty()) { delete e; return fail(MRE_ERR_MODEL, err); }
  if (const char* it = getenv("MRE_DEBUG_ITERS")) e->hM.opt_rec.iterations = atoi(it);  // profiling knob only
  int rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    delete e;
    return fail(MRE_ERR_NOGPU, "mre_create: no HIP device visible (the HIP path has no CPU fallback)");
  }
  if (device_id < 0 || device_id >= ndev) {
    delete e;
    return fail(MRE_ERR_ARG, "mre_create: device_id out of range");
  }
  rc = create_buffers(e, num_envs, device_id);
  if (rc != MRE_OK) {
    const std::string msg = g_err;  // mre_destroy must not clobber the reason
    mre_destroy(e);
    g_err = msg;
    return rc;
  }
  *out = e;
  return MRE_OK;
}

extern "C" int mre_destroy(mre_env* e) {
  if (!e) return MRE_OK;
  (void)hipSetDevice(e->device);
  (void)drain(e);
  if (getenv("MRE_DEBUG_TIMING") && e->dbg_calls > 0)
    fprintf(stderr, "mre: %ld pipelined calls, %.1f us per call in the library, of which %.1f us waiting for launch info\n",
            e->dbg_calls, 1e6 * e->dbg_call_s / e->dbg_calls, 1e6 * e->dbg_wait_s / e->dbg_calls);
  auto free_group = [](mre_env::Group& G) {
    if (G.st) { (void)hipStreamSynchronize(G.st); (void)hipStreamDestroy(G.st); }
    if (G.st2) { (void)hipStreamSynchronize(G.st2); (void)hipStreamDestroy(G.st2); }
    if (G.ev_fork) (void)hipEventDestroy(G.ev_fork);
    if (G.ev_join) (void)hipEventDestroy(G.ev_join);
    for (auto& O : G.out) if (O.ev_info) (void)hipEventDestroy(O.ev_info);
  };
  for (auto& G : e->groups) free_group(G);
  free_group(e->qgroup);
  if (e->q_ws) (void)hipFree(e->q_ws);
  if (e->q_gen) (void)hipFree(e->q_gen);
  if (e->h_q_err) (void)hipHostFree(e->h_q_err);
  if (e->h_qlist) (void)hipHostFree(e->h_qlist);
  if (e->h_qgrp_order) (void)hipHostFree(e->h_qgrp_order);
  if (e->ev_main) (void)hipEventDestroy(e->ev_main);
  if (e->h_grp_order) (void)hipHostFree(e->h_grp_order);
  for (float* p : e->seq_copy) if (p) (void)hipFree(p);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->stream2) (void)hipStreamSynchronize(e->stream2);
  void* ptrs[] = {e->dM, e->qpos, e->qvel, e->qacc_ws, e->ctrl, e->nprops, e->prop_size, e->osc_target,
                  e->grip_closed, e->converged, e->mask, e->sites, e->status, e->stats, e->d_osc, e->d_osc_env, e->order,
                  e->geoms, e->prop_rgb, e->bg_depth, e->bg_rgb, e->bg_seg,
                  e->d_large, e->mask_r, e->qfine, e->sv_qfine, e->nstep, e->sv_nstep, e->sv_qpos, e->sv_qvel, e->sv_qacc_ws, e->sv_ctrl,
                  e->sv_status, e->auto_order, e->sv_converged, e->contacts, e->contacts_full, e->settle_steps,
                  e->d_env_ids, e->ps_attempts, e->ps_prop, e->ps_tick, e->ps_which, e->ps_bounds, e->ps_pose, e->ps_zones,
                  e->ps_pick};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (e->h_launch_info) (void)hipHostFree(e->h_launch_info);
  if (e->h_info_last) (void)hipHostFree(e->h_info_last);
  if (e->h_large_stage) (void)hipHostFree(e->h_large_stage);
  if (e->d_pending) (void)hipFree(e->d_pending);
  if (e->h_auto_order) (void)hipHostFree(e->h_auto_order);
  for (auto& pr : e->events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  if (e->ev_order) (void)hipEventDestroy(e->ev_order);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->stream2) (void)hipStreamDestroy(e->stream2);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return MRE_OK;
}

extern "C" int mre_num_envs(const mre_env* e) { return e ? e->N : 0; }
extern "C" void* mre_stream(mre_env* e) { return e ? (void*)e->stream : nullptr; }
extern "C" int mre_sync(mre_env* e) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  HIPCHK(hipSetDevice(e->device));
  DRAIN(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  return MRE_OK;
}

static int copy_in(mre_env* e, void* dst, const void* src, size_t n) {
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, e->stream));
  return MRE_OK;
}
static int copy_out(mre_env* e, void* dst, const void* src, size_t n) {
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MRE_OK;
}
// returns device mask pointer or nullptr
static int stage_mask(mre_env* e, const uint8_t* mask, const uint8_t** dmask) {
  *dmask = nullptr;
  if (!mask) return MRE_OK;
  int rc = copy_in(e, e->mask, mask, (size_t)e->N);
  *dmask = e->mask;
  return rc;
}

extern "C" int mre_set_props(mre_env* e, const int32_t* nprops, const float* prop_half_size) {
  if (!e || !nprops || !prop_half_size) return fail(MRE_ERR_ARG, "mre_set_props: null");
  DRAIN(e);
  int rc = copy_in(e, e->nprops, nprops, (size_t)e->N * 4);
  if (rc) return rc;
  return copy_in(e, e->prop_size, prop_half_size, (size_t)e->N * NPROP * 3 * 4);
}

extern "C" int mre_reset(mre_env* e, const uint8_t* mask) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  const uint8_t* dmask;
  int rc = stage_mask(e, mask, &dmask);
  if (rc) return rc;
  mre_launch_reset(e->dM, e->N, e->qpos, e->qvel, e->qacc_ws, e->qfine, e->ctrl, e->status, e->nstep, dmask, e->stream);
  HIPCHK(hipGetLastError());
  if (!mask) e->tick_tail_valid = false;   // (a new episode: what the per-tick launches measured no longer describes it)
  // a reset env starts on the compact kernel again (the mask may be a device pointer: read a host copy)
  bool changed = false;
  std::vector<uint8_t> hmask;
  if (mask) {
    hmask.resize((size_t)e->N);
    rc = copy_out(e, hmask.data(), dmask, (size_t)e->N);
    if (rc) return rc;
  }
  for (int i = 0; i < e->N; i++)
    if (!e->large_only && e->h_large[i] && (!mask || hmask[i])) { e->h_large[i] = 0; e->n_large--; changed = true; }
  if (changed) {
    HIPCHK(hipMemcpyAsync(e->d_large, e->h_large.data(), (size_t)e->N, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return MRE_OK;
}

// ---- batched overhead camera (csrc/mre_render.hip)
static void fill_args(mre_env* e, StepArgs& a);
static bool is_device_ptr(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice;
}

extern "C" int mre_set_render_colours(mre_env* e, const uint8_t* prop_rgb, const float* geom_rgb) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  const size_t N = (size_t)e->N;
  if (!e->prop_rgb) {
    HIPCHK(hipMalloc(&e->prop_rgb, N * NPROP * 3));
    HIPCHK(hipMemsetAsync(e->prop_rgb, 128, N * NPROP * 3, e->stream));
    for (int g = 0; g < NG; g++) for (int k = 0; k < 3; k++) e->geom_rgb[g][k] = 0.5f;
  }
  if (prop_rgb) { int rc = copy_in(e, e->prop_rgb, prop_rgb, N * NPROP * 3); if (rc) return rc; }
  if (geom_rgb) { memcpy(e->geom_rgb, geom_rgb, sizeof(e->geom_rgb)); e->bg_valid = false; }
  HIPCHK(hipStreamSynchronize(e->stream));
  return MRE_OK;
}

extern "C" int mre_render(mre_env* e, const float* cam_pos, const float* cam_mat, float fovy_deg, int height, int width,
                          uint8_t* rgb, float* depth, uint8_t* seg, const uint8_t* mask) {
  if (!e || !cam_pos || !cam_mat) return fail(MRE_ERR_ARG, "mre_render: null argument");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  if (height <= 0 || width <= 0 || (width & 3) != 0 || width / 4 > 320 || !(fovy_deg > 0.f && fovy_deg < 180.f))
    return fail(MRE_ERR_ARG, "mre_render: width must be a multiple of 4 (<= 1280), 0 < fovy < 180");
  if ((rgb && !is_device_ptr(rgb)) || (depth && !is_device_ptr(depth)) || (seg && !is_device_ptr(seg)))
    return fail(MRE_ERR_ARG, "mre_render: image buffers must be device pointers");
  if (depth && ((uintptr_t)depth & 15)) return fail(MRE_ERR_ARG, "mre_render: depth must be 16-byte aligned");
  if ((rgb && ((uintptr_t)rgb & 3)) || (seg && ((uintptr_t)seg & 3)))
    return fail(MRE_ERR_ARG, "mre_render: rgb / seg must be 4-byte aligned");
  int rc = MRE_OK;
  if (!e->prop_rgb) { rc = mre_set_render_colours(e, nullptr, nullptr); if (rc) return rc; }
  const size_t N = (size_t)e->N;
  if (!e->geoms) HIPCHK(hipMalloc(&e->geoms, N * NG * 16 * 4));
  const uint8_t* dmask;
  rc = stage_mask(e, mask, &dmask);
  if (rc) return rc;
  // geometry of the current state: a zero-step launch of the step kernel (kinematics + export)
  StepArgs a;
  fill_args(e, a);
  a.nsteps = 0; a.trace = nullptr; a.env_order = nullptr; a.env_mask = dmask; a.geoms = e->geoms;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (e->profiling) {  // same event bracket as launch_step: tools/bench_render.py times the camera with it
    if (e->events_used == e->events.size()) {
      hipEvent_t x, y;
      HIPCHK(hipEventCreate(&x)); HIPCHK(hipEventCreate(&y));
      e->events.emplace_back(x, y);
    }
    e0 = e->events[e->events_used].first; e1 = e->events[e->events_used].second;
    e->events_used++;
    HIPCHK(hipEventRecord(e0, e->stream));
  }
  launch_compact(e, a, e->stream);
  HIPCHK(hipGetLastError());
  RenderArgs r;
  memset(&r, 0, sizeof(r));
  r.N = e->N; r.height = height; r.width = width;
  r.geoms = e->geoms; r.nprops = e->nprops; r.prop_rgb = e->prop_rgb;
  memcpy(r.geom_rgb, e->geom_rgb, sizeof(r.geom_rgb));
  for (int k = 0; k < 3; k++) r.cam_pos[k] = cam_pos[k];
  for (int k = 0; k < 9; k++) r.cam_mat[k] = cam_mat[k];
  r.fy = 0.5f * (float)height / tanf(0.5f * fovy_deg * 3.14159265358979323846f / 180.f);
  // arena.xml:18 (positional light) and MuJoCo's default headlight (ambient 0.1, diffuse 0.4)
  r.light_pos[0] = 0.7f; r.light_pos[1] = 0.f; r.light_pos[2] = 1.6f;
  r.ambient = 0.1f; r.head_diffuse = 0.4f; r.light_diffuse = 0.7f;
  // arena.xml:5-6: checker .2 .3 .4 / .1 .2 .3, texrepeat 5 per metre of a 2 x 2 checker
  const float c0[3] = {0.2f, 0.3f, 0.4f}, c1[3] = {0.1f, 0.2f, 0.3f};
  for (int k = 0; k < 3; k++) { r.checker[0][k] = c0[k]; r.checker[1][k] = c1[k]; }
  r.checker_size = 0.1f;
  r.zfar = 100.f;
  r.rgb = rgb; r.depth = depth; r.seg = seg; r.env_mask = dmask;
  const int rows_per_iter = 320 / (width / 4);
  int row_groups = (height + rows_per_iter - 1) / rows_per_iter;
  int cap = 8;  // 8 row groups per env: the per-workgroup geom set-up is amortised over 30 row pairs
  if (const char* rg = getenv("MRE_RENDER_ROW_GROUPS")) cap = atoi(rg);  // tuning knob
  if (cap < 1) cap = 1;
  if (row_groups > cap) row_groups = cap;
  // The static geoms (ground plane, table: geoms 0 and 1, fixed to the world) look the same in every
  // env and every frame of a camera: their image is rendered once per camera and every frame then
  // starts from it and composites the moving geoms (robot hulls, cubes) on top.
  constexpr int N_STATIC = 2;
  bool use_bg = true;
  if (const char* nb = getenv("MRE_RENDER_NO_BACKGROUND")) use_bg = atoi(nb) == 0;  // diagnostic
  if (use_bg) {
    float key[16] = {cam_pos[0], cam_pos[1], cam_pos[2], cam_mat[0], cam_mat[1], cam_mat[2], cam_mat[3], cam_mat[4],
                     cam_mat[5], cam_mat[6], cam_mat[7], cam_mat[8], fovy_deg, 0.f, 0.f, 0.f};
    if (!e->bg_valid || e->bg_h != height || e->bg_w != width || memcmp(key, e->bg_key, sizeof(key)) != 0) {
      if (e->bg_h != height || e->bg_w != width) {
        for (void* p : {(void*)e->bg_depth, (void*)e->bg_rgb, (void*)e->bg_seg}) if (p) (void)hipFree(p);
        e->bg_depth = nullptr; e->bg_rgb = nullptr; e->bg_seg = nullptr;
        const size_t px = (size_t)height * width;
        HIPCHK(hipMalloc(&e->bg_depth, px * 4)); HIPCHK(hipMalloc(&e->bg_rgb, px * 3)); HIPCHK(hipMalloc(&e->bg_seg, px));
        e->bg_h = height; e->bg_w = width;
      }
      // the static geoms' poses do not depend on the env: cast them for env 0 (exported above even
      // when env 0 is masked out? no -- so export it unmasked once)
      if (dmask) {
        StepArgs a0 = a;
        a0.env_mask = nullptr;
        launch_compact(e, a0, e->stream);
        HIPCHK(hipGetLastError());
      }
      RenderArgs b = r;
      b.N = 1; b.env_mask = nullptr; b.g0 = 0; b.g1 = N_STATIC;
      b.rgb = e->bg_rgb; b.depth = e->bg_depth; b.seg = e->bg_seg;
      mre_launch_render(&b, row_groups, e->stream);
      HIPCHK(hipGetLastError());
      memcpy(e->bg_key, key, sizeof(key));
      e->bg_valid = true;
    }
    r.g0 = N_STATIC; r.g1 = NG;
    r.bg_depth = e->bg_depth; r.bg_rgb = e->bg_rgb; r.bg_seg = e->bg_seg;
  } else {
    r.g0 = 0; r.g1 = NG;
  }
  mre_launch_render(&r, row_groups, e->stream);
  HIPCHK(hipGetLastError());
  if (e1) HIPCHK(hipEventRecord(e1, e->stream));
  return MRE_OK;
}

extern "C" int mre_set_fallback(mre_env* e, int mode) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  if (mode < 0 || mode > 2) return fail(MRE_ERR_ARG, "mre_set_fallback: mode is 0 (compact only), 1 (fallback) or 2 (large only)");
  e->fallback = mode != 0;
  e->large_only = mode == 2;
  e->compact_only = mode == 0;
  HIPCHK(hipStreamSynchronize(e->stream));
  if (mode != 1) {
    e->h_large.assign((size_t)e->N, mode == 2 ? 1 : 0);
    HIPCHK(hipMemcpy(e->d_large, e->h_large.data(), (size_t)e->N, hipMemcpyHostToDevice));
  }
  return MRE_OK;
}

// CRC-32C (Castagnoli) of a host buffer: the checksum of TFRecord framing (dataset.py writes the
// reference's RLDS episodes, transporter_network_data_generation.py:56-111); slicing-by-8 tables
namespace {
struct Crc32cTables {   // built once, by the C++ runtime's thread-safe initialisation of the function-local static
  uint32_t T[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
      T[0][i] = c;
    }
    for (int k = 1; k < 8; k++)
      for (uint32_t i = 0; i < 256; i++) T[k][i] = (T[k - 1][i] >> 8) ^ T[0][T[k - 1][i] & 0xFFu];
  }
};
}  // namespace
extern "C" uint32_t mre_crc32c(const void* data, size_t n) {
  static const Crc32cTables tables;
  const uint32_t (*T)[256] = tables.T;
  const unsigned char* p = (const unsigned char*)data;
  uint32_t crc = 0xFFFFFFFFu;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
    lo ^= crc;
    crc = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^ T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^
          T[3][hi & 0xFF] ^ T[2][(hi >> 8) & 0xFF] ^ T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
    p += 8; n -= 8;
  }
  while (n--) crc = T[0][(crc ^ *p++) & 0xFFu] ^ (crc >> 8);
  return crc ^ 0xFFFFFFFFu;
}

// ---- episode records on the device (csrc/mre_records.hip): packed varints and CRC-32C of byte rows
extern "C" uint32_t mre_crc32c_combine(uint32_t crc_a, uint32_t crc_b, size_t len_b) {
  return mre_rec_crc32c_combine(crc_a, crc_b, len_b);
}

static size_t rec_segments(size_t row_bytes) { return (row_bytes + REC_PACK_SEG - 1) / REC_PACK_SEG; }

extern "C" size_t mre_records_workspace_bytes(int rows, size_t row_bytes) {
  if (rows <= 0 || row_bytes == 0 || row_bytes > REC_MAX_ROW_BYTES) return 0;
  return 2 * (size_t)rows * rec_segments(row_bytes) * sizeof(uint32_t);   // segment offsets + segment CRCs
}

// the checks the two calls share; fills the row interface of RecArgs (nseg for `seg` bytes per segment)
static int rec_args(const char* who, RecArgs& a, const uint8_t* src, size_t row_stride, size_t row_bytes,
                    const int32_t* rows_idx, int src_rows, int rows, void* workspace, size_t workspace_bytes, size_t seg) {
  const std::string w(who);
  if (!src || rows <= 0 || src_rows <= 0 || row_bytes == 0 || !workspace)
    return fail(MRE_ERR_ARG, w + ": null argument or empty row set");
  if (row_bytes > REC_MAX_ROW_BYTES) return fail(MRE_ERR_ARG, w + ": row_bytes above 2^30");
  if (row_stride < row_bytes && src_rows > 1) return fail(MRE_ERR_ARG, w + ": row_stride below row_bytes");
  if (!rows_idx && rows > src_rows) return fail(MRE_ERR_ARG, w + ": more rows than the source holds and no index list");
  const size_t nseg = (row_bytes + seg - 1) / seg;
  if ((size_t)rows * nseg > 0x7FFFFFFFull) return fail(MRE_ERR_ARG, w + ": rows x segments above 2^31 - 1");
  if (workspace_bytes < mre_records_workspace_bytes(rows, row_bytes) || ((uintptr_t)workspace & 3))
    return fail(MRE_ERR_ARG, w + ": workspace smaller than mre_records_workspace_bytes() or not 4-byte aligned");
  if (!is_device_ptr(src) || !is_device_ptr(workspace) || (rows_idx && !is_device_ptr(rows_idx)))
    return fail(MRE_ERR_ARG, w + ": src, rows_idx and workspace must be device pointers");
  memset(&a, 0, sizeof(a));
  a.src = src; a.stride = row_stride; a.row_bytes = (uint32_t)row_bytes; a.idx = rows_idx;
  a.src_rows = (uint32_t)src_rows; a.rows = (uint32_t)rows; a.nseg = (uint32_t)nseg;
  a.segoff = (uint32_t*)workspace;
  a.segcrc = a.segoff + (size_t)rows * rec_segments(row_bytes);
  return MRE_OK;
}

extern "C" int mre_varint_pack_rows(void* stream, const uint8_t* src, size_t row_stride, size_t row_bytes,
                                    const int32_t* rows_idx, int src_rows, int rows, uint8_t* out, size_t out_capacity,
                                    int64_t* off, uint32_t* len, uint32_t* crc, void* workspace, size_t workspace_bytes) {
  RecArgs a;
  int rc = rec_args("mre_varint_pack_rows", a, src, row_stride, row_bytes, rows_idx, src_rows, rows, workspace,
                    workspace_bytes, REC_PACK_SEG);
  if (rc) return rc;
  if (!off || !len || !is_device_ptr(off) || !is_device_ptr(len) || ((uintptr_t)off & 7) || ((uintptr_t)len & 3))
    return fail(MRE_ERR_ARG, "mre_varint_pack_rows: off / len must be aligned device pointers");
  if (out) {
    // the worst case, not the actual length: the length is only known on the device, and nothing may be written
    // beyond the caller's buffer whatever the rows hold
    if (out_capacity / 2 / (size_t)rows < row_bytes)
      return fail(MRE_ERR_ARG, "mre_varint_pack_rows: out_capacity below the worst case 2 * rows * row_bytes");
    if (!crc || !is_device_ptr(out) || !is_device_ptr(crc) || ((uintptr_t)crc & 3))
      return fail(MRE_ERR_ARG, "mre_varint_pack_rows: out / crc must be device pointers (crc 4-byte aligned)");
  }
  a.out = out; a.off = (long long*)off; a.len = len; a.crc = crc;
  mre_launch_varint_size(&a, (hipStream_t)stream);
  if (out) mre_launch_varint_pack(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

extern "C" int mre_crc32c_rows(void* stream, const uint8_t* src, size_t row_stride, size_t row_bytes,
                               const int32_t* rows_idx, int src_rows, int rows, uint32_t* crc, void* workspace,
                               size_t workspace_bytes) {
  RecArgs a;
  int rc = rec_args("mre_crc32c_rows", a, src, row_stride, row_bytes, rows_idx, src_rows, rows, workspace,
                    workspace_bytes, REC_CRC_SEG);
  if (rc) return rc;
  if (!crc || !is_device_ptr(crc) || ((uintptr_t)crc & 3))
    return fail(MRE_ERR_ARG, "mre_crc32c_rows: crc must be a 4-byte aligned device pointer");
  a.crc = crc;
  mre_launch_crc32c_rows(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

static size_t unpack_segments(size_t max_src_len) { return (max_src_len + REC_UNPACK_SEG - 1) / REC_UNPACK_SEG; }

extern "C" size_t mre_varint_unpack_workspace_bytes(int rows, size_t max_src_len) {
  if (rows <= 0 || max_src_len == 0 || max_src_len > REC_MAX_PACKED_BYTES) return 0;
  return (size_t)rows * unpack_segments(max_src_len) * sizeof(uint32_t);   // start bytes per segment, then their scan
}

extern "C" int mre_varint_unpack_rows(void* stream, const uint8_t* src, size_t src_bytes, const int64_t* src_off,
                                      const int64_t* src_len, const int64_t* nvalues, const int64_t* out_off, int rows,
                                      size_t max_src_len, uint8_t* out, size_t out_capacity, uint32_t* status,
                                      void* workspace, size_t workspace_bytes) {
  const std::string w("mre_varint_unpack_rows");
  if (!src || !src_off || !src_len || !nvalues || !out_off || !out || !status || !workspace || rows <= 0 ||
      src_bytes == 0 || out_capacity == 0)
    return fail(MRE_ERR_ARG, w + ": null argument, empty buffer or empty row set");
  if (max_src_len == 0 || max_src_len > REC_MAX_PACKED_BYTES) return fail(MRE_ERR_ARG, w + ": max_src_len outside 1 .. 2^31");
  const size_t nseg = unpack_segments(max_src_len);
  if ((size_t)rows * nseg > 0x7FFFFFFFull) return fail(MRE_ERR_ARG, w + ": rows x segments above 2^31 - 1");
  if (workspace_bytes < mre_varint_unpack_workspace_bytes(rows, max_src_len) || ((uintptr_t)workspace & 3))
    return fail(MRE_ERR_ARG, w + ": workspace smaller than mre_varint_unpack_workspace_bytes() or not 4-byte aligned");
  if ((((uintptr_t)src_off | (uintptr_t)src_len | (uintptr_t)nvalues | (uintptr_t)out_off) & 7) || ((uintptr_t)status & 3))
    return fail(MRE_ERR_ARG, w + ": descriptors must be 8-byte aligned, status 4-byte aligned");
  if (!is_device_ptr(src) || !is_device_ptr(src_off) || !is_device_ptr(src_len) || !is_device_ptr(nvalues) ||
      !is_device_ptr(out_off) || !is_device_ptr(out) || !is_device_ptr(status) || !is_device_ptr(workspace))
    return fail(MRE_ERR_ARG, w + ": src, the descriptors, out, status and workspace must be device pointers");
  UnpackArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.src_bytes = src_bytes;
  a.src_off = (const long long*)src_off; a.src_len = (const long long*)src_len;
  a.nvalues = (const long long*)nvalues; a.out_off = (const long long*)out_off;
  a.max_src_len = max_src_len; a.rows = (uint32_t)rows; a.nseg = (uint32_t)nseg;
  a.out = out; a.out_capacity = out_capacity; a.status = status; a.segoff = (uint32_t*)workspace;
  mre_launch_varint_unpack(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

extern "C" int mre_wait_stream(mre_env* e, void* stream) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  HIPCHK(hipSetDevice(e->device));
  if (!e->ev_order) HIPCHK(hipEventCreateWithFlags(&e->ev_order, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e->ev_order, (hipStream_t)stream));
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_order, 0));
  return MRE_OK;
}

extern "C" int mre_set_solver(mre_env* e, int solver) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  if (solver != MRE_SOLVER_PGS && solver != MRE_SOLVER_NEWTON)
    return fail(MRE_ERR_ARG, "mre_set_solver: solver is 0 (PGS) or 2 (Newton)");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->solver = solver;   // host-side only: it picks the kernel instantiation, no kernel reads it
  return MRE_OK;
}

extern "C" int mre_get_solver(mre_env* e) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  return e->solver;
}

// {queue launches so far, waves of a queue launch, control ticks per queue launch (the library's choice), enabled,
//  envs handed over to the large kernel inside a queue launch so far}
extern "C" int mre_get_queue_info(mre_env* e, long long* out5) {
  if (!e || !out5) return fail(MRE_ERR_ARG, "mre_get_queue_info: null");
  DRAIN(e);
  out5[0] = e->n_queue_launches; out5[1] = e->queue_waves; out5[2] = e->queue_ticks; out5[3] = e->queue_ok ? 1 : 0;
  out5[4] = e->n_handovers;
  return MRE_OK;
}

extern "C" int mre_get_fallback_stats(mre_env* e, long long* out4) {
  if (!e || !out4) return fail(MRE_ERR_ARG, "mre_get_fallback_stats: null");
  DRAIN(e);
  out4[0] = e->n_large; out4[1] = e->n_reruns; out4[2] = e->n_promotions; out4[3] = e->n_demotions;
  return MRE_OK;
}

extern "C" int mre_set_state(mre_env* e, const float* qpos, const float* qvel) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  int rc = MRE_OK;
  if (qpos) rc = copy_in(e, e->qpos, qpos, (size_t)e->N * NQP * 4);
  if (!rc && qvel) rc = copy_in(e, e->qvel, qvel, (size_t)e->N * NVP * 4);
  // a float32 row IS the value: the low-order words of the robot's angles / velocities start from zero
  // the float32 rows ARE the state now: the low-order words of what was overwritten go to zero (robot joints, cube poses /
  // robot and cube velocities)
  if (!rc && qpos) {
    HIPCHK(hipMemset2DAsync(e->qfine, QFINE_ROW * 4, 0, QFINE * 2, (size_t)e->N, e->stream));
    HIPCHK(hipMemset2DAsync(e->qfine + QFINE_CUBE_Q, QFINE_ROW * 4, 0, (QFINE_CUBE_V - QFINE_CUBE_Q) * 4, (size_t)e->N, e->stream));
  }
  if (!rc && qvel) {
    HIPCHK(hipMemset2DAsync(e->qfine + QFINE / 2, QFINE_ROW * 4, 0, QFINE * 2, (size_t)e->N, e->stream));
    HIPCHK(hipMemset2DAsync(e->qfine + QFINE_CUBE_V, QFINE_ROW * 4, 0, (QFINE_ROW - QFINE_CUBE_V) * 4, (size_t)e->N, e->stream));
  }
  return rc;
}

// physics.data.qpos / .qvel as the reference holds them (float64): the robot's 15 joints are carried as
// double-float pairs on the device (StepArgs::qfine), the cubes' coordinates as float32.  Host pointers.
extern "C" int mre_get_state_f64(mre_env* e, double* qpos, double* qvel) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  const size_t N = (size_t)e->N;
  std::vector<float> hq(N * NQP), hv(N * NVP), hf(N * QFINE_ROW);
  int rc = copy_out(e, hq.data(), e->qpos, N * NQP * 4);
  if (!rc) rc = copy_out(e, hv.data(), e->qvel, N * NVP * 4);
  if (!rc) rc = copy_out(e, hf.data(), e->qfine, N * QFINE_ROW * 4);
  if (rc) return rc;
  for (size_t i = 0; i < N; i++) {
    if (qpos) for (int k = 0; k < NQ; k++)
      qpos[i * NQ + k] = (double)hq[i * NQP + k] + (double)hf[i * QFINE_ROW + (k < NRV ? k : QFINE_CUBE_Q + (k - NRV))];
    if (qvel) for (int k = 0; k < NV; k++)
      qvel[i * NV + k] = (double)hv[i * NVP + k] + (double)hf[i * QFINE_ROW + (k < NRV ? QFINE / 2 + k : QFINE_CUBE_V + (k - NRV))];
  }
  return MRE_OK;
}
extern "C" int mre_set_state_f64(mre_env* e, const double* qpos, const double* qvel) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  const size_t N = (size_t)e->N;
  std::vector<float> hq(N * NQP), hv(N * NVP), hf(N * QFINE_ROW);
  int rc = copy_out(e, hq.data(), e->qpos, N * NQP * 4);
  if (!rc) rc = copy_out(e, hv.data(), e->qvel, N * NVP * 4);
  if (!rc) rc = copy_out(e, hf.data(), e->qfine, N * QFINE_ROW * 4);
  if (rc) return rc;
  for (size_t i = 0; i < N; i++) {
    if (qpos) for (int k = 0; k < NQ; k++) {
      const float hi = (float)qpos[i * NQ + k];
      hq[i * NQP + k] = hi;
      hf[i * QFINE_ROW + (k < NRV ? k : QFINE_CUBE_Q + (k - NRV))] = (float)(qpos[i * NQ + k] - (double)hi);
    }
    if (qvel) for (int k = 0; k < NV; k++) {
      const float hi = (float)qvel[i * NV + k];
      hv[i * NVP + k] = hi;
      hf[i * QFINE_ROW + (k < NRV ? QFINE / 2 + k : QFINE_CUBE_V + (k - NRV))] = (float)(qvel[i * NV + k] - (double)hi);
    }
  }
  rc = copy_in(e, e->qpos, hq.data(), N * NQP * 4);
  if (!rc) rc = copy_in(e, e->qvel, hv.data(), N * NVP * 4);
  if (!rc) rc = copy_in(e, e->qfine, hf.data(), N * QFINE_ROW * 4);
  if (!rc) HIPCHK(hipStreamSynchronize(e->stream));   // (the staged rows must outlive the uploads)
  return rc;
}
// physics.data.time (models/robot_arm.py:68-69): physics steps since the last mre_reset times the timestep, per env
// (envs differ after PropPlacer's settle, whose exit is per env).  Host pointer [N].
extern "C" int mre_get_time(mre_env* e, double* time) {
  if (!e || !time) return fail(MRE_ERR_ARG, "mre_get_time: null");
  DRAIN(e);
  std::vector<int> hn((size_t)e->N);
  int rc = copy_out(e, hn.data(), e->nstep, (size_t)e->N * 4);
  if (rc) return rc;
  for (int i = 0; i < e->N; i++) time[i] = (double)hn[i] * (double)e->hM.opt_rec.timestep;
  return MRE_OK;
}
extern "C" int mre_get_ctrl(mre_env* e, float* ctrl) {
  if (!e || !ctrl) return fail(MRE_ERR_ARG, "mre_get_ctrl: null");
  DRAIN(e);
  return copy_out(e, ctrl, e->ctrl, (size_t)e->N * NU * 4);
}

extern "C" int mre_get_state(mre_env* e, float* qpos, float* qvel) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  int rc = MRE_OK;
  if (qpos) rc = copy_out(e, qpos, e->qpos, (size_t)e->N * NQP * 4);
  if (!rc && qvel) rc = copy_out(e, qvel, e->qvel, (size_t)e->N * NVP * 4);
  return rc;
}
// final (qpos, qvel, status) rows of every env, packed on the device: out[N][MRE_FINAL_W] (device pointer), enqueued on
// the handle's stream -- the local block of the end-of-rollout all_gather (bench.py, distributed.py)
extern "C" int mre_pack_final_state(mre_env* e, float* out) {
  if (!e || !out) return fail(MRE_ERR_ARG, "null");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, out) != hipSuccess || at.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return fail(MRE_ERR_ARG, "mre_pack_final_state: out must be a device pointer");
  }
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  mre_launch_pack_final(e->N, e->qpos, e->qvel, e->status, out, e->stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}
extern "C" int mre_set_warmstart(mre_env* e, const float* w) {
  if (!e || !w) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  return copy_in(e, e->qacc_ws, w, (size_t)e->N * NVP * 4);
}
extern "C" int mre_get_warmstart(mre_env* e, float* w) {
  if (!e || !w) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  return copy_out(e, w, e->qacc_ws, (size_t)e->N * NVP * 4);
}
extern "C" int mre_set_ctrl(mre_env* e, const float* ctrl) {
  if (!e || !ctrl) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  return copy_in(e, e->ctrl, ctrl, (size_t)e->N * NU * 4);
}

static void fill_args(mre_env* e, StepArgs& a) {
  memset(&a, 0, sizeof(a));
  a.M = e->dM; a.N = e->N; a.seq_stride = e->N;
  a.qpos = e->qpos; a.qvel = e->qvel; a.qacc_ws = e->qacc_ws; a.ctrl = e->ctrl; a.qfine = e->qfine;
  a.nprops = e->nprops; a.prop_size = e->prop_size;
  a.control_steps = 1; a.mode = CTRL_HELD;
  a.osc = e->d_osc_env ? e->d_osc_env : e->d_osc; a.osc_stride = e->d_osc_env ? 1 : 0;
  a.osc_target = e->osc_target; a.grip_closed = e->grip_closed;
  a.sites = e->sites; a.status = e->status; a.stats = e->stats; a.nstep = e->nstep;
  a.env_order = e->use_order ? e->order : (e->have_auto_order ? e->auto_order : nullptr);
  a.trace = e->trace; a.trace_nenv = e->trace_nenv; a.trace_max = e->trace_max; a.trace_base = e->trace_pos;
}

extern "C" int mre_step(mre_env* e, int nsubsteps, unsigned flags) {
  if (!e || nsubsteps < 0) return fail(MRE_ERR_ARG, "mre_step: bad argument");
  StepArgs a;
  fill_args(e, a);
  a.nsteps = nsubsteps; a.flags = flags;
  if (nsubsteps > 0) a.sites = nullptr;  // (site poses are refreshed by mre_get_sites: no kinematics pass for them here)
  int rc = launch_step(e, a);
  if (rc) return rc;
  if (e->trace) e->trace_pos += nsubsteps;
  return MRE_OK;
}

// T control ticks as launches of `ticks_per_launch` ticks each (every env group: one launch per chunk), enqueued from
// here without returning to the caller in between: the host stays up to `ring` launches ahead of every group.
// ticks_per_launch <= 0 or >= nticks: ONE launch for the whole sequence (mre_rollout).
extern "C" int mre_rollout_ticks(mre_env* e, const float* ctrl_seq, int nticks, int control_steps, unsigned flags,
                                 int ticks_per_launch) {
  if (!e || !ctrl_seq || nticks < 0 || control_steps < 1) return fail(MRE_ERR_ARG, "mre_rollout: bad argument");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ctrl_seq) != hipSuccess || at.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return fail(MRE_ERR_ARG, "mre_rollout: ctrl_seq must be a device pointer");
  }
  int per = (ticks_per_launch <= 0 || ticks_per_launch > nticks) ? nticks : ticks_per_launch;
  bool allow_queue = ticks_per_launch >= 2;   // the caller's cut into launches of several ticks: queue launches where they apply
  // the library's choice (ticks_per_launch <= 0) for a batch that does not fit the GPU's wave slots: queue launches
  if (ticks_per_launch <= 0 && e->queue_ok && e->queue_waves > 0 && e->N > e->queue_waves && nticks >= 2) {
    if (nticks >= e->queue_min_ticks || (nticks >= 8 && !(e->tick_tail_valid && e->tick_tail < e->queue_tail_min))) {
      // (equal parts, none of a single tick: a launch of one tick is not a queue launch)
      const int nl = (nticks + e->queue_ticks - 1) / e->queue_ticks;
      per = (nticks + nl - 1) / nl;   // (a last part of a single tick is an ordinary launch)
      allow_queue = true;
    } else {
      per = 1;   // a short window: one launch per tick and env group (mre_env::queue_min_ticks)
    }
  }
  const float* src = ctrl_seq;
  if ((e->groups.size() > 1 || e->queue_ok) && nticks > 0) {
    // a pipelined launch may be re-run (capacity fallback) after this call has returned: it reads the controls
    // from the handle's own copy (RING + 1 buffers: a launch's info is processed at the latest when the RING-th launch
    // after it is issued, so the copy of call k is needed until call k + RING has been issued)
    const size_t n = (size_t)nticks * (size_t)e->N * NU;
    if (n > e->seq_cap) {
      DRAIN_PENDING(e);
      for (float*& p : e->seq_copy) { if (p) HIPCHK(hipFree(p)); p = nullptr; HIPCHK(hipMalloc(&p, n * 4)); }
      e->seq_cap = n;
    }
    float* dst = e->seq_copy[e->seq_calls++ % (unsigned)(mre_env::RING + 1)];
    HIPCHK(hipMemcpyAsync(dst, ctrl_seq, n * 4, hipMemcpyDeviceToDevice, e->stream));
    src = dst;
  }
  for (int t0 = 0; t0 < nticks || (nticks == 0 && t0 == 0); t0 += per) {
    const int nt = nticks - t0 < per ? nticks - t0 : per;
    StepArgs a;
    fill_args(e, a);   // (trace_base follows trace_pos)
    a.nsteps = nt * control_steps; a.control_steps = control_steps; a.mode = CTRL_SEQ;
    a.ctrl_seq = src + (size_t)t0 * (size_t)e->N * NU; a.flags = flags;
    a.sites = nullptr;  // (as in mre_step)
    int rc = launch_step(e, a, false, true, allow_queue);
    if (rc) return rc;
    if (e->trace) e->trace_pos += a.nsteps;
    if (nticks == 0) break;
  }
  return MRE_OK;
}

extern "C" int mre_rollout(mre_env* e, const float* ctrl_seq, int nticks, int control_steps, unsigned flags) {
  return mre_rollout_ticks(e, ctrl_seq, nticks, control_steps, flags, 0);
}

extern "C" int mre_set_trace(mre_env* e, float* out, int nenv, int max_steps) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  if (out) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, out) != hipSuccess || at.type != hipMemoryTypeDevice) {
      (void)hipGetLastError();
      return fail(MRE_ERR_ARG, "mre_set_trace: trace buffer must be a device pointer");
    }
    if (nenv <= 0 || nenv > e->N || max_steps <= 0) return fail(MRE_ERR_ARG, "mre_set_trace: bad sizes");
  }
  e->trace = out; e->trace_nenv = out ? nenv : 0; e->trace_max = out ? max_steps : 0; e->trace_pos = 0;
  return MRE_OK;
}

extern "C" int mre_osc_configure(mre_env* e, const float* gains, const float* null_q, const float* thr,
                                 int pinv_always) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  if (gains) {
    e->osc.kp_pos = gains[0]; e->osc.kd_pos = gains[1]; e->osc.kp_ori = gains[2];
    e->osc.kd_ori = gains[3]; e->osc.kp_null = gains[4]; e->osc.kd_null = gains[5];
  }
  if (null_q) for (int k = 0; k < 7; k++) e->osc.null_q[k] = null_q[k];
  if (thr) { e->osc.pos_thresh = thr[0]; e->osc.ori_thresh = thr[1]; }
  e->osc.pinv_always = pinv_always;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->d_osc, &e->osc, sizeof(OscConfig), hipMemcpyHostToDevice));
  if (e->d_osc_env) { (void)hipFree(e->d_osc_env); e->d_osc_env = nullptr; }
  return MRE_OK;
}

// per-env controller parameters (a population of gain sets, one per env): any NULL array keeps the
// shared configuration's values; mre_osc_configure afterwards returns to one shared set
extern "C" int mre_osc_configure_env(mre_env* e, const float* gains, const float* null_q, const float* thr) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  const size_t N = (size_t)e->N;
  std::vector<OscConfig> h(N, e->osc);
  for (size_t i = 0; i < N; i++) {
    if (gains) {
      const float* g = gains + 6 * i;
      for (int k = 0; k < 6; k++)
        if (!(g[k] >= 0.f) || !std::isfinite(g[k])) return fail(MRE_ERR_ARG, "mre_osc_configure_env: gains must be finite and >= 0");
      h[i].kp_pos = g[0]; h[i].kd_pos = g[1]; h[i].kp_ori = g[2]; h[i].kd_ori = g[3]; h[i].kp_null = g[4]; h[i].kd_null = g[5];
    }
    if (null_q) for (int k = 0; k < 7; k++) h[i].null_q[k] = null_q[7 * i + k];
    if (thr) { h[i].pos_thresh = thr[2 * i]; h[i].ori_thresh = thr[2 * i + 1]; }
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  if (!e->d_osc_env) HIPCHK(hipMalloc(&e->d_osc_env, N * sizeof(OscConfig)));
  HIPCHK(hipMemcpy(e->d_osc_env, h.data(), N * sizeof(OscConfig), hipMemcpyHostToDevice));
  return MRE_OK;
}

extern "C" int mre_gripper_set(mre_env* e, const uint8_t* closed) {
  if (!e || !closed) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  return copy_in(e, e->grip_closed, closed, (size_t)e->N);
}

extern "C" int mre_get_sites(mre_env* e, float* tcp_pos, float* eef_pose, float* prop_pose) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  // refresh site poses for the current state (0 physics steps = kinematics only)
  StepArgs a;
  fill_args(e, a);
  a.nsteps = 0; a.trace = nullptr;
  launch_compact(e, a, e->stream);
  HIPCHK(hipGetLastError());
  const size_t N = (size_t)e->N;
  std::vector<float> hs(N * 16), hq;
  int rc = copy_out(e, hs.data(), e->sites, N * 64);
  if (rc) return rc;
  if (prop_pose) {
    hq.resize(N * NQP);
    rc = copy_out(e, hq.data(), e->qpos, N * NQP * 4);
    if (rc) return rc;
  }
  // gather on the host into temporaries, then copy to the (host or device) destinations
  std::vector<float> t3(N * 3), t7(N * 7), tp(N * NPROP * 7);
  for (size_t i = 0; i < N; i++) {
    for (int k = 0; k < 3; k++) t3[i * 3 + k] = hs[i * 16 + k];
    for (int k = 0; k < 7; k++) t7[i * 7 + k] = hs[i * 16 + 3 + k];
    if (prop_pose)
      for (int p = 0; p < NPROP; p++)
        for (int k = 0; k < 7; k++) tp[(i * NPROP + p) * 7 + k] = hq[i * NQP + NRV + 7 * p + k];
  }
  if (tcp_pos) { rc = copy_out(e, tcp_pos, t3.data(), N * 12); if (rc) return rc; }
  if (eef_pose) { rc = copy_out(e, eef_pose, t7.data(), N * 28); if (rc) return rc; }
  if (prop_pose) { rc = copy_out(e, prop_pose, tp.data(), N * NPROP * 28); if (rc) return rc; }
  return MRE_OK;
}

extern "C" int mre_get_status(mre_env* e, uint32_t* status) {
  if (!e || !status) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  return copy_out(e, status, e->status, (size_t)e->N * 4);
}
extern "C" int mre_get_solver_stats(mre_env* e, int32_t* stats) {
  if (!e || !stats) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  return copy_out(e, stats, e->stats, (size_t)e->N * 16);
}

extern "C" int mre_osc_set_target(mre_env* e, const float* pos, const float* quat, const float* vel,
                                  const float* angvel, const uint8_t* mask) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  // small host-side merge: targets persist per env, NULL keeps the old value
  const size_t N = (size_t)e->N;
  std::vector<float> t(N * 16);
  int rc = copy_out(e, t.data(), e->osc_target, N * 64);
  if (rc) return rc;
  std::vector<float> hp, hq, hv, hw;
  std::vector<uint8_t> hm;
  auto fetch = [&](const float* src, int w, std::vector<float>& dst) -> int {
    if (!src) return MRE_OK;
    dst.resize(N * w);
    return copy_out(e, dst.data(), src, N * w * 4);
  };
  if ((rc = fetch(pos, 3, hp)) || (rc = fetch(quat, 4, hq)) || (rc = fetch(vel, 3, hv)) ||
      (rc = fetch(angvel, 3, hw)))
    return rc;
  if (mask) { hm.resize(N); rc = copy_out(e, hm.data(), mask, N); if (rc) return rc; }
  for (size_t i = 0; i < N; i++) {
    if (mask && !hm[i]) continue;
    float* r = &t[i * 16];
    if (pos) for (int k = 0; k < 3; k++) r[k] = hp[i * 3 + k];
    if (quat) for (int k = 0; k < 4; k++) r[3 + k] = hq[i * 4 + k];
    if (vel) for (int k = 0; k < 3; k++) r[7 + k] = hv[i * 3 + k];
    if (angvel) for (int k = 0; k < 3; k++) r[10 + k] = hw[i * 3 + k];
  }
  rc = copy_in(e, e->osc_target, t.data(), N * 64);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));  // t goes out of scope
  return MRE_OK;
}

extern "C" int mre_run_controller(mre_env* e, int nticks, int control_steps, uint8_t* converged_out) {
  if (!e || nticks < 0 || control_steps < 1) return fail(MRE_ERR_ARG, "mre_run_controller: bad argument");
  // One scripted phase is 400 ticks (2000 steps).  With the capacity fallback an overflow costs a
  // re-run of the launch it happened in, so the call is cut into launches of RUN_CHUNK ticks: the
  // state round-trips through HBM exactly, the converged flag carries over (F_CONV_CONTINUE) and
  // NOT_CONVERGED is judged by the last launch only (F_CONV_OPEN on the others) -- bit-identical to
  // one launch (tests/test_gpu_api.py), and a re-run repeats at most one chunk.
  int chunk = nticks;
  bool queue = false;
  if (e->fallback && !e->large_only) {
    chunk = 50;
    // a batch that exceeds the GPU's wave slots: queue launches (mre_env::qgroup) -- an overflow is handled inside the
    // launch, so the launches are as long as the queue's
    queue = e->queue_ok && !e->compact_only && e->queue_waves > 0 && e->N > e->queue_waves && !e->use_order &&
            (nticks >= e->queue_min_ticks || (nticks >= 8 && !(e->tick_tail_valid && e->tick_tail < e->queue_tail_min)));
    if (queue) chunk = e->queue_run_ticks;
    if (const char* c = getenv("MRE_RUN_CHUNK")) { const int v = atoi(c); chunk = v > 0 ? v : nticks; }  // tuning knob
  }
  if (chunk <= 0 || chunk > nticks) chunk = nticks;
  if (queue && chunk > QUEUE_TICKS_MAX) chunk = QUEUE_TICKS_MAX;
  DRAIN(e);
  if (nticks > 0 && e->converged) HIPCHK(hipMemsetAsync(e->converged, 0, (size_t)e->N, e->stream));
  int t0 = 0;
  do {
    const int n = (nticks - t0 < chunk) ? nticks - t0 : chunk;
    StepArgs a;
    fill_args(e, a);
    a.nsteps = n * control_steps; a.control_steps = control_steps; a.mode = CTRL_OSC;
    a.converged = e->converged;
    if (t0 > 0) a.flags |= F_CONV_CONTINUE;
    if (t0 + n < nticks) a.flags |= F_CONV_OPEN;
    // (a call that is one launch and hands the converged flags back completes before it returns anyway: one
    // launch of the whole batch then costs less than one per env group)
    int rc = launch_step(e, a, false, /*pipeline_ok=*/queue || !(converged_out != nullptr && chunk >= nticks), /*allow_queue=*/queue);
    if (rc) return rc;
    if (e->trace) e->trace_pos += a.nsteps;
    t0 += n;
  } while (t0 < nticks);
  if (converged_out) { DRAIN(e); return copy_out(e, converged_out, e->converged, (size_t)e->N); }
  return MRE_OK;
}

// OSC.compute_control_output() + MinMax.compute_control_output() on the current state, no stepping
// (models/robot_arm.py:71-73): tau[N][7] arm torques, grip[N] gripper command (either may be NULL)
extern "C" int mre_osc_compute(mre_env* e, float* tau, float* grip) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  StepArgs a;
  fill_args(e, a);
  a.nsteps = 0; a.control_steps = 1; a.mode = CTRL_OSC; a.flags = F_OSC_EVAL; a.trace = nullptr;
  HIPCHK(hipSetDevice(e->device));
  launch_compact(e, a, e->stream);
  HIPCHK(hipGetLastError());
  const size_t N = (size_t)e->N;
  std::vector<float> h(N * NU);
  int rc = copy_out(e, h.data(), e->ctrl, N * NU * 4);
  if (rc) return rc;
  std::vector<float> ht(N * 7), hg(N);
  for (size_t i = 0; i < N; i++) {
    for (int k = 0; k < 7; k++) ht[i * 7 + k] = h[i * NU + k];
    hg[i] = h[i * NU + 7];
  }
  // (copy_out synchronises: the staging vectors die with this frame)
  if (tau) { rc = copy_out(e, tau, ht.data(), N * 7 * 4); if (rc) return rc; }
  if (grip) { rc = copy_out(e, grip, hg.data(), N * 4); if (rc) return rc; }
  return MRE_OK;
}

// ---- device buffers and launch arguments of k_pose_search (mre_place_props, mre_prop_place, mre_sort_colours)
static int search_buffers(mre_env* e) {
  if (e->ps_attempts) return MRE_OK;
  const size_t N = (size_t)e->N;
  HIPCHK(hipMalloc(&e->ps_attempts, N * 4)); HIPCHK(hipMalloc(&e->ps_prop, N * 4));
  HIPCHK(hipMalloc(&e->ps_tick, N * 4)); HIPCHK(hipMalloc(&e->ps_which, N * 4));
  HIPCHK(hipMalloc(&e->ps_bounds, N * 6 * 8)); HIPCHK(hipMalloc(&e->ps_pose, N * 7 * 8));
  HIPCHK(hipMalloc(&e->ps_zones, N * NPROP * 4 * 8)); HIPCHK(hipMalloc(&e->ps_pick, N * 7 * 8));
  return MRE_OK;
}
static void fill_search(mre_env* e, SearchArgs& sa) {
  memset(&sa, 0, sizeof(sa));
  sa.M = e->dM; sa.N = e->N; sa.qpos = e->qpos; sa.qfine = e->qfine; sa.nprops = e->nprops; sa.prop_size = e->prop_size;
  sa.env_ids = e->d_env_ids; sa.env_id_offset = e->env_id_offset;
  sa.attempts = e->ps_attempts; sa.fixed_prop = -1;
}

// physics.forward() + physics.data.contact on the current poses: one zero-step launch that runs the
// kinematics and the narrow phase and exports every DETECTED contact (dist < margin), per env
// [count, (geom1, geom2, dist) x CONTACT_EXPORT]; count < 0: the list was cut at -count.
static int detect_contacts(mre_env* e, const uint8_t* dmask, bool full = false, bool active_only = false) {
  const size_t N = (size_t)e->N, row = 1 + 3 * CONTACT_EXPORT;
  if (!e->contacts) HIPCHK(hipMalloc(&e->contacts, N * row * 4));
  if (full && !e->contacts_full) HIPCHK(hipMalloc(&e->contacts_full, N * CONTACT_EXPORT * 12 * 4));
  StepArgs a;
  fill_args(e, a);
  a.nsteps = 0; a.flags = F_DETECT | (active_only ? F_DETECT_ACTIVE : 0u); a.trace = nullptr; a.env_mask = dmask;
  a.contacts = e->contacts; a.contacts_full = full ? e->contacts_full : nullptr;
  a.sites = nullptr; a.geoms = nullptr;
  launch_compact(e, a, e->stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

extern "C" int mre_get_contacts(mre_env* e, int32_t* count, float* contacts) {
  if (!e || !count || !contacts) return fail(MRE_ERR_ARG, "mre_get_contacts: null");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  int rc = detect_contacts(e, nullptr);
  if (rc) return rc;
  const size_t N = (size_t)e->N, row = 1 + 3 * CONTACT_EXPORT;
  std::vector<float> h(N * row);
  rc = copy_out(e, h.data(), e->contacts, h.size() * 4);
  if (rc) return rc;
  std::vector<int32_t> hc(N);
  std::vector<float> ho(N * 3 * CONTACT_EXPORT);
  for (size_t i = 0; i < N; i++) {
    hc[i] = (int32_t)h[i * row];
    memcpy(&ho[i * 3 * CONTACT_EXPORT], &h[i * row + 1], 3 * CONTACT_EXPORT * 4);
  }
  if ((rc = copy_out(e, count, hc.data(), N * 4))) return rc;
  return copy_out(e, contacts, ho.data(), ho.size() * 4);
}

// The whole mjContact record of the same zero-step launch: rows of 15 = pos[3], frame[9], dist, geom1, geom2.
// active_only: the launch runs collide(.., detect = false), the call every step makes -- its early-outs see
// margin - gap, not margin, so this list is what the next solve would be given, not a filtered copy of the other.
extern "C" int mre_get_contacts_full(mre_env* e, int active_only, int32_t* count, float* contacts) {
  if (!e || !count || !contacts) return fail(MRE_ERR_ARG, "mre_get_contacts_full: null");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  int rc = detect_contacts(e, nullptr, true, active_only != 0);
  if (rc) return rc;
  const size_t N = (size_t)e->N, row = 1 + 3 * CONTACT_EXPORT, W = 15;
  std::vector<float> h(N * row), hf(N * CONTACT_EXPORT * 12);
  if ((rc = copy_out(e, h.data(), e->contacts, h.size() * 4))) return rc;
  if ((rc = copy_out(e, hf.data(), e->contacts_full, hf.size() * 4))) return rc;
  std::vector<int32_t> hc(N);
  std::vector<float> ho(N * CONTACT_EXPORT * W, 0.f);
  for (size_t i = 0; i < N; i++) {
    const int32_t c = (int32_t)h[i * row];
    const bool cut = c < 0 || c > CONTACT_EXPORT;   // capacity overflow, or more contacts than rows
    const int n = cut ? CONTACT_EXPORT : c;
    hc[i] = cut ? -n : n;
    for (int k = 0; k < n; k++) {
      float* o = &ho[(i * CONTACT_EXPORT + k) * W];
      memcpy(o, &hf[(i * CONTACT_EXPORT + k) * 12], 12 * 4);
      const float* t = &h[i * row + 1 + 3 * k];
      o[12] = t[2]; o[13] = t[0]; o[14] = t[1];
    }
  }
  if ((rc = copy_out(e, count, hc.data(), N * 4))) return rc;
  return copy_out(e, contacts, ho.data(), ho.size() * 4);
}

// ---- PropPlacer.__call__ (environment/prop_initializer.py:164-283), batched.
// Props are placed one index at a time over the whole batch, as the reference places them one
// after the other: every env that still needs prop p draws a pose (position ~ U(workspace), yaw =
// pi U(0,1); counter RNG keyed by (seed, GLOBAL env id, p * max_attempts + attempt, channel)) in its
// own attempt loop on the device (k_pose_search evaluates physics.forward() of the moved prop: its
// frame and the narrow phase of its pairs), and the pose is rejected while prop p
// has any detected contact (dist < margin 0.15) with a geom other than the table -- placed props and
// robot geoms alike (_has_collisions_with_prop, :121-140; props not yet placed are parked out of
// reach, the reference disables their contacts).  Then the physics settles with the robot frozen;
// every env leaves the loop by itself once max |qvel| < 1e-3 and max |qacc| < 1e-2 after at least
// `settle_steps` steps (:240-258), at most 2 s; envs that never settle get MRE_ST_NOT_SETTLED.
extern "C" int mre_place_props(mre_env* e, const uint8_t* mask, uint64_t seed, const float* ws_min,
                               const float* ws_max, int max_attempts, int settle_steps) {
  if (!e || !ws_min || !ws_max || max_attempts < 1) return fail(MRE_ERR_ARG, "mre_place_props: bad argument");
  DRAIN(e);
  const size_t N = (size_t)e->N;
  std::vector<uint8_t> hm(N, 1);
  int rc;
  if (mask) { rc = copy_out(e, hm.data(), mask, N); if (rc) return rc; }
  std::vector<int> np(N);
  if ((rc = copy_out(e, np.data(), e->nprops, N * 4))) return rc;
  double lo[3], hi[3];
  for (int k = 0; k < 3; k++) { lo[k] = ws_min[k]; hi[k] = ws_max[k]; }
  if ((rc = search_buffers(e))) return rc;
  if (settle_steps > 0 && !e->settle_steps) HIPCHK(hipMalloc(&e->settle_steps, N * 4));
  if (settle_steps > 0) HIPCHK(hipMemsetAsync(e->settle_steps, 0, N * 4, e->stream));
  std::vector<int> att(N), hs(N), nst(N);
  std::vector<uint32_t> st(N);
  std::vector<float> qp(N * NQP);
  std::vector<uint8_t> todo = hm;      // envs whose cubes are (still) to be placed
  std::vector<uint8_t> failed(N, 0);   // no pose within max_attempts for one of the env's cubes
  e->last_settle_max = 0;
  // PropPlacer.place_and_settle (environment/prop_initializer.py:240-258): place, settle with the robot frozen,
  // and place AGAIN the envs whose cubes are still moving after max_settle_physics_time -- up to
  // max_settle_physics_attempts (10) times, per env (the other envs keep what they have)
  const int max_settle_attempts = settle_steps > 0 ? 10 : 1;
  for (int round = 0; round < max_settle_attempts; round++) {
    bool any = false;
    for (size_t i = 0; i < N; i++) any = any || todo[i];
    if (!any) break;
    if ((rc = copy_out(e, qp.data(), e->qpos, qp.size() * 4)) || (rc = copy_out(e, nst.data(), e->nstep, N * 4))) return rc;
    // props that are about to be placed start from their parking pose
    for (size_t i = 0; i < N; i++)
      if (todo[i])
        for (int p = 0; p < NPROP; p++) {
          float* q = &qp[i * NQP + NRV + 7 * p];
          for (int k = 0; k < 3; k++) q[k] = e->hM.park_pos[p][k];
          q[3] = 1.f; q[4] = q[5] = q[6] = 0.f;
        }
    if ((rc = copy_in(e, e->qpos, qp.data(), qp.size() * 4)) || (rc = copy_in(e, e->mask, todo.data(), N))) return rc;
    {   // the parked poses and the velocities written here are float32 values: their low-order words are zero
      std::vector<float> hf(N * QFINE_ROW);
      if ((rc = copy_out(e, hf.data(), e->qfine, hf.size() * 4))) return rc;
      for (size_t i = 0; i < N; i++)
        if (todo[i]) for (int k = QFINE_CUBE_Q; k < QFINE_ROW; k++) hf[i * QFINE_ROW + k] = 0.f;
      if ((rc = copy_in(e, e->qfine, hf.data(), hf.size() * 4))) return rc;
    }
    if (round > 0) {   // a second try starts from rest
      std::vector<float> z(N * NVP, 0.f), qv(N * NVP);
      if ((rc = copy_out(e, qv.data(), e->qvel, qv.size() * 4))) return rc;
      for (size_t i = 0; i < N; i++)
        if (todo[i]) for (int k = NRV; k < NVP; k++) qv[i * NVP + k] = 0.f;
      if ((rc = copy_in(e, e->qvel, qv.data(), qv.size() * 4))) return rc;
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    // one search launch per prop index: every env that still needs prop p runs its own attempt loop on
    // the device (k_pose_search) and writes the accepted pose into its qpos row
    for (int p = 0; p < NPROP; p++) {
      SearchArgs sa;
      fill_search(e, sa);
      sa.env_mask = e->mask; sa.seed = seed; sa.fixed_prop = p;
      for (int k = 0; k < 3; k++) { sa.shared_bounds[k] = lo[k]; sa.shared_bounds[3 + k] = hi[k]; }
      sa.tick0 = ((long long)round * NPROP + p) * (long long)max_attempts;
      sa.max_attempts = max_attempts; sa.yaw_mode = 1; sa.max_dist = INFINITY; sa.commit = 1;
      mre_launch_pose_search(&sa, e->stream);
      HIPCHK(hipGetLastError());
      if ((rc = copy_out(e, att.data(), e->ps_attempts, N * 4))) return rc;
      bool dropped = false;
      for (size_t i = 0; i < N; i++)
        if (todo[i] && p < np[i] && att[i] <= 0) { failed[i] = 1; todo[i] = 0; dropped = true; }
      // (_REJECTION_SAMPLING_FAILED is an exception of ONE env in the reference: here that env is flagged
      //  MRE_ST_PLACEMENT_FAILED, its remaining cubes stay parked, and the other envs carry on)
      if (dropped && (rc = copy_in(e, e->mask, todo.data(), N))) return rc;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    if (settle_steps <= 0) break;
    StepArgs a;
    fill_args(e, a);
    a.trace = nullptr;
    // _max_settle_physics_time = 2 s; min time = settle_steps * dt (0.3 s in the reference)
    a.nsteps = (int)std::lround(2.0 / e->hM.opt_rec.timestep);
    if (a.nsteps < settle_steps) a.nsteps = settle_steps;
    a.flags = F_FREEZE_ROBOT | F_SETTLE_EXIT; a.env_mask = e->mask;
    a.settle_steps = e->settle_steps; a.min_settle_steps = settle_steps;
    const bool prof = e->profiling;
    e->profiling = false;  // setup, not a control tick
    rc = launch_step(e, a, /*settle=*/true);
    e->profiling = prof;
    if (rc) return rc;
    if ((rc = copy_out(e, hs.data(), e->settle_steps, N * 4))) return rc;
    if (getenv("MRE_DEBUG_PLACE")) {
      int nt = 0, ns = 0;
      for (size_t i = 0; i < N; i++) if (todo[i]) { nt++; ns += hs[i] >= 0; }
      fprintf(stderr, "mre_place_props round %d: %d envs placed, %d settled\n", round, nt, ns);
    }
    int settled_now = 0;
    for (size_t i = 0; i < N; i++) {
      if (!todo[i]) continue;
      const int n = hs[i] < 0 ? -hs[i] : hs[i];
      if (n > e->last_settle_max) e->last_settle_max = n;
      if (hs[i] >= 0) { todo[i] = 0; settled_now++; }               // settled
    }
    // a round in which NO env came to rest is not bad luck of a placement but the solver: PGS at 100 sweeps leaves a
    // friction creep of 1e-3 rad/s on resting cubes that never passes the velocity test (all 4096 envs of the bench,
    // in every one of ten rounds; with Newton all settle in the first).  Placing again cannot help: stop, flag them
    // (only where that diagnosis can hold: PGS, a batch large enough that "none of them" is not chance, first round;
    //  a lone env keeps its ten attempts like the reference's)
    const bool give_up = settled_now == 0 && round == 0 && N >= 64 && e->solver != MRE_SOLVER_NEWTON;
    bool left = false;
    for (size_t i = 0; i < N; i++) left = left || todo[i];
    if (left) {
      // `physics.data.time = original_time` after EVERY failed attempt, the last one included
      // (prop_initializer.py:240-258): the clock goes back for every env that did not settle in this round
      std::vector<int> now(N);
      if ((rc = copy_out(e, now.data(), e->nstep, N * 4))) return rc;
      for (size_t i = 0; i < N; i++) if (todo[i]) now[i] = nst[i];
      if ((rc = copy_in(e, e->nstep, now.data(), N * 4))) return rc;
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (give_up) break;
  }
  // status: envs that never settled (the reference logs _SETTLING_PHYSICS_FAILED and goes on), envs without a pose
  bool flag = false;
  for (size_t i = 0; i < N; i++) flag = flag || failed[i] || (settle_steps > 0 && todo[i]);
  if (flag) {
    if ((rc = copy_out(e, st.data(), e->status, N * 4))) return rc;
    for (size_t i = 0; i < N; i++) {
      if (failed[i]) st[i] |= MRE_ST_PLACEMENT_FAILED;
      else if (settle_steps > 0 && todo[i]) st[i] |= MRE_ST_NOT_SETTLED;
    }
    if ((rc = copy_in(e, e->status, st.data(), N * 4))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return MRE_OK;
}

extern "C" int mre_get_settle_steps(mre_env* e, int32_t* steps) {
  if (!e || !steps) return fail(MRE_ERR_ARG, "mre_get_settle_steps: null");
  DRAIN(e);
  if (!e->settle_steps) return fail(MRE_ERR_ARG, "mre_get_settle_steps: no settle has run");
  return copy_out(e, steps, e->settle_steps, (size_t)e->N * 4);
}

// ---- prop_place (tasks/rearrangement.py:597-665), batched: env i looks for a pose of cube prop[i] in
// [bounds[i][0:3], bounds[i][3:6]] (the reference's min_pose / max_pose) with orientation Ry(180 deg),
// rejected while a detected contact with a geom other than the table has dist <= max_dist (0.05 in the
// reference).  Draw t of env i is keyed by (seed, global env id, tick[i] + t).  The physics state is not
// touched (the reference works on a deepcopy).  attempts[i]: draws used, 0 = nothing asked (prop[i] < 0),
// < 0 = no pose within max_attempts (the reference raises "Failed to find collision free place pose.").
extern "C" int mre_prop_place(mre_env* e, uint64_t seed, const int32_t* prop, const double* bounds, const int32_t* tick,
                              int max_attempts, float max_dist, double* pose, int32_t* attempts) {
  if (!e || !prop || !bounds || !tick || !pose || !attempts || max_attempts < 1)
    return fail(MRE_ERR_ARG, "mre_prop_place: bad argument");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  const size_t N = (size_t)e->N;
  int rc = search_buffers(e);
  if (rc) return rc;
  if ((rc = copy_in(e, e->ps_prop, prop, N * 4)) || (rc = copy_in(e, e->ps_bounds, bounds, N * 48)) ||
      (rc = copy_in(e, e->ps_tick, tick, N * 4)))
    return rc;
  HIPCHK(hipMemsetAsync(e->ps_pose, 0, N * 56, e->stream));
  SearchArgs sa;
  fill_search(e, sa);
  sa.seed = seed; sa.prop = e->ps_prop; sa.bounds = e->ps_bounds; sa.tick_base = e->ps_tick;
  sa.max_attempts = max_attempts; sa.yaw_mode = 0;
  sa.fixed_quat[0] = 0.0; sa.fixed_quat[1] = 0.0; sa.fixed_quat[2] = 1.0; sa.fixed_quat[3] = 0.0;  // mju_mat2Quat(Ry(180 deg))
  sa.max_dist = max_dist; sa.commit = 0; sa.pose = e->ps_pose;
  mre_launch_pose_search(&sa, e->stream);
  HIPCHK(hipGetLastError());
  if ((rc = copy_out(e, pose, e->ps_pose, N * 56))) return rc;
  return copy_out(e, attempts, e->ps_attempts, N * 4);
}

// ---- sort_colours (tasks/rearrangement.py:700-751), batched and on the device: the first cube (prop
// order) outside its colour's zone, prop_pick for it (:579-595) and prop_place inside the zone (z = 0.4).
// zones [N][4][4]: lo x, lo y, hi x, hi y of every cube's zone; call_counts[i] * 10000 is the first tick of
// env i's place draws (seed + 1 keys them, like the host restatement demo_logic.batched_place_pose).
// which[i]: selected cube, -1 = every cube is in its zone (pick / place rows are then unspecified).
extern "C" int mre_sort_colours(mre_env* e, uint64_t seed, const int32_t* call_counts, const double* zones,
                                int max_attempts, float max_dist, int32_t* which, double* pick, double* place,
                                int32_t* attempts) {
  if (!e || !call_counts || !zones || !which || !pick || !place || !attempts || max_attempts < 1)
    return fail(MRE_ERR_ARG, "mre_sort_colours: bad argument");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  const size_t N = (size_t)e->N;
  int rc = search_buffers(e);
  if (rc) return rc;
  std::vector<int32_t> ticks(N);
  if ((rc = copy_out(e, ticks.data(), call_counts, N * 4))) return rc;
  for (size_t i = 0; i < N; i++) ticks[i] *= 10000;   // MAX_PLACE_ATTEMPTS draws reserved per call
  if ((rc = copy_in(e, e->ps_tick, ticks.data(), N * 4)) || (rc = copy_in(e, e->ps_zones, zones, N * NPROP * 32))) return rc;
  SortArgs so;
  so.M = e->dM; so.N = e->N; so.qpos = e->qpos; so.nprops = e->nprops; so.zones = e->ps_zones; so.place_z = 0.4;
  so.which = e->ps_which; so.pick = e->ps_pick; so.bounds = e->ps_bounds;
  mre_launch_sort_select(&so, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(e->ps_pose, 0, N * 56, e->stream));
  SearchArgs sa;
  fill_search(e, sa);
  sa.seed = seed + 1; sa.prop = e->ps_which; sa.bounds = e->ps_bounds; sa.tick_base = e->ps_tick;
  sa.max_attempts = max_attempts; sa.yaw_mode = 0;
  sa.fixed_quat[2] = 1.0;
  sa.max_dist = max_dist; sa.commit = 0; sa.pose = e->ps_pose;
  mre_launch_pose_search(&sa, e->stream);
  HIPCHK(hipGetLastError());
  if ((rc = copy_out(e, which, e->ps_which, N * 4)) || (rc = copy_out(e, pick, e->ps_pick, N * 56)) ||
      (rc = copy_out(e, place, e->ps_pose, N * 56)))
    return rc;
  return copy_out(e, attempts, e->ps_attempts, N * 4);
}

// Per-env record of the last guarded launch (the rows the capacity fallback and the dispatch order read):
// info[i] = {overflow flag (-1: env was not part of the launch), max contacts | duration << 16 (s_memtime
// ticks >> 10), max constraint rows, max robot rows | max cube-cube contacts << 16}.
extern "C" int mre_get_launch_info(mre_env* e, int32_t* info) {
  if (!e || !info) return fail(MRE_ERR_ARG, "mre_get_launch_info: null");
  DRAIN(e);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  return copy_out(e, info, e->h_info_last, (size_t)e->N * 16);
}

extern "C" int mre_set_env_ids(mre_env* e, const long long* ids) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  if (ids) e->env_ids.assign(ids, ids + e->N); else e->env_ids.clear();
  if (e->d_env_ids) { HIPCHK(hipFree(e->d_env_ids)); e->d_env_ids = nullptr; }
  if (ids) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMalloc(&e->d_env_ids, (size_t)e->N * 8));
    return copy_in(e, e->d_env_ids, e->env_ids.data(), (size_t)e->N * 8);
  }
  return MRE_OK;
}

extern "C" int mre_set_env_id_offset(mre_env* e, long long offset) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  e->env_ids.clear();
  if (e->d_env_ids) { (void)hipFree(e->d_env_ids); e->d_env_ids = nullptr; }
  e->env_id_offset = offset;
  return MRE_OK;
}

extern "C" int mre_profile_enable(mre_env* e, int on) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  e->profiling = on != 0;
  e->events_used = 0;
  return MRE_OK;
}
extern "C" int mre_profile_read(mre_env* e, float* total_ms, int* launches) {
  if (!e || !total_ms || !launches) return fail(MRE_ERR_ARG, "null");
  DRAIN(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  float tot = 0.f;
  for (size_t k = 0; k < e->events_used; k++) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->events[k].first, e->events[k].second));
    tot += ms;
  }
  *total_ms = tot; *launches = (int)e->events_used;
  e->events_used = 0;
  return MRE_OK;
}

extern "C" int mre_set_env_order(mre_env* e, const int32_t* order) {
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  DRAIN(e);
  if (!order) { e->use_order = false; return MRE_OK; }
  int rc = copy_in(e, e->order, order, (size_t)e->N * 4);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  e->use_order = true;
  return MRE_OK;
}

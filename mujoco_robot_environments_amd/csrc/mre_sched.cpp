// mre_sched.cpp -- how stepping launches are issued: the capacity fallback, the pipelined env groups with their ring of
// unprocessed launches, and the queue launches.  What a launch computes is the kernels' business; the rules applied
// here are mre_policy.h's.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "mre_env.h"
#include "mre_launch.h"

using namespace mre;

// solver-specific instantiations of the step kernel (opt_solver of the model, mre_set_solver)
static void launch_compact(const mre_env* e, const StepArgs& a, hipStream_t st, bool settle = false) {
  const StepKernels& K = step_kernels(e->solver);
  (settle ? K.settle : K.step)(&a, st);
}
static void launch_large(const mre_env* e, const StepArgs& a, hipStream_t st) { step_kernels(e->solver).large(&a, st); }

// The compact kernel on `st` for the envs of `a` that are not flagged large and, when one is (run_large), the large
// kernel for those beside it on `st2`, joined into `st` again.
static int launch_split(const mre_env* e, const StepArgs& a, bool run_large, bool settle, hipStream_t st, hipStream_t st2,
                        hipEvent_t ev_fork, hipEvent_t ev_join) {
  StepArgs ac = a;
  ac.want_large = 0;
  if (run_large) {
    HIPCHK(hipEventRecord(ev_fork, st));
    HIPCHK(hipStreamWaitEvent(st2, ev_fork, 0));
    StepArgs al = a;
    al.want_large = 1;
    launch_large(e, al, st2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev_join, st2));
  }
  launch_compact(e, ac, st, settle);
  HIPCHK(hipGetLastError());
  if (run_large) HIPCHK(hipStreamWaitEvent(st, ev_join, 0));
  return MRE_OK;
}

// The fallback decisions (policy::decide) for the envs [lo, lo + n) from a launch's info: flags, counters and the re-run
// marks (h_rerun).  Returns how many envs overflowed the compact kernel and have to be re-run.
static int apply_launch_info(mre_env* e, const int* info, int lo, int n, bool* changed) {
  int nrerun = 0;
  for (int i = lo; i < lo + n; i++) {
    const bool was = e->h_large[i] != 0;
    const policy::Action act = policy::decide(info + 4 * (size_t)i, was, e->solver == MRE_SOLVER_NEWTON, e->compact_only, e->large_only);
    const bool now = policy::flag_after(act, was);
    if (now != was) { e->h_large[i] = now; *changed = true; }
    if (now && !was) { e->n_large++; e->n_promotions++; } else if (was && !now) { e->n_large--; e->n_demotions++; }
    if (act == policy::HANDED_OVER) e->n_handovers++;
    e->h_rerun[i] = act == policy::RERUN;
    nrerun += act == policy::RERUN;
  }
  return nrerun;
}
// ... and the envs marked for a re-run put back to their saved rows on `st` (mask_r then selects them for the re-run)
static int restore_rerun_rows(mre_env* e, int lo, int n, uint8_t* pending, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(e->mask_r + lo, e->h_rerun.data() + lo, (size_t)n, hipMemcpyHostToDevice, st));
  mre_launch_restore_rows(e->mask_r, lo, n, e->qpos, e->sv_qpos, e->qvel, e->sv_qvel, e->qacc_ws, e->sv_qacc_ws,
                          e->qfine, e->sv_qfine, e->ctrl, e->sv_ctrl, e->nstep, e->sv_nstep, e->status, e->sv_status,
                          e->converged, e->sv_converged, pending, st);
  return MRE_OK;
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
  int younger[mre_env::RING];   // the staged records the younger outstanding launches read
  for (int k = 1; k < G.nout; k++) younger[k - 1] = G.out[(slot + k) % mre_env::RING].stage;
  const int fs = policy::free_stage(G.cur, younger, G.nout - 1);
  int* const order_stage = G.h_order + (size_t)fs * (size_t)e->N;
  bool changed = false;
  const long long handovers0 = e->n_handovers;
  const int nrerun = apply_launch_info(e, info, G.lo, G.n, &changed);
  if (&G == &e->qgroup) e->queue_last_handovers = (int)(e->n_handovers - handovers0);
  else if (O.args.nsteps == O.args.control_steps && (e->tail_samples++ & 3u) == 0u && G.n >= 256) {
    // spread of this tick's durations over the group's envs (mre_env::tick_tail)
    float ratio;
    e->tail_scratch.resize((size_t)G.n);
    if (policy::tick_tail_ratio(info, G.lo, G.n, e->tail_scratch.data(), &ratio)) {
      e->tick_tail = e->tick_tail_valid ? 0.9f * e->tick_tail + 0.1f * ratio : ratio;
      e->tick_tail_valid = true;
    }
  }
  // (what is decided here takes effect with the NEXT launch enqueued for the group -- the one after the younger
  //  outstanding launch -- which reads the staged record straight from mapped host memory)
  // longest processing time first within the group; no duration reported: the order it has
  if (policy::sort_longest_first(info, G.lo, G.n, order_stage) == 0)
    memcpy(order_stage + G.lo, G.h_order + (size_t)G.cur * (size_t)e->N + G.lo, (size_t)G.n * 4);
  if (nrerun > 0) {
    int rc = restore_rerun_rows(e, G.lo, G.n, e->d_pending, G.st);
    if (rc) return rc;
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
int mre::drain(mre_env* e, bool api_call) {
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

// a launch under the capacity fallback: split by the envs' flags, state rows copied aside, launch info reported
static void guard_args(mre_env* e, StepArgs& a) {
  a.large = e->d_large; a.launch_info = e->d_launch_info;
  a.sv_qpos = e->sv_qpos; a.sv_qvel = e->sv_qvel; a.sv_qacc_ws = e->sv_qacc_ws; a.sv_qfine = e->sv_qfine;
  a.sv_ctrl = e->sv_ctrl; a.sv_status = e->sv_status; a.sv_converged = e->sv_converged; a.sv_nstep = e->sv_nstep;
}

// Enqueue one launch of a group (queue: a queue launch, the group is mre_env::qgroup) behind what it has in flight.
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
    (void)policy::sort_longest_first(e->h_info_last, G.lo, G.n, G.h_order + (size_t)G.cur * N);
  }
  a.N = G.n; a.env_order = G.d_order + (size_t)G.cur * N + G.lo; a.seq_stride = e->N;
  hipEvent_t p0, p1;   // profiling bracket of the launch
  rc = profile_events(e, &p0, &p1);
  if (rc) return rc;
  HIPCHK(hipStreamWaitEvent(G.st, e->ev_main, 0));
  if (p0) HIPCHK(hipEventRecord(p0, G.st));
  guard_args(e, a);
  a.pending = e->d_pending;
  const int slot = (G.head + G.nout) % mre_env::RING;
  a.large = e->d_large_stage + (size_t)G.cur * N;
  a.launch_info = e->d_launch_info + (size_t)slot * 4 * N;
  const uint8_t* const fl = e->h_large_stage + (size_t)G.cur * N;   // (the very flags the kernels will read)
  if (queue) {
    // Queue launch: compact waves on G.st, the large kernel's waves next to them on G.st2 (capacity fallback inside the
    // launch: mre_kernels.hip, queue_pop).  Ready lists, per-env accumulators and the count of finished envs start at
    // zero (one block from the allocation's start, a multiple of 16 bytes); the envs flagged large are bucket 0 of the
    // large shard.
    StepArgs ac = a;
    ac.want_large = 0;
    const StepKernels& K = step_kernels(e->solver);
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
    // 1. the large kernel's waiting launch, first: see step_body (q_gen)
    StepArgs al = ac;
    al.want_large = 1; al.q_wait = 1;
    const int lw = policy::queue_large_waves(e->h_info_last, fl, G.lo, G.n, nl, e->queue_last_handovers,
                                             policy::queue_spare_large(e->queue_last_handovers, e->queue_spare_large),
                                             e->queue_large_waves_max);
    // (test knob MRE_QUEUE_TEST_SERIAL=1: on the compact kernel's own stream, i.e. strictly before it -- what a profiler
    //  that serialises dispatches makes of the two streams; the launch then leaves after its bounded wait and the one
    //  behind the compact kernel does the large kernel's whole share)
    hipStream_t const st_large = e->queue_test_serial ? G.st : G.st2;
    K.queue_large(&al, lw, st_large);
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
    K.queue(&ac, nwaves, G.st);
    HIPCHK(hipGetLastError());
    // Behind the compact kernel, the large kernel once more, not waiting: nothing to do when the two ran side by side
    // (a few microseconds), the rest of the job when they did not -- results never depend on how the GPU overlaps them.
    // (as many waves as the GPU holds of the large kernel: when a scripted phase closes hundreds of grasps inside one
    //  launch, the hand-overs outnumber the waiting launch's spare waves and pile up behind them -- here, with the compact
    //  kernel gone, they all run at once)
    al.q_wait = 0;
    const int sweep = G.n < 3 * e->queue_large_waves_max ? G.n : 3 * e->queue_large_waves_max;
    K.queue_large(&al, sweep, G.st);
    e->n_queue_launches++;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamWaitEvent(G.st, G.ev_join, 0));
  } else {
    bool run_large = false;
    for (int i = G.lo; i < G.lo + G.n && !run_large; i++) run_large = fl[i] != 0;
    rc = launch_split(e, a, run_large, false, G.st, G.st2, G.ev_fork, G.ev_join);
    if (rc) return rc;
  }
  if (p1) HIPCHK(hipEventRecord(p1, G.st));
  // (the kernels stored their 16 B of launch info per env into mapped host memory: the event is all that follows)
  HIPCHK(hipEventRecord(G.out[slot].ev_info, G.st));
  G.out[slot].args = a;
  G.out[slot].stage = G.cur;
  G.nout++;
  return MRE_OK;
}
// One group's part of a stepping call: finish its previous launch, enqueue the new one, do not wait.
static int launch_group(mre_env* e, mre_env::Group& G, const StepArgs& a_full, bool queue = false) {
  while (G.nout > policy::ring_keep(a_full.nsteps, e->ring)) {
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
int mre::launch_step(mre_env* e, const StepArgs& a, bool settle, bool pipeline_ok, bool allow_queue) {
  if (e->broken) return drain(e);   // (reports the failure)
  HIPCHK(hipSetDevice(e->device));  // the HIP current device is per thread; callers may have moved it
  const bool guarded = e->fallback && a.nsteps > 0 && (a.flags & F_NO_CONSTRAINTS) == 0;
  if (++e->calls_since_drain >= 2) e->sync_streak = 0;
  // a launch that only steps the whole batch: no mask, no caller's order, nothing exported, no early exit
  const bool plain = pipeline_ok && guarded && !settle && a.env_mask == nullptr && !e->use_order && a.contacts == nullptr &&
                     a.settle_steps == nullptr && a.geoms == nullptr && (a.flags & (F_DETECT | F_SETTLE_EXIT | F_OSC_EVAL)) == 0;
  const bool pipelined = plain && e->sync_streak < 2 && e->groups.size() > 1 && a.trace == nullptr;
  // a rollout of several ticks over more envs than the GPU holds waves: one queue launch of all envs (mre_env::qgroup)
  const bool queue = plain && allow_queue && policy::queue_fits(e->queue_ok, e->queue_waves, e->N) && !e->compact_only && !e->large_only &&
                     (a.mode == CTRL_SEQ || a.mode == CTRL_OSC) && a.control_steps > 0 && a.nsteps % a.control_steps == 0 &&
                     a.nsteps >= 2 * a.control_steps && a.nsteps <= QUEUE_TICKS_MAX * a.control_steps;
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
        if (!done[g] && (e->groups[g].nout <= policy::ring_keep(a.nsteps, e->ring) ||   // (nothing to wait for)
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
  hipEvent_t e0, e1;
  { int rc = profile_events(e, &e0, &e1); if (rc) return rc; }
  if (e0) HIPCHK(hipEventRecord(e0, e->stream));
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
    StepArgs ag = a;
    guard_args(e, ag);
    // (recounted from the flags every launch: an env flagged large is masked out of the compact
    // kernel, so the large kernel MUST run whenever a flag is set)
    e->n_large = 0;
    for (size_t i = 0; i < N; i++) e->n_large += e->h_large[i];
    { int rc = launch_split(e, ag, e->n_large > 0, settle, e->stream, e->stream2, e->ev_fork, e->ev_join); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(e->stream));   // (launch info: stored to mapped host memory by the kernels)
    memcpy(e->h_info_last, e->h_launch_info, N * 16);
    bool changed = false;
    const int nrerun = apply_launch_info(e, e->h_launch_info, 0, e->N, &changed);
    // dispatch order for the next launch: longest first; no duration reported: none
    if (!e->use_order) {
      e->have_auto_order = policy::sort_longest_first(e->h_launch_info, 0, e->N, e->h_auto_order) > 0;
      // (the pinned staging buffer is rewritten only after the next launch's read-back sync)
      if (e->have_auto_order) HIPCHK(hipMemcpyAsync(e->auto_order, e->h_auto_order, N * 4, hipMemcpyHostToDevice, e->stream));
    }
    if (nrerun > 0) {
      int rc = restore_rerun_rows(e, 0, e->N, nullptr, e->stream);
      if (rc) return rc;
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

// ------------------------------------------------------------------- set-up (the release is mre_destroy's: the handle owns all of it)
// a group's stream pair (the large kernel's at `pr2`), its fork / join events and one event per ring entry
static int group_create(mre_env* e, mre_env::Group& G, int pr, int pr2) {
  int rc;
  if ((rc = new_stream(e, &G.st, &pr)) || (rc = new_stream(e, &G.st2, &pr2)) || (rc = new_event(e, &G.ev_fork)) ||
      (rc = new_event(e, &G.ev_join)))
    return rc;
  for (auto& o : G.out) if ((rc = new_event(e, &o.ev_info))) return rc;
  return MRE_OK;
}

int mre::sched_create(mre_env* e) {
  const int num_envs = e->N;
  const size_t N = (size_t)num_envs;
  int least = 0, greatest = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  // env groups of the pipelined stepping path (MRE_GROUPS = 1: every call completes before it returns)
  int ng = 4, min_envs = 512;   // (measured on the bench: 2, 3 and 4 groups are within 1 % for Newton, 4 best for PGS)
  if (const char* g = getenv("MRE_GROUPS")) ng = atoi(g);
  if (const char* g = getenv("MRE_GROUP_MIN")) min_envs = atoi(g);   // test knob: smallest group worth a launch of its own
  if (ng < 1) ng = 1;
  if (ng > 8) ng = 8;
  if (const char* r = getenv("MRE_RING")) { e->ring = atoi(r); if (e->ring < 2) e->ring = 2; if (e->ring > mre_env::RING) e->ring = mre_env::RING; }
  while (ng > 1 && num_envs < min_envs * ng) ng--;
  const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
  int rc;
  if ((rc = alloc_host(e, &e->h_grp_order, mre_env::NSTAGE * N * 4, mapped, &e->d_grp_order))) return rc;
  for (int k = 0; k < mre_env::NSTAGE; k++)
    for (int i = 0; i < num_envs; i++) e->h_grp_order[(size_t)k * N + i] = i;
  if ((rc = new_event(e, &e->ev_main))) return rc;
  e->groups.resize(ng);
  // the queue's group: all envs, default stream priority
  auto& Q = e->qgroup;
  Q.lo = 0; Q.n = num_envs;
  if ((rc = alloc_host(e, &e->h_qgrp_order, mre_env::NSTAGE * N * 4, mapped, &Q.d_order))) return rc;
  Q.h_order = e->h_qgrp_order;
  for (int k = 0; k < mre_env::NSTAGE; k++)
    for (int i = 0; i < num_envs; i++) Q.h_order[(size_t)k * N + i] = i;
  // the large kernel's waves on a stream of HIGHER priority: its own hardware queue (streams of one priority share a
  // few), and its few workgroups are placed before the compact kernel's 2048 fill the compute units' LDS
  if ((rc = group_create(e, Q, least, greatest))) return rc;
  if (const char* q = getenv("MRE_QUEUE")) e->queue_ok = atoi(q) != 0;
  if (const char* q = getenv("MRE_QUEUE_TICKS")) { const int v = atoi(q); if (v >= 2 && v <= QUEUE_TICKS_MAX) e->queue_ticks = v; }
  if (e->queue_run_ticks > e->queue_ticks) e->queue_run_ticks = e->queue_ticks;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, e->device));
  e->queue_waves = prop.multiProcessorCount * std::min(step_kernels(MRE_SOLVER_PGS).queue_waves_per_cu(),
                                                       step_kernels(MRE_SOLVER_NEWTON).queue_waves_per_cu());
  if (const char* q = getenv("MRE_QUEUE_WAVES")) { const int v = atoi(q); if (v > 0) e->queue_waves = v; }   // test knob
  if (const char* q = getenv("MRE_QUEUE_SHARDS")) { const int v = atoi(q); if (v >= 1 && v <= QUEUE_SHARDS_MAX) e->queue_shards = v; }
  if (const char* q = getenv("MRE_QUEUE_MIN_TICKS")) { const int v = atoi(q); if (v >= 2) e->queue_min_ticks = v; }
  if (const char* q = getenv("MRE_QUEUE_TAIL_MIN")) { const float v = (float)atof(q); if (v > 0.f) e->queue_tail_min = v; }
  if (const char* q = getenv("MRE_QUEUE_TEST_SERIAL")) e->queue_test_serial = atoi(q) != 0;
  if (const char* q = getenv("MRE_QUEUE_SPARE_LARGE")) { const int v = atoi(q); if (v >= 0) e->queue_spare_large = v; }
  e->queue_large_waves_max = 2 * prop.multiProcessorCount;
  if (const char* q = getenv("MRE_QUEUE_LSHARDS")) { const int v = atoi(q); if (v >= 1 && v <= QUEUE_LSHARDS_MAX) e->queue_lshards = v; }
  if ((rc = alloc_dev(e, &e->q_ws, ((2 * (size_t)(QUEUE_SHARDS_MAX + QUEUE_LSHARDS_MAX) * QUEUE_TICKS_MAX + 16 + 4 * N +
                                     (size_t)QUEUE_TICKS_MAX * (2 * N + QUEUE_SHARDS_MAX + QUEUE_LSHARDS_MAX)) * 4 + 15) / 16 * 16)) ||
      (rc = alloc_dev(e, &e->q_gen, 64)))
    return rc;
  HIPCHK(hipMemsetAsync(e->q_gen, 0, 64, e->stream));
  if ((rc = alloc_host(e, &e->h_qlist, (size_t)(mre_env::RING + 1) * (N + 32) * 4, hipHostMallocDefault)) ||
      (rc = alloc_host(e, &e->h_q_err, 64, mapped)))
    return rc;
  *e->h_q_err = 0;
  for (int g = 0; g < ng; g++) {
    auto& G = e->groups[g];
    G.h_order = e->h_grp_order; G.d_order = e->d_grp_order;
    G.lo = (int)((long long)num_envs * g / ng);
    G.n = (int)((long long)num_envs * (g + 1) / ng) - G.lo;
    // descending stream priorities stagger the groups: the first group's workgroups are dispatched first and the
    // later groups fill the slots its slow envs leave idle (MRE_GROUP_PRIORITY=0: equal priorities)
    int pr = 0;
    const char* gp = getenv("MRE_GROUP_PRIORITY");
    if (!(gp && atoi(gp) == 0)) { pr = greatest + g; if (pr > least) pr = least; }
    // tuning knob: one digit per group, 0 = highest priority level
    if (const char* map = getenv("MRE_GROUP_PRIO_MAP")) {
      if ((int)strlen(map) > g && map[g] >= '0' && map[g] <= '9') { pr = greatest + (map[g] - '0'); if (pr > least) pr = least; }
    }
    if ((rc = group_create(e, G, pr, pr))) return rc;
  }
  return MRE_OK;
}

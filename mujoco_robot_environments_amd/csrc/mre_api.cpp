// mre_api.cpp -- the entry points of the C ABI (include/mre.h) that work on an mre_env handle; those that take a stream
// and no handle are mre_stream_api.cpp's.  Creates and destroys the handle (what it owns is recorded by mre_env.h's four
// functions), uploads the fp32 DevModel that mre_model.cpp builds from the model blob, stages host arrays and
// enqueues kernels; how stepping launches are issued is mre_sched.cpp's.  No torch types; plain pointers and sizes only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

#include "mre_env.h"
#include "mre_launch.h"
#include "mre_model.h"

using namespace mre;

static thread_local std::string g_err;
int mre::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// The opening of every entry that works on a handle.  A NULL handle, or a NULL among the pointers the entry requires
// (`args_ok`), is refused with the entry's text before any HIP call; then the handle's device is selected -- the HIP
// current device is per thread, and everything an entry allocates, copies or launches below relies on it -- and, with
// DRAIN_FIRST, what the stepping calls left pending is completed (mre::drain: the call counts as one that touches the
// state).  The stepping calls themselves and mre_wait_stream leave it pending; mre_num_envs, mre_stream and
// mre_get_solver read one member, make no HIP call and do not open with it.
enum Pending { LEAVE_PENDING, DRAIN_FIRST };
#define ENTER(e, args_ok, text, pending)                        \
  do {                                                          \
    if (!(e) || !(args_ok)) return fail(MRE_ERR_ARG, text);     \
    HIPCHK(hipSetDevice((e)->device));                          \
    if ((pending) == DRAIN_FIRST) DRAIN(e);                     \
  } while (0)

// ------------------------------------------------------------------- staging
// The caller's array to the device, enqueued on the handle's stream: it is borrowed for the call (include/mre.h).
static int copy_in(mre_env* e, void* dst, const void* src, size_t n) {
  HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, e->stream));
  return MRE_OK;
}
static int copy_out(mre_env* e, void* dst, const void* src, size_t n) {
  HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MRE_OK;
}
// Host staging in vectors of this file's own.  A host vector handed to an asynchronous copy must outlive it: fetch and
// store return only when the handle's stream has run the copy, so the vector may change or die as soon as they have
// returned, and no call site reasons about that again.  src / dst: a device array of the handle or an array of the
// caller (host or device).
template <class T> static int fetch(mre_env* e, const void* src, size_t count, std::vector<T>& h) {
  h.resize(count);
  return copy_out(e, h.data(), src, count * sizeof(T));
}
template <class T> static int store(mre_env* e, void* dst, const std::vector<T>& h) {
  return copy_out(e, dst, h.data(), h.size() * sizeof(T));
}
// Read dev[N][row], let edit(i, row i) change the rows of the envs `pick` names, write all of it back.
template <class T, class Pick, class Edit> static int patch_rows(mre_env* e, T* dev, size_t row, Pick pick, Edit edit) {
  std::vector<T> h;
  int rc = fetch(e, dev, (size_t)e->N * row, h);
  if (rc) return rc;
  for (size_t i = 0; i < (size_t)e->N; i++) if (pick(i)) edit(i, &h[i * row]);
  return store(e, dev, h);
}
// the state rows with their low-order words: qpos [N][NQP], qvel [N][NVP], qfine [N][QFINE_ROW]
static int read_state(mre_env* e, std::vector<float>& hq, std::vector<float>& hv, std::vector<float>& hf) {
  const size_t N = (size_t)e->N;
  int rc = fetch(e, e->qpos, N * NQP, hq);
  if (!rc) rc = fetch(e, e->qvel, N * NVP, hv);
  if (!rc) rc = fetch(e, e->qfine, N * QFINE_ROW, hf);
  return rc;
}
// returns device mask pointer or nullptr
static int stage_mask(mre_env* e, const uint8_t* mask, const uint8_t** dmask) {
  *dmask = nullptr;
  if (!mask) return MRE_OK;
  int rc = copy_in(e, e->mask, mask, (size_t)e->N);
  *dmask = e->mask;
  return rc;
}

static void fill_args(mre_env* e, StepArgs& a) {
  memset(&a, 0, sizeof(a));
  a.M = e->dM; a.N = e->N; a.seq_stride = e->N;
  a.qpos = e->qpos; a.qvel = e->qvel; a.qacc_ws = e->qacc_ws; a.ctrl = e->ctrl; a.qfine = e->qfine;
  a.nprops = e->nprops; a.prop_size = e->prop_size;
  a.control_steps = 1; a.mode = CTRL_HELD; a.flags = e->base_flags;
  a.osc = e->d_osc_env ? e->d_osc_env : e->d_osc; a.osc_stride = e->d_osc_env ? 1 : 0;
  a.osc_target = e->osc_target; a.grip_closed = e->grip_closed;
  a.sites = e->sites; a.status = e->status; a.stats = e->stats; a.nstep = e->nstep;
  a.env_order = e->use_order ? e->order : (e->have_auto_order ? e->auto_order : nullptr);
  a.trace = e->trace; a.trace_nenv = e->trace_nenv; a.trace_max = e->trace_max; a.trace_base = e->trace_pos;
}
// A launch of the step kernel that steps nothing -- kinematics, and whatever the flags and outputs of `a` (from fill_args,
// plus what the caller set) ask for on the current state -- on the handle's stream, outside the scheduler and untraced.
static int zero_step(mre_env* e, StepArgs& a) {
  a.nsteps = 0; a.trace = nullptr;
  step_kernels(e->solver).step(&a, e->stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ------------------------------------------------------------------- lifecycle
extern "C" const char* mre_last_error(void) { return g_err.c_str(); }

// allocation part of mre_create: on any failure the caller releases what exists via mre_destroy
static int create_buffers(mre_env* e, int num_envs, int device_id) {
  e->N = num_envs;
  e->device = device_id;
  const size_t N = (size_t)num_envs;
  const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
  int rc = new_stream(e, &e->stream);
  auto dev = [&](auto** p, size_t bytes) { if (!rc) rc = alloc_dev(e, p, bytes); };
  // (the sv_* are the rows a guarded launch copies aside, StepArgs::sv_*.  The first copy on the null stream and the first
  // memsets on the handle's stream come BEFORE stream2 and sched_create's streams exist, as they always have: with all of
  // them moved behind sched_create the per-tick launches of bench.py ran at 21.7 instead of 23.4 M env-steps/s in three
  // alternating runs, and at 23.4 again with them back here -- profiles/README.md, handle_late_memsets_bench_*.json)
  dev(&e->dM, sizeof(DevModel));
  if (rc) return rc;
  HIPCHK(hipMemcpy(e->dM, &e->hM, sizeof(DevModel), hipMemcpyHostToDevice));
  dev(&e->qpos, N * NQP * 4); dev(&e->qvel, N * NVP * 4); dev(&e->qacc_ws, N * NVP * 4); dev(&e->ctrl, N * NU * 4);
  dev(&e->qfine, N * QFINE_ROW * 4); dev(&e->sv_qfine, N * QFINE_ROW * 4); dev(&e->nstep, N * 4); dev(&e->sv_nstep, N * 4);
  if (rc) return rc;
  // (device memsets are enqueued on the handle's stream: a hipMemset on the null stream is
  // asynchronous and is NOT ordered against a non-blocking stream)
  HIPCHK(hipMemsetAsync(e->qfine, 0, N * QFINE_ROW * 4, e->stream)); HIPCHK(hipMemsetAsync(e->nstep, 0, N * 4, e->stream));
  dev(&e->nprops, N * 4); dev(&e->prop_size, N * NPROP * 3 * 4); dev(&e->osc_target, N * 16 * 4); dev(&e->grip_closed, N);
  dev(&e->converged, N); dev(&e->mask, N); dev(&e->sites, N * 16 * 4); dev(&e->status, N * 4); dev(&e->stats, N * 4 * 4);
  dev(&e->order, N * 4); dev(&e->auto_order, N * 4);
  if (!rc) rc = alloc_host(e, &e->h_auto_order, N * 4, hipHostMallocDefault);
  if (!rc) rc = new_stream(e, &e->stream2);
  if (!rc) rc = new_event(e, &e->ev_fork);
  if (!rc) rc = new_event(e, &e->ev_join);
  dev(&e->d_large, N); dev(&e->mask_r, N);
  dev(&e->sv_qpos, N * NQP * 4); dev(&e->sv_qvel, N * NVP * 4); dev(&e->sv_qacc_ws, N * NVP * 4); dev(&e->sv_ctrl, N * NU * 4);
  dev(&e->sv_status, N * 4); dev(&e->sv_converged, N);
  if (!rc) rc = alloc_host(e, &e->h_launch_info, mre_env::RING * N * 16, mapped, &e->d_launch_info);
  if (!rc) rc = alloc_host(e, &e->h_info_last, N * 16, hipHostMallocDefault);
  if (!rc) rc = alloc_host(e, &e->h_large_stage, mre_env::NSTAGE * N, mapped, &e->d_large_stage);
  dev(&e->d_pending, N);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(e->d_pending, 0, N, e->stream)); HIPCHK(hipMemsetAsync(e->d_large, 0, N, e->stream));
  memset(e->h_launch_info, 0xFF, mre_env::RING * N * 16);
  memset(e->h_info_last, 0xFF, N * 16);   // -1: no launch yet
  memset(e->h_large_stage, 0, mre_env::NSTAGE * N);
  e->h_large.assign(N, 0); e->h_rerun.assign(N, 0);
  if ((rc = sched_create(e))) return rc;
  if (const char* fb = getenv("MRE_NO_FALLBACK")) e->fallback = atoi(fb) == 0;  // profiling knob only
  if (const char* ng = getenv("MRE_NARROW_GENERIC")) e->base_flags = atoi(ng) != 0 ? F_CLIP_ALWAYS : 0u;  // comparison knob only
  if (const char* ng = getenv("MRE_NEWTON_GENERIC")) e->base_flags |= atoi(ng) != 0 ? F_NW_ALL_TILES : 0u;  // likewise: every Hessian tile
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
  if ((rc = alloc_dev(e, &e->d_osc, sizeof(OscConfig)))) return rc;
  HIPCHK(hipMemcpy(e->d_osc, &e->osc, sizeof(OscConfig), hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(e->stream));
  rc = mre_reset(e, nullptr);
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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    delete e;
    return fail(MRE_ERR_NOGPU, "mre_create: no HIP device visible (the HIP path has no CPU fallback)");
  }
  if (device_id < 0 || device_id >= ndev) {
    delete e;
    return fail(MRE_ERR_ARG, "mre_create: device_id out of range");
  }
  const int rc = create_buffers(e, num_envs, device_id);
  if (rc != MRE_OK) {
    const std::string msg = g_err;  // mre_destroy must not clobber the reason
    mre_destroy(e);
    g_err = msg;
    return rc;
  }
  *out = e;
  return MRE_OK;
}

// Drain, let every stream of the handle finish, then release what the handle recorded: device memory, host memory,
// events, streams.
extern "C" int mre_destroy(mre_env* e) {
  if (!e) return MRE_OK;
  (void)hipSetDevice(e->device);
  (void)drain(e);
  if (getenv("MRE_DEBUG_TIMING") && e->dbg_calls > 0)
    fprintf(stderr, "mre: %ld pipelined calls, %.1f us per call in the library, of which %.1f us waiting for launch info\n",
            e->dbg_calls, 1e6 * e->dbg_call_s / e->dbg_calls, 1e6 * e->dbg_wait_s / e->dbg_calls);
  for (hipStream_t s : e->owned.streams) (void)hipStreamSynchronize(s);
  for (void* p : e->owned.dev) (void)hipFree(p);
  for (void* p : e->owned.host) (void)hipHostFree(p);
  for (hipEvent_t ev : e->owned.events) (void)hipEventDestroy(ev);
  for (hipStream_t s : e->owned.streams) (void)hipStreamDestroy(s);
  delete e;
  return MRE_OK;
}

extern "C" int mre_num_envs(const mre_env* e) { return e ? e->N : 0; }
extern "C" void* mre_stream(mre_env* e) { return e ? (void*)e->stream : nullptr; }
extern "C" int mre_sync(mre_env* e) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  HIPCHK(hipStreamSynchronize(e->stream));
  return MRE_OK;
}

extern "C" int mre_set_props(mre_env* e, const int32_t* nprops, const float* prop_half_size) {
  ENTER(e, nprops && prop_half_size, "mre_set_props: null", DRAIN_FIRST);
  int rc = copy_in(e, e->nprops, nprops, (size_t)e->N * 4);
  if (rc) return rc;
  return copy_in(e, e->prop_size, prop_half_size, (size_t)e->N * NPROP * 3 * 4);
}

extern "C" int mre_reset(mre_env* e, const uint8_t* mask) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  const uint8_t* dmask;
  int rc = stage_mask(e, mask, &dmask);
  if (rc) return rc;
  mre_launch_reset(e->dM, e->N, e->qpos, e->qvel, e->qacc_ws, e->qfine, e->ctrl, e->status, e->nstep, dmask, e->stream);
  HIPCHK(hipGetLastError());
  if (!mask) e->tick_tail_valid = false;   // (a new episode: what the per-tick launches measured no longer describes it)
  // a reset env starts on the compact kernel again (the mask may be a device pointer: read a host copy)
  bool changed = false;
  std::vector<uint8_t> hmask;
  if (mask && (rc = fetch(e, dmask, (size_t)e->N, hmask))) return rc;
  for (int i = 0; i < e->N; i++)
    if (!e->large_only && e->h_large[i] && (!mask || hmask[i])) { e->h_large[i] = 0; e->n_large--; changed = true; }
  return changed ? store(e, e->d_large, e->h_large) : MRE_OK;
}

// ---- batched overhead camera (csrc/mre_render.hip)
extern "C" int mre_set_render_colours(mre_env* e, const uint8_t* prop_rgb, const float* geom_rgb) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  const size_t N = (size_t)e->N;
  if (!e->prop_rgb) {
    int rc = alloc_dev(e, &e->prop_rgb, N * NPROP * 3);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(e->prop_rgb, 128, N * NPROP * 3, e->stream));
    for (int g = 0; g < NG; g++) for (int k = 0; k < 3; k++) e->geom_rgb[g][k] = 0.5f;
  }
  if (prop_rgb) { int rc = copy_in(e, e->prop_rgb, prop_rgb, N * NPROP * 3); if (rc) return rc; }
  if (geom_rgb) { memcpy(e->geom_rgb, geom_rgb, sizeof(e->geom_rgb)); e->bg_valid = false; }
  HIPCHK(hipStreamSynchronize(e->stream));
  return MRE_OK;
}

static int render_check(float fovy_deg, int height, int width, const uint8_t* rgb, const float* depth, const uint8_t* seg) {
  if (height <= 0 || width <= 0 || (width & 3) != 0 || width / 4 > 320 || !(fovy_deg > 0.f && fovy_deg < 180.f))
    return fail(MRE_ERR_ARG, "mre_render: width must be a multiple of 4 (<= 1280), 0 < fovy < 180");
  if ((rgb && !is_device_ptr(rgb)) || (depth && !is_device_ptr(depth)) || (seg && !is_device_ptr(seg)))
    return fail(MRE_ERR_ARG, "mre_render: image buffers must be device pointers");
  if (depth && ((uintptr_t)depth & 15)) return fail(MRE_ERR_ARG, "mre_render: depth must be 16-byte aligned");
  if ((rgb && ((uintptr_t)rgb & 3)) || (seg && ((uintptr_t)seg & 3)))
    return fail(MRE_ERR_ARG, "mre_render: rgb / seg must be 4-byte aligned");
  return MRE_OK;
}
// row groups per env of a render launch
static int render_row_groups(int height, int width) {
  const int rows_per_iter = 320 / (width / 4);
  int row_groups = (height + rows_per_iter - 1) / rows_per_iter;
  int cap = 8;  // 8 row groups per env: the per-workgroup geom set-up is amortised over 30 row pairs
  if (const char* rg = getenv("MRE_RENDER_ROW_GROUPS")) cap = atoi(rg);  // tuning knob
  if (cap < 1) cap = 1;
  return row_groups > cap ? cap : row_groups;
}

// what of the scene does not depend on the state: image size, camera, the arena's lights, checker and clip constants
static void render_scene(RenderArgs& r, const mre_env* e, const float* cam_pos, const float* cam_mat, float fovy_deg,
                         int height, int width) {
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
}

// The static geoms (ground plane, table: geoms 0 and 1, fixed to the world) look the same in every
// env and every frame of a camera: their image is rendered once per camera and every frame then
// starts from it and composites the moving geoms (robot hulls, cubes) on top.
constexpr int N_STATIC = 2;
// Makes the cached image that of this camera and image size (r: the frame's scene, a: the frame's geometry launch).
static int refresh_background(mre_env* e, const StepArgs& a, const RenderArgs& r, float fovy_deg, int row_groups) {
  float key[16] = {r.cam_pos[0], r.cam_pos[1], r.cam_pos[2], r.cam_mat[0], r.cam_mat[1], r.cam_mat[2], r.cam_mat[3], r.cam_mat[4],
                   r.cam_mat[5], r.cam_mat[6], r.cam_mat[7], r.cam_mat[8], fovy_deg, 0.f, 0.f, 0.f};
  if (e->bg_valid && e->bg_h == r.height && e->bg_w == r.width && memcmp(key, e->bg_key, sizeof(key)) == 0) return MRE_OK;
  if (e->bg_h != r.height || e->bg_w != r.width) {
    e->bg_h = e->bg_w = 0; e->bg_valid = false;   // (until all three exist again: a failure leaves no size beside a null)
    release(e, &e->bg_depth); release(e, &e->bg_rgb); release(e, &e->bg_seg);
    const size_t px = (size_t)r.height * r.width;
    int rc;
    if ((rc = alloc_dev(e, &e->bg_depth, px * 4)) || (rc = alloc_dev(e, &e->bg_rgb, px * 3)) || (rc = alloc_dev(e, &e->bg_seg, px)))
      return rc;
    e->bg_h = r.height; e->bg_w = r.width;
  }
  // the static geoms' poses do not depend on the env: cast them for env 0 (exported by the frame's launch even
  // when env 0 is masked out? no -- so export it unmasked once)
  if (a.env_mask) {
    StepArgs a0 = a;
    a0.env_mask = nullptr;
    int rc = zero_step(e, a0);
    if (rc) return rc;
  }
  RenderArgs b = r;
  b.N = 1; b.env_mask = nullptr; b.g0 = 0; b.g1 = N_STATIC;
  b.rgb = e->bg_rgb; b.depth = e->bg_depth; b.seg = e->bg_seg;
  mre_launch_render(&b, row_groups, e->stream);
  HIPCHK(hipGetLastError());
  memcpy(e->bg_key, key, sizeof(key));
  e->bg_valid = true;
  return MRE_OK;
}

extern "C" int mre_render(mre_env* e, const float* cam_pos, const float* cam_mat, float fovy_deg, int height, int width,
                          uint8_t* rgb, float* depth, uint8_t* seg, const uint8_t* mask) {
  ENTER(e, cam_pos && cam_mat, "mre_render: null argument", DRAIN_FIRST);
  int rc = render_check(fovy_deg, height, width, rgb, depth, seg);
  if (rc) return rc;
  if (!e->prop_rgb) { rc = mre_set_render_colours(e, nullptr, nullptr); if (rc) return rc; }
  if ((rc = alloc_dev(e, &e->geoms, (size_t)e->N * NG * 16 * 4))) return rc;
  const uint8_t* dmask;
  rc = stage_mask(e, mask, &dmask);
  if (rc) return rc;
  // geometry of the current state: a zero-step launch of the step kernel (kinematics + export)
  StepArgs a;
  fill_args(e, a);
  a.env_order = nullptr; a.env_mask = dmask; a.geoms = e->geoms;
  hipEvent_t e0, e1;   // same event bracket as launch_step: tools/bench_render.py times the camera with it
  rc = profile_events(e, &e0, &e1);
  if (rc) return rc;
  if (e0) HIPCHK(hipEventRecord(e0, e->stream));
  if ((rc = zero_step(e, a))) return rc;
  RenderArgs r;
  render_scene(r, e, cam_pos, cam_mat, fovy_deg, height, width);
  r.rgb = rgb; r.depth = depth; r.seg = seg; r.env_mask = dmask;
  const int row_groups = render_row_groups(height, width);
  bool use_bg = true;
  if (const char* nb = getenv("MRE_RENDER_NO_BACKGROUND")) use_bg = atoi(nb) == 0;  // diagnostic
  r.g0 = 0; r.g1 = NG;
  if (use_bg) {
    if ((rc = refresh_background(e, a, r, fovy_deg, row_groups))) return rc;
    r.g0 = N_STATIC;
    r.bg_depth = e->bg_depth; r.bg_rgb = e->bg_rgb; r.bg_seg = e->bg_seg;
  }
  mre_launch_render(&r, row_groups, e->stream);
  HIPCHK(hipGetLastError());
  if (e1) HIPCHK(hipEventRecord(e1, e->stream));
  return MRE_OK;
}

extern "C" int mre_set_fallback(mre_env* e, int mode) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
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

extern "C" int mre_wait_stream(mre_env* e, void* stream) {
  ENTER(e, true, "null handle", LEAVE_PENDING);
  if (!e->ev_order) { int rc = new_event(e, &e->ev_order); if (rc) return rc; }
  HIPCHK(hipEventRecord(e->ev_order, (hipStream_t)stream));
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_order, 0));
  return MRE_OK;
}

extern "C" int mre_set_solver(mre_env* e, int solver) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  if (solver != MRE_SOLVER_PGS && solver != MRE_SOLVER_NEWTON)
    return fail(MRE_ERR_ARG, "mre_set_solver: solver is 0 (PGS) or 2 (Newton)");
  HIPCHK(hipStreamSynchronize(e->stream));
  e->solver = solver;   // host-side only: it picks the kernel instantiation, no kernel reads it
  return MRE_OK;
}

extern "C" int mre_get_solver(mre_env* e) {   // (no HIP call: the return value is the solver, not a status)
  if (!e) return fail(MRE_ERR_ARG, "null handle");
  return e->solver;
}

// {queue launches so far, waves of a queue launch, control ticks per queue launch (the library's choice), enabled,
//  envs handed over to the large kernel inside a queue launch so far}
extern "C" int mre_get_queue_info(mre_env* e, long long* out5) {
  ENTER(e, out5, "mre_get_queue_info: null", DRAIN_FIRST);
  out5[0] = e->n_queue_launches; out5[1] = e->queue_waves; out5[2] = e->queue_ticks; out5[3] = e->queue_ok ? 1 : 0;
  out5[4] = e->n_handovers;
  return MRE_OK;
}

extern "C" int mre_get_fallback_stats(mre_env* e, long long* out4) {
  ENTER(e, out4, "mre_get_fallback_stats: null", DRAIN_FIRST);
  out4[0] = e->n_large; out4[1] = e->n_reruns; out4[2] = e->n_promotions; out4[3] = e->n_demotions;
  return MRE_OK;
}

extern "C" int mre_set_state(mre_env* e, const float* qpos, const float* qvel) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  int rc = MRE_OK;
  if (qpos) rc = copy_in(e, e->qpos, qpos, (size_t)e->N * NQP * 4);
  if (!rc && qvel) rc = copy_in(e, e->qvel, qvel, (size_t)e->N * NVP * 4);
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

// physics.data.qpos / .qvel as the reference holds them (float64): every coordinate is carried as a double-float pair
// on the device, the float32 row entry and its low-order word (StepArgs::qfine; qfine_of_q / qfine_of_v).  Host pointers.
extern "C" int mre_get_state_f64(mre_env* e, double* qpos, double* qvel) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  const size_t N = (size_t)e->N;
  std::vector<float> hq, hv, hf;
  int rc = read_state(e, hq, hv, hf);
  if (rc) return rc;
  for (size_t i = 0; i < N; i++) {
    if (qpos) for (int k = 0; k < NQ; k++) qpos[i * NQ + k] = (double)hq[i * NQP + k] + (double)hf[i * QFINE_ROW + qfine_of_q(k)];
    if (qvel) for (int k = 0; k < NV; k++) qvel[i * NV + k] = (double)hv[i * NVP + k] + (double)hf[i * QFINE_ROW + qfine_of_v(k)];
  }
  return MRE_OK;
}
extern "C" int mre_set_state_f64(mre_env* e, const double* qpos, const double* qvel) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  const size_t N = (size_t)e->N;
  std::vector<float> hq, hv, hf;
  int rc = read_state(e, hq, hv, hf);
  if (rc) return rc;
  for (size_t i = 0; i < N; i++) {
    if (qpos) for (int k = 0; k < NQ; k++) {
      const float hi = (float)qpos[i * NQ + k];
      hq[i * NQP + k] = hi;
      hf[i * QFINE_ROW + qfine_of_q(k)] = (float)(qpos[i * NQ + k] - (double)hi);
    }
    if (qvel) for (int k = 0; k < NV; k++) {
      const float hi = (float)qvel[i * NV + k];
      hv[i * NVP + k] = hi;
      hf[i * QFINE_ROW + qfine_of_v(k)] = (float)(qvel[i * NV + k] - (double)hi);
    }
  }
  rc = store(e, e->qpos, hq);
  if (!rc) rc = store(e, e->qvel, hv);
  if (!rc) rc = store(e, e->qfine, hf);
  return rc;
}
// physics.data.time (models/robot_arm.py:68-69): physics steps since the last mre_reset times the timestep, per env
// (envs differ after PropPlacer's settle, whose exit is per env).  Host pointer [N].
extern "C" int mre_get_time(mre_env* e, double* time) {
  ENTER(e, time, "mre_get_time: null", DRAIN_FIRST);
  std::vector<int> hn;
  int rc = fetch(e, e->nstep, (size_t)e->N, hn);
  if (rc) return rc;
  for (int i = 0; i < e->N; i++) time[i] = (double)hn[i] * (double)e->hM.opt_rec.timestep;
  return MRE_OK;
}
extern "C" int mre_get_ctrl(mre_env* e, float* ctrl) {
  ENTER(e, ctrl, "mre_get_ctrl: null", DRAIN_FIRST);
  return copy_out(e, ctrl, e->ctrl, (size_t)e->N * NU * 4);
}

extern "C" int mre_get_state(mre_env* e, float* qpos, float* qvel) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  int rc = MRE_OK;
  if (qpos) rc = copy_out(e, qpos, e->qpos, (size_t)e->N * NQP * 4);
  if (!rc && qvel) rc = copy_out(e, qvel, e->qvel, (size_t)e->N * NVP * 4);
  return rc;
}
// final (qpos, qvel, status) rows of every env, packed on the device: out[N][MRE_FINAL_W] (device pointer), enqueued on
// the handle's stream -- the local block of the end-of-rollout all_gather (bench.py, distributed.py)
extern "C" int mre_pack_final_state(mre_env* e, float* out) {
  ENTER(e, out, "null", DRAIN_FIRST);
  if (!is_device_ptr(out)) return fail(MRE_ERR_ARG, "mre_pack_final_state: out must be a device pointer");
  mre_launch_pack_final(e->N, e->qpos, e->qvel, e->status, out, e->stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}
// mj_jacSite / mj_fullM / qfrc_bias of the arm on the current state, packed per env by k_arm_dynamics: out[N][MRE_DYN_W]
// (device pointer), enqueued on the handle's stream.  One kernel for every handle: the rows do not depend on the solver.
extern "C" int mre_get_arm_dynamics(mre_env* e, int site, float* out) {
  ENTER(e, out, "mre_get_arm_dynamics: null", DRAIN_FIRST);
  if (site != 0 && site != 1) return fail(MRE_ERR_ARG, "mre_get_arm_dynamics: site must be 0 (controller site) or 1 (pinch site)");
  if (!is_device_ptr(out) || ((uintptr_t)out & 7))
    return fail(MRE_ERR_ARG, "mre_get_arm_dynamics: out must be a device pointer, 8-byte aligned");
  DynArgs a;
  memset(&a, 0, sizeof(a));
  a.M = e->dM; a.N = e->N; a.qpos = e->qpos; a.qvel = e->qvel; a.qfine = e->qfine; a.nprops = e->nprops;
  a.prop_size = e->prop_size; a.site = site; a.out = out;
  mre_launch_arm_dynamics(&a, e->stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}
extern "C" int mre_set_warmstart(mre_env* e, const float* w) {
  ENTER(e, w, "null", DRAIN_FIRST);
  return copy_in(e, e->qacc_ws, w, (size_t)e->N * NVP * 4);
}
extern "C" int mre_get_warmstart(mre_env* e, float* w) {
  ENTER(e, w, "null", DRAIN_FIRST);
  return copy_out(e, w, e->qacc_ws, (size_t)e->N * NVP * 4);
}
extern "C" int mre_set_ctrl(mre_env* e, const float* ctrl) {
  ENTER(e, ctrl, "null", DRAIN_FIRST);
  return copy_in(e, e->ctrl, ctrl, (size_t)e->N * NU * 4);
}

extern "C" int mre_step(mre_env* e, int nsubsteps, unsigned flags) {
  ENTER(e, nsubsteps >= 0, "mre_step: bad argument", LEAVE_PENDING);
  StepArgs a;
  fill_args(e, a);
  a.nsteps = nsubsteps; a.flags |= flags;
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
  ENTER(e, ctrl_seq && nticks >= 0 && control_steps >= 1, "mre_rollout: bad argument", LEAVE_PENDING);
  if (!is_device_ptr(ctrl_seq)) return fail(MRE_ERR_ARG, "mre_rollout: ctrl_seq must be a device pointer");
  int per = (ticks_per_launch <= 0 || ticks_per_launch > nticks) ? nticks : ticks_per_launch;
  bool allow_queue = ticks_per_launch >= 2;   // the caller's cut into launches of several ticks: queue launches where they apply
  // the library's choice (ticks_per_launch <= 0) for a batch that does not fit the GPU's wave slots: queue launches
  if (ticks_per_launch <= 0 && policy::queue_fits(e->queue_ok, e->queue_waves, e->N) && nticks >= 2) {
    if (policy::window_wants_queue(nticks, e->queue_min_ticks, e->tick_tail_valid, e->tick_tail, e->queue_tail_min)) {
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
      e->seq_cap = 0;
      for (float*& p : e->seq_copy) { release(e, &p); int rc = alloc_dev(e, &p, n * 4); if (rc) return rc; }
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
    a.ctrl_seq = src + (size_t)t0 * (size_t)e->N * NU; a.flags |= flags;
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
  ENTER(e, true, "null handle", DRAIN_FIRST);
  if (out) {
    if (!is_device_ptr(out)) return fail(MRE_ERR_ARG, "mre_set_trace: trace buffer must be a device pointer");
    if (nenv <= 0 || nenv > e->N || max_steps <= 0) return fail(MRE_ERR_ARG, "mre_set_trace: bad sizes");
  }
  e->trace = out; e->trace_nenv = out ? nenv : 0; e->trace_max = out ? max_steps : 0; e->trace_pos = 0;
  return MRE_OK;
}

extern "C" int mre_osc_configure(mre_env* e, const float* gains, const float* null_q, const float* thr,
                                 int pinv_always) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  if (gains) {
    e->osc.kp_pos = gains[0]; e->osc.kd_pos = gains[1]; e->osc.kp_ori = gains[2];
    e->osc.kd_ori = gains[3]; e->osc.kp_null = gains[4]; e->osc.kd_null = gains[5];
  }
  if (null_q) for (int k = 0; k < 7; k++) e->osc.null_q[k] = null_q[k];
  if (thr) { e->osc.pos_thresh = thr[0]; e->osc.ori_thresh = thr[1]; }
  e->osc.pinv_always = pinv_always;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->d_osc, &e->osc, sizeof(OscConfig), hipMemcpyHostToDevice));
  release(e, &e->d_osc_env);
  return MRE_OK;
}

// per-env controller parameters (a population of gain sets, one per env): any NULL array keeps the
// shared configuration's values; mre_osc_configure afterwards returns to one shared set
extern "C" int mre_osc_configure_env(mre_env* e, const float* gains, const float* null_q, const float* thr) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
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
  int rc = alloc_dev(e, &e->d_osc_env, N * sizeof(OscConfig));
  if (rc) return rc;
  HIPCHK(hipMemcpy(e->d_osc_env, h.data(), N * sizeof(OscConfig), hipMemcpyHostToDevice));
  return MRE_OK;
}

extern "C" int mre_gripper_set(mre_env* e, const uint8_t* closed) {
  ENTER(e, closed, "null", DRAIN_FIRST);
  return copy_in(e, e->grip_closed, closed, (size_t)e->N);
}

extern "C" int mre_get_sites(mre_env* e, float* tcp_pos, float* eef_pose, float* prop_pose) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  // refresh site poses for the current state (0 physics steps = kinematics only)
  StepArgs a;
  fill_args(e, a);
  int rc = zero_step(e, a);
  if (rc) return rc;
  const size_t N = (size_t)e->N;
  std::vector<float> hs, hq;
  if ((rc = fetch(e, e->sites, N * 16, hs))) return rc;
  if (prop_pose && (rc = fetch(e, e->qpos, N * NQP, hq))) return rc;
  // gather on the host into temporaries, then copy to the (host or device) destinations
  std::vector<float> t3(N * 3), t7(N * 7), tp(N * NPROP * 7);
  for (size_t i = 0; i < N; i++) {
    for (int k = 0; k < 3; k++) t3[i * 3 + k] = hs[i * 16 + k];
    for (int k = 0; k < 7; k++) t7[i * 7 + k] = hs[i * 16 + 3 + k];
    if (prop_pose)
      for (int p = 0; p < NPROP; p++)
        for (int k = 0; k < 7; k++) tp[(i * NPROP + p) * 7 + k] = hq[i * NQP + NRV + 7 * p + k];
  }
  if (tcp_pos && (rc = store(e, tcp_pos, t3))) return rc;
  if (eef_pose && (rc = store(e, eef_pose, t7))) return rc;
  if (prop_pose && (rc = store(e, prop_pose, tp))) return rc;
  return MRE_OK;
}

extern "C" int mre_get_status(mre_env* e, uint32_t* status) {
  ENTER(e, status, "null", DRAIN_FIRST);
  return copy_out(e, status, e->status, (size_t)e->N * 4);
}
extern "C" int mre_get_solver_stats(mre_env* e, int32_t* stats) {
  ENTER(e, stats, "null", DRAIN_FIRST);
  return copy_out(e, stats, e->stats, (size_t)e->N * 16);
}

extern "C" int mre_osc_set_target(mre_env* e, const float* pos, const float* quat, const float* vel,
                                  const float* angvel, const uint8_t* mask) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  // small host-side merge: targets persist per env, NULL keeps the old value
  const size_t N = (size_t)e->N;
  std::vector<float> hp, hq, hv, hw;
  std::vector<uint8_t> hm;
  int rc;
  if ((pos && (rc = fetch(e, pos, N * 3, hp))) || (quat && (rc = fetch(e, quat, N * 4, hq))) ||
      (vel && (rc = fetch(e, vel, N * 3, hv))) || (angvel && (rc = fetch(e, angvel, N * 3, hw))) ||
      (mask && (rc = fetch(e, mask, N, hm))))
    return rc;
  return patch_rows(e, e->osc_target, 16, [&](size_t i) { return !mask || hm[i]; }, [&](size_t i, float* r) {
    if (pos) for (int k = 0; k < 3; k++) r[k] = hp[i * 3 + k];
    if (quat) for (int k = 0; k < 4; k++) r[3 + k] = hq[i * 4 + k];
    if (vel) for (int k = 0; k < 3; k++) r[7 + k] = hv[i * 3 + k];
    if (angvel) for (int k = 0; k < 3; k++) r[10 + k] = hw[i * 3 + k];
  });
}

extern "C" int mre_run_controller(mre_env* e, int nticks, int control_steps, uint8_t* converged_out) {
  ENTER(e, nticks >= 0 && control_steps >= 1, "mre_run_controller: bad argument", LEAVE_PENDING);
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
    queue = policy::queue_fits(e->queue_ok, e->queue_waves, e->N) && !e->compact_only && !e->use_order &&
            policy::window_wants_queue(nticks, e->queue_min_ticks, e->tick_tail_valid, e->tick_tail, e->queue_tail_min);
    if (queue) chunk = e->queue_run_ticks;
    if (const char* c = getenv("MRE_RUN_CHUNK")) { const int v = atoi(c); chunk = v > 0 ? v : nticks; }  // tuning knob
  }
  if (chunk <= 0 || chunk > nticks) chunk = nticks;
  if (queue && chunk > QUEUE_TICKS_MAX) chunk = QUEUE_TICKS_MAX;
  DRAIN(e);   // (after the cut is chosen: the drain updates what the cut is chosen by)
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
  ENTER(e, true, "null handle", DRAIN_FIRST);
  StepArgs a;
  fill_args(e, a);
  a.mode = CTRL_OSC; a.flags |= F_OSC_EVAL;
  int rc = zero_step(e, a);
  if (rc) return rc;
  const size_t N = (size_t)e->N;
  std::vector<float> h;
  if ((rc = fetch(e, e->ctrl, N * NU, h))) return rc;
  std::vector<float> ht(N * 7), hg(N);
  for (size_t i = 0; i < N; i++) {
    for (int k = 0; k < 7; k++) ht[i * 7 + k] = h[i * NU + k];
    hg[i] = h[i * NU + 7];
  }
  if (tau && (rc = store(e, tau, ht))) return rc;
  if (grip && (rc = store(e, grip, hg))) return rc;
  return MRE_OK;
}

// ---- device buffers and launch arguments of k_pose_search (mre_place_props, mre_prop_place, mre_sort_colours)
static int search_buffers(mre_env* e) {
  const size_t N = (size_t)e->N;
  int rc;
  if ((rc = alloc_dev(e, &e->ps_attempts, N * 4)) || (rc = alloc_dev(e, &e->ps_prop, N * 4)) ||
      (rc = alloc_dev(e, &e->ps_tick, N * 4)) || (rc = alloc_dev(e, &e->ps_which, N * 4)) ||
      (rc = alloc_dev(e, &e->ps_bounds, N * 6 * 8)) || (rc = alloc_dev(e, &e->ps_pose, N * 7 * 8)) ||
      (rc = alloc_dev(e, &e->ps_zones, N * NPROP * 4 * 8)) || (rc = alloc_dev(e, &e->ps_pick, N * 7 * 8)))
    return rc;
  return MRE_OK;
}
static void fill_search(mre_env* e, SearchArgs& sa) {
  memset(&sa, 0, sizeof(sa));
  sa.M = e->dM; sa.N = e->N; sa.qpos = e->qpos; sa.qfine = e->qfine; sa.nprops = e->nprops; sa.prop_size = e->prop_size;
  sa.env_ids = e->d_env_ids; sa.env_id_offset = e->env_id_offset;
  sa.attempts = e->ps_attempts; sa.fixed_prop = -1; sa.flags = e->base_flags;
}

// physics.forward() + physics.data.contact on the current poses: one zero-step launch that runs the
// kinematics and the narrow phase and exports every DETECTED contact (dist < margin), per env
// [count, (geom1, geom2, dist) x CONTACT_EXPORT]; count < 0: the list was cut at -count.
static int detect_contacts(mre_env* e, const uint8_t* dmask, bool full = false, bool active_only = false) {
  const size_t N = (size_t)e->N, row = 1 + 3 * CONTACT_EXPORT;
  int rc = alloc_dev(e, &e->contacts, N * row * 4);
  if (!rc && full) rc = alloc_dev(e, &e->contacts_full, N * CONTACT_EXPORT * 12 * 4);
  if (rc) return rc;
  StepArgs a;
  fill_args(e, a);
  a.flags |= F_DETECT | (active_only ? F_DETECT_ACTIVE : 0u); a.env_mask = dmask;
  a.contacts = e->contacts; a.contacts_full = full ? e->contacts_full : nullptr;
  a.sites = nullptr; a.geoms = nullptr;
  return zero_step(e, a);
}

extern "C" int mre_get_contacts(mre_env* e, int32_t* count, float* contacts) {
  ENTER(e, count && contacts, "mre_get_contacts: null", DRAIN_FIRST);
  int rc = detect_contacts(e, nullptr);
  if (rc) return rc;
  const size_t N = (size_t)e->N, row = 1 + 3 * CONTACT_EXPORT;
  std::vector<float> h;
  if ((rc = fetch(e, e->contacts, N * row, h))) return rc;
  std::vector<int32_t> hc(N);
  std::vector<float> ho(N * 3 * CONTACT_EXPORT);
  for (size_t i = 0; i < N; i++) {
    hc[i] = (int32_t)h[i * row];
    memcpy(&ho[i * 3 * CONTACT_EXPORT], &h[i * row + 1], 3 * CONTACT_EXPORT * 4);
  }
  if ((rc = store(e, count, hc))) return rc;
  return store(e, contacts, ho);
}

// The whole mjContact record of the same zero-step launch: rows of 15 = pos[3], frame[9], dist, geom1, geom2.
// active_only: the launch runs collide(.., detect = false), the call every step makes -- its early-outs see
// margin - gap, not margin, so this list is what the next solve would be given, not a filtered copy of the other.
extern "C" int mre_get_contacts_full(mre_env* e, int active_only, int32_t* count, float* contacts) {
  ENTER(e, count && contacts, "mre_get_contacts_full: null", DRAIN_FIRST);
  int rc = detect_contacts(e, nullptr, true, active_only != 0);
  if (rc) return rc;
  const size_t N = (size_t)e->N, row = 1 + 3 * CONTACT_EXPORT, W = 15;
  std::vector<float> h, hf;
  if ((rc = fetch(e, e->contacts, N * row, h)) || (rc = fetch(e, e->contacts_full, N * CONTACT_EXPORT * 12, hf))) return rc;
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
  if ((rc = store(e, count, hc))) return rc;
  return store(e, contacts, ho);
}

// ---- PropPlacer.__call__, in parts.  What one mre_place_props call keeps on the host between them:
struct Placement {
  std::vector<uint8_t> todo;     // envs whose cubes are (still) to be placed
  std::vector<uint8_t> failed;   // no pose within max_attempts for one of the env's cubes
  std::vector<int> nprops;       // cubes per env
  std::vector<int> clock;        // nstep of every env when the current round began
  bool any_todo() const { return std::any_of(todo.begin(), todo.end(), [](uint8_t t) { return t != 0; }); }
};

// A round begins: the clock is noted, the cubes of the envs to place go to their parking poses (float32 values: the
// low-order words of the cubes' poses and velocities are zero) and, from the second round on, come to rest.
static int place_park(mre_env* e, Placement& P, int round) {
  const auto todo = [&](size_t i) { return P.todo[i] != 0; };
  int rc = fetch(e, e->nstep, (size_t)e->N, P.clock);
  if (rc) return rc;
  rc = patch_rows(e, e->qpos, NQP, todo, [&](size_t, float* row) {
    for (int p = 0; p < NPROP; p++) {
      float* q = row + NRV + 7 * p;
      for (int k = 0; k < 3; k++) q[k] = e->hM.park_pos[p][k];
      q[3] = 1.f; q[4] = q[5] = q[6] = 0.f;
    }
  });
  if (!rc) rc = store(e, e->mask, P.todo);
  if (!rc) rc = patch_rows(e, e->qfine, QFINE_ROW, todo, [](size_t, float* row) { for (int k = QFINE_CUBE_Q; k < QFINE_ROW; k++) row[k] = 0.f; });
  if (!rc && round > 0)   // a second try starts from rest
    rc = patch_rows(e, e->qvel, NVP, todo, [](size_t, float* row) { for (int k = NRV; k < NVP; k++) row[k] = 0.f; });
  return rc;
}

// one search launch per prop index: every env that still needs prop p runs its own attempt loop on
// the device (k_pose_search) and writes the accepted pose into its qpos row
static int place_search(mre_env* e, Placement& P, int round, uint64_t seed, const float* ws_min, const float* ws_max, int max_attempts) {
  const size_t N = (size_t)e->N;
  std::vector<int> att;
  for (int p = 0; p < NPROP; p++) {
    SearchArgs sa;
    fill_search(e, sa);
    sa.env_mask = e->mask; sa.seed = seed; sa.fixed_prop = p;
    for (int k = 0; k < 3; k++) { sa.shared_bounds[k] = ws_min[k]; sa.shared_bounds[3 + k] = ws_max[k]; }
    sa.tick0 = ((long long)round * NPROP + p) * (long long)max_attempts;
    sa.max_attempts = max_attempts; sa.yaw_mode = 1; sa.max_dist = INFINITY; sa.commit = 1;
    mre_launch_pose_search(&sa, e->stream);
    HIPCHK(hipGetLastError());
    int rc = fetch(e, e->ps_attempts, N, att);
    if (rc) return rc;
    bool dropped = false;
    for (size_t i = 0; i < N; i++)
      if (P.todo[i] && p < P.nprops[i] && att[i] <= 0) { P.failed[i] = 1; P.todo[i] = 0; dropped = true; }
    // (_REJECTION_SAMPLING_FAILED is an exception of ONE env in the reference: here that env is flagged
    //  MRE_ST_PLACEMENT_FAILED, its remaining cubes stay parked, and the other envs carry on)
    if (dropped && (rc = store(e, e->mask, P.todo))) return rc;
  }
  return MRE_OK;
}

// The physics settles with the robot frozen, every env leaving by itself; the envs that came to rest are done.
// *settled_now: how many did.
static int place_settle(mre_env* e, Placement& P, int round, int settle_steps, int* settled_now) {
  const size_t N = (size_t)e->N;
  StepArgs a;
  fill_args(e, a);
  a.trace = nullptr;
  // _max_settle_physics_time = 2 s; min time = settle_steps * dt (0.3 s in the reference)
  a.nsteps = (int)std::lround(2.0 / e->hM.opt_rec.timestep);
  if (a.nsteps < settle_steps) a.nsteps = settle_steps;
  a.flags |= F_FREEZE_ROBOT | F_SETTLE_EXIT; a.env_mask = e->mask;
  a.settle_steps = e->settle_steps; a.min_settle_steps = settle_steps;
  const bool prof = e->profiling;
  e->profiling = false;  // setup, not a control tick
  int rc = launch_step(e, a, /*settle=*/true);
  e->profiling = prof;
  if (rc) return rc;
  std::vector<int> hs;
  if ((rc = fetch(e, e->settle_steps, N, hs))) return rc;
  if (getenv("MRE_DEBUG_PLACE")) {
    int nt = 0, ns = 0;
    for (size_t i = 0; i < N; i++) if (P.todo[i]) { nt++; ns += hs[i] >= 0; }
    fprintf(stderr, "mre_place_props round %d: %d envs placed, %d settled\n", round, nt, ns);
  }
  *settled_now = 0;
  for (size_t i = 0; i < N; i++) {
    if (!P.todo[i]) continue;
    const int n = hs[i] < 0 ? -hs[i] : hs[i];
    if (n > e->last_settle_max) e->last_settle_max = n;
    if (hs[i] >= 0) { P.todo[i] = 0; (*settled_now)++; }               // settled
  }
  return MRE_OK;
}

// `physics.data.time = original_time` after EVERY failed attempt, the last one included
// (prop_initializer.py:240-258): the clock goes back for every env that did not settle in this round
static int place_rewind(mre_env* e, const Placement& P) {
  if (!P.any_todo()) return MRE_OK;
  return patch_rows(e, e->nstep, 1, [&](size_t i) { return P.todo[i] != 0; }, [&](size_t i, int* n) { *n = P.clock[i]; });
}

// status: envs that never settled (the reference logs _SETTLING_PHYSICS_FAILED and goes on), envs without a pose
static int place_flag(mre_env* e, const Placement& P, bool settling) {
  const auto flagged = [&](size_t i) { return P.failed[i] || (settling && P.todo[i]); };
  bool any = false;
  for (size_t i = 0; i < (size_t)e->N; i++) any = any || flagged(i);
  if (!any) return MRE_OK;
  return patch_rows(e, e->status, 1, flagged, [&](size_t i, uint32_t* st) {
    *st |= P.failed[i] ? MRE_ST_PLACEMENT_FAILED : MRE_ST_NOT_SETTLED;
  });
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
  ENTER(e, ws_min && ws_max && max_attempts >= 1, "mre_place_props: bad argument", DRAIN_FIRST);
  const size_t N = (size_t)e->N;
  Placement P;
  P.todo.assign(N, 1);
  P.failed.assign(N, 0);
  int rc;
  if (mask && (rc = fetch(e, mask, N, P.todo))) return rc;
  if ((rc = fetch(e, e->nprops, N, P.nprops)) || (rc = search_buffers(e))) return rc;
  if (settle_steps > 0) {
    if ((rc = alloc_dev(e, &e->settle_steps, N * 4))) return rc;
    HIPCHK(hipMemsetAsync(e->settle_steps, 0, N * 4, e->stream));
  }
  e->last_settle_max = 0;
  // PropPlacer.place_and_settle (environment/prop_initializer.py:240-258): place, settle with the robot frozen,
  // and place AGAIN the envs whose cubes are still moving after max_settle_physics_time -- up to
  // max_settle_physics_attempts (10) times, per env (the other envs keep what they have)
  const int max_settle_attempts = settle_steps > 0 ? 10 : 1;
  for (int round = 0; round < max_settle_attempts && P.any_todo(); round++) {
    if ((rc = place_park(e, P, round)) || (rc = place_search(e, P, round, seed, ws_min, ws_max, max_attempts))) return rc;
    if (settle_steps <= 0) break;
    int settled_now = 0;
    if ((rc = place_settle(e, P, round, settle_steps, &settled_now))) return rc;
    // a round in which NO env came to rest is not bad luck of a placement but the solver: PGS at 100 sweeps leaves a
    // friction creep of 1e-3 rad/s on resting cubes that never passes the velocity test (all 4096 envs of the bench,
    // in every one of ten rounds; with Newton all settle in the first).  Placing again cannot help: stop, flag them
    // (only where that diagnosis can hold: PGS, a batch large enough that "none of them" is not chance, first round;
    //  a lone env keeps its ten attempts like the reference's)
    const bool give_up = settled_now == 0 && round == 0 && N >= 64 && e->solver != MRE_SOLVER_NEWTON;
    if ((rc = place_rewind(e, P))) return rc;
    if (give_up) break;
  }
  return place_flag(e, P, settle_steps > 0);
}

extern "C" int mre_get_settle_steps(mre_env* e, int32_t* steps) {
  ENTER(e, steps, "mre_get_settle_steps: null", DRAIN_FIRST);
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
  ENTER(e, prop && bounds && tick && pose && attempts && max_attempts >= 1, "mre_prop_place: bad argument", DRAIN_FIRST);
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
  ENTER(e, call_counts && zones && which && pick && place && attempts && max_attempts >= 1, "mre_sort_colours: bad argument",
        DRAIN_FIRST);
  const size_t N = (size_t)e->N;
  int rc = search_buffers(e);
  if (rc) return rc;
  std::vector<int32_t> ticks;
  if ((rc = fetch(e, call_counts, N, ticks))) return rc;
  for (size_t i = 0; i < N; i++) ticks[i] *= 10000;   // MAX_PLACE_ATTEMPTS draws reserved per call
  if ((rc = store(e, e->ps_tick, ticks)) || (rc = copy_in(e, e->ps_zones, zones, N * NPROP * 32))) return rc;
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
  ENTER(e, info, "mre_get_launch_info: null", DRAIN_FIRST);
  HIPCHK(hipStreamSynchronize(e->stream));
  return copy_out(e, info, e->h_info_last, (size_t)e->N * 16);
}

extern "C" int mre_set_env_ids(mre_env* e, const long long* ids) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  if (ids) e->env_ids.assign(ids, ids + e->N); else e->env_ids.clear();
  release(e, &e->d_env_ids);
  if (!ids) return MRE_OK;
  int rc = alloc_dev(e, &e->d_env_ids, (size_t)e->N * 8);
  return rc ? rc : copy_in(e, e->d_env_ids, e->env_ids.data(), (size_t)e->N * 8);   // (env_ids lives as long as the handle)
}

extern "C" int mre_set_env_id_offset(mre_env* e, long long offset) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  e->env_ids.clear();
  release(e, &e->d_env_ids);
  e->env_id_offset = offset;
  return MRE_OK;
}

extern "C" int mre_profile_enable(mre_env* e, int on) {
  ENTER(e, true, "null handle", DRAIN_FIRST);
  e->profiling = on != 0;
  e->events_used = 0;
  return MRE_OK;
}
extern "C" int mre_profile_read(mre_env* e, float* total_ms, int* launches) {
  ENTER(e, total_ms && launches, "null", DRAIN_FIRST);
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
  ENTER(e, true, "null handle", DRAIN_FIRST);
  if (!order) { e->use_order = false; return MRE_OK; }
  int rc = copy_in(e, e->order, order, (size_t)e->N * 4);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  e->use_order = true;
  return MRE_OK;
}

// mre_launch.h -- the host's view of the kernel launchers that the .hip units define (extern "C", one per kernel
// instantiation), and the solver's choice among the step kernel's.  Host side only: the .hip units do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mre.h"
#include "mre_dev.h"

extern "C" {
void mre_launch_step(const mre::StepArgs* args, hipStream_t stream);
void mre_launch_settle(const mre::StepArgs* args, hipStream_t stream);
void mre_launch_step_large(const mre::StepArgs* args, hipStream_t stream);
void mre_launch_step_queue(const mre::StepArgs* args, int nwaves, hipStream_t stream);
void mre_launch_step_queue_large(const mre::StepArgs* args, int nwaves, hipStream_t stream);
int mre_queue_waves_per_cu(void);
void mre_launch_step_newton(const mre::StepArgs* args, hipStream_t stream);
void mre_launch_settle_newton(const mre::StepArgs* args, hipStream_t stream);
void mre_launch_step_large_newton(const mre::StepArgs* args, hipStream_t stream);
void mre_launch_step_queue_newton(const mre::StepArgs* args, int nwaves, hipStream_t stream);
void mre_launch_step_queue_large_newton(const mre::StepArgs* args, int nwaves, hipStream_t stream);
int mre_queue_waves_per_cu_newton(void);
void mre_launch_render(const mre::RenderArgs* args, int row_groups, hipStream_t stream);
void mre_launch_pack_final(int N, const float* qpos, const float* qvel, const uint32_t* status, float* out, hipStream_t stream);
void mre_launch_restore_rows(const uint8_t* sel, int env0, int N, float* qpos, const float* sv_qpos, float* qvel,
                             const float* sv_qvel, float* qacc_ws, const float* sv_qacc_ws, float* qfine, const float* sv_qfine,
                             float* ctrl, const float* sv_ctrl, int* nstep, const int* sv_nstep, uint32_t* status,
                             const uint32_t* sv_status, uint8_t* converged, const uint8_t* sv_converged, uint8_t* pending,
                             hipStream_t stream);
void mre_launch_pose_search(const mre::SearchArgs* args, hipStream_t stream);
void mre_launch_sort_select(const mre::SortArgs* args, hipStream_t stream);
void mre_launch_arm_dynamics(const mre::DynArgs* args, hipStream_t stream);
void mre_launch_reset(const mre::DevModel* M, int N, float* qpos, float* qvel, float* qacc_ws, float* qfine, float* ctrl,
                      uint32_t* status, int* nstep, const uint8_t* mask, hipStream_t stream);
}

namespace mre {

// solver-specific instantiations of the step kernel (opt_solver of the model, mre_set_solver)
struct StepKernels {
  void (*step)(const StepArgs*, hipStream_t), (*settle)(const StepArgs*, hipStream_t), (*large)(const StepArgs*, hipStream_t);
  void (*queue)(const StepArgs*, int nwaves, hipStream_t), (*queue_large)(const StepArgs*, int nwaves, hipStream_t);
  int (*queue_waves_per_cu)(void);
};
inline const StepKernels& step_kernels(int solver) {
  static const StepKernels table[2] = {
      {mre_launch_step, mre_launch_settle, mre_launch_step_large, mre_launch_step_queue, mre_launch_step_queue_large,
       mre_queue_waves_per_cu},
      {mre_launch_step_newton, mre_launch_settle_newton, mre_launch_step_large_newton, mre_launch_step_queue_newton,
       mre_launch_step_queue_large_newton, mre_queue_waves_per_cu_newton}};
  return table[solver == MRE_SOLVER_NEWTON];
}

}  // namespace mre

// What is literally the same in the two Transporter heads on the device: the place head (csrc/mre_correlate.hip,
// mre_correlate_grad.hip) and the pick head (csrc/mre_attend.hip).  Each head keeps its own softmax merge, order of merging
// slots and per-lane accumulation: they decide the last bit of its outputs (soft_merge, acc_merge and the slot kernels say how
// they differ).  Small structs go by VALUE: by reference the compiler has kept a branch chain and a register more (DESIGN.md
// 8f, "One scan for both kernels").  NOT part of lib.source_hash(): nothing here is launched by the step or the camera.
#ifndef MRE_HEAD_H
#define MRE_HEAD_H
#include <hip/hip_runtime.h>

#include "mre_warp_input_point.h"

namespace {

constexpr float L2E = 1.44269504088896340736f;
constexpr int NO_INDEX = 0x7FFFFFFF;
constexpr uint32_t MAX_GRID_Y = 65535, MAX_GRID = 1u << 20;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// `better` is a total order on (value, index) -- greater value, then lower index -- so a reduction gives the first occurrence
// of the maximum in whatever order it combines; a NaN is never better than anything.
__device__ __forceinline__ bool better(float v2, int i2, float v1, int i1) { return v2 > v1 || (v2 == v1 && i2 < i1); }

struct Best { float v; int i; };   // (-inf, NO_INDEX) is the empty set

__device__ __forceinline__ Best best_merge(Best a, Best b) { return better(b.v, b.i, a.v, a.i) ? b : a; }

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float v = __shfl_xor(b.v, m, 64);
    const int i = __shfl_xor(b.i, m, 64);
    if (better(v, i, b.v, b.i)) { b.v = v; b.i = i; }
  }
  return b;
}

struct Soft { float m, s; };   // max and sum of exp(l - max); (-inf, 0) is the empty set.  Each head has its own merge.

// The finish of a softmax from its (max, sum): lse, the target's logit `tl` and the loss; NaN for a target outside [0, cells)
struct SoftEnd { float lse, target_logit, loss; };

__device__ __forceinline__ bool soft_inside(int64_t tgt, int64_t cells) { return tgt >= 0 && tgt < cells; }

__device__ __forceinline__ SoftEnd soft_finish(Soft b, int64_t tgt, int64_t cells, float tl) {
  const float lse = b.m + logf(b.s);
  const float t = soft_inside(tgt, cells) ? tl : __builtin_nanf("");
  return SoftEnd{lse, t, lse - t};
}

// one workgroup per (x, env): blockIdx.x is x, y and z the env (at most 65 535 in y; n < 2^31 envs)
__device__ __forceinline__ uint32_t env_index(void) { return blockIdx.z * gridDim.y + blockIdx.y; }

inline dim3 env_grid(uint32_t x, uint32_t n) {
  const uint32_t gy = n < MAX_GRID_Y ? n : MAX_GRID_Y;
  return dim3(x, gy, (n + gy - 1) / gy);
}

// one wave per env, the envs strided over the grid
inline dim3 wave_per_env_grid(uint32_t n) { return dim3(n < MAX_GRID ? n : MAX_GRID); }

}  // namespace
#endif

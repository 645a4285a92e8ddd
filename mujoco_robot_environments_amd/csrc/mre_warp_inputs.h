// Network-ready inputs on the device (csrc/mre_warp_inputs.hip): the nearest-neighbour affine gather of mre_warp_maps
// written as a planar, per-channel normalised float32 or bfloat16 tensor -- what a convolution consumes.
// Shared between the kernel's translation unit and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here
// is launched by the step or the camera.
#ifndef MRE_WARP_INPUTS_H
#define MRE_WARP_INPUTS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mre_warp.h"
#include "mre_warp_input_point.h"

constexpr int WI_MAX_CHANNELS = 8;
constexpr uint32_t WI_SRC_HEIGHT = 3;   // MRE_SRC_HEIGHT (include/mre.h); 0, 1, 2: the colour bytes

// The channel table travels by value: it is the same in every lane, so it lives in SGPRs.
struct WarpInputArgs {
  WarpSource source;     // cmap: read only when a colour source is named, null otherwise
  uint32_t vec;          // out_w % 4 == 0 and out aligned for a lane's 4 elements of every channel plane
  uint32_t colour;       // a channel reads a colour byte
  uint32_t bf16;         // out holds bfloat16, else float32
  uint32_t channels;     // 1 .. WI_MAX_CHANNELS
  uint32_t src[WI_MAX_CHANNELS];
  float scale[WI_MAX_CHANNELS], bias[WI_MAX_CHANNELS];
  void* out;             // [samples][channels][out_h][out_w]
};

// one launch on `stream`; every element of out is written exactly once
extern "C" void mre_launch_warp_inputs(const WarpInputArgs* a, hipStream_t stream);
#endif

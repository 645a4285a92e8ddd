// Warped and cropped maps on the device (csrc/mre_warp.hip): a nearest-neighbour affine gather of the height, colour and
// label maps of mre_heightmap -- the SE(2) perturbation and the rotated pick crops of a Transporter training sample.
// Shared between the kernel's translation unit and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here
// is launched by the step or the camera.
#ifndef MRE_WARP_H
#define MRE_WARP_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mre_warp_point.h"

constexpr int WP_TILE_H = 16;                // rows of a workgroup's tile
constexpr int WP_TILE_W = 64;                // columns of it: 16 lanes x 4 consecutive columns
constexpr uint32_t WP_MAX_DIM = 4096;        // rows / columns of a source or output map at most
constexpr uint32_t WP_MAX_GRID = 1u << 20;   // workgroups of a launch at most; work items beyond are looped over

// What the map warp and the network inputs (csrc/mre_warp_inputs.h) gather from, and the shape of what they gather into:
// filled once by the C ABI, read by the one statement of the gather (csrc/mre_warp_gather.h).
struct WarpSource {
  const float* hmap;     // [n][in_h][in_w]
  const uint8_t* cmap;   // [n][in_h][in_w][3] or null
  const int32_t* index;  // [samples] or null (sample s reads map s)
  const float* mats;     // [samples][6]
  uint32_t n, in_h, in_w;
  uint32_t samples, out_h, out_w, tiles_x, tiles_y;
};

struct WarpArgs {
  WarpSource source;
  const uint8_t* smap;   // [n][in_h][in_w] or null
  uint32_t vec;          // out_w % 4 == 0 and every output base aligned for the wide stores
  float* out_h_;         // [samples][out_h][out_w]
  uint8_t* out_c;        // [samples][out_h][out_w][3] or null (with cmap)
  uint8_t* out_s;        // [samples][out_h][out_w] or null (with smap)
  int32_t* from;         // [samples][out_h][out_w] or null
};

// one launch on `stream`; every element of every non-null output is written exactly once
extern "C" void mre_launch_warp_maps(const WarpArgs* a, hipStream_t stream);
#endif

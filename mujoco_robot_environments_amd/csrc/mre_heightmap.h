// Orthographic heightmaps on the device (csrc/mre_heightmap.hip): the camera's depth / rgb / seg frames of every env
// binned top-down into a height map, a colour map, a label map and the source pixel of every cell.  Shared between the
// kernel's translation unit and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here is launched by the
// step or the camera.
#ifndef MRE_HEIGHTMAP_H
#define MRE_HEIGHTMAP_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mre_heightmap_point.h"

#ifndef MRE_HM_TILE
#define MRE_HM_TILE 64   // cells per side of a workgroup's tile: 32 KB of 64-bit keys in LDS (32: 8 KB, measured slower
                         // at the camera's frame because the tiles' source rectangles overlap more: DESIGN.md 8f.5)
#endif
constexpr int HM_TILE = MRE_HM_TILE;
constexpr uint32_t HM_MAX_OUT = 4096;        // rows / columns of a map at most
constexpr uint32_t HM_MAX_GRID = 1u << 20;   // workgroups of a launch at most; work items beyond are looped over

struct HeightmapArgs {
  const float* depth;    // [n][h][w]
  const uint8_t* rgb;    // [n][h][w][3] or null
  const uint8_t* seg;    // [n][h][w] or null
  uint32_t n, h, w;      // h * w < 2^31
  HmGrid g;
  float inv[9];          // the inverse of A, row-major: inv * (P - pos) = depth * (u, v, 1)
  float cell;            // 1 / inv_cell
  uint32_t whole_image;  // A has no usable inverse: every workgroup scans the whole image
  uint32_t out_h, out_w, tiles_x, tiles_y;
  float* hmap;           // [n][out_h][out_w]
  uint8_t* cmap;         // [n][out_h][out_w][3] or null (with rgb)
  uint8_t* smap;         // [n][out_h][out_w] or null (with seg)
  int32_t* src;          // [n][out_h][out_w] or null
};

// one launch on `stream`; every element of every non-null output is written exactly once
extern "C" void mre_launch_heightmap(const HeightmapArgs* a, hipStream_t stream);
#endif

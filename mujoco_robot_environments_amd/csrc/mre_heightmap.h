// Orthographic heightmaps on the device (csrc/mre_heightmap.hip, one camera; csrc/mre_heightmap_views.hip, several fused):
// the depth / rgb / seg frames of every env binned top-down into a height map, a colour map, a label map and the source
// pixel of every cell.  Shared between the kernels' translation units and the C ABI (mre_stream_api.cpp); NOT part of
// lib.source_hash(): nothing here is launched by the step or the camera.
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

// Several views fused into one set of maps (csrc/mre_heightmap_views.hip): what differs per view travels
// by value in the kernel arguments (128 B a view), the grid and the outputs once.
constexpr int HM_MAX_VIEWS = 8;              // MRE_HM_MAX_VIEWS of include/mre.h; the key has 4 bits for the view
constexpr uint32_t HM_VIEW_PIXELS = 1u << 28;   // h * w of a view stays below: the key has 28 bits for the index

struct HeightmapView {
  const float* depth;    // [n][h][w]
  const uint8_t* rgb;    // [n][h][w][3] or null (every view or none)
  const uint8_t* seg;    // [n][h][w] or null (every view or none)
  uint32_t h, w;         // h * w < 2^28
  uint32_t whole_image;  // as HeightmapArgs::whole_image
  uint32_t hw;           // h * w
  float cam[12];         // HmGrid::cam of this view
  float inv[9];          // as HeightmapArgs::inv
  float pad;             // to 128 B
};

struct HeightmapViewsArgs {
  HeightmapView v[HM_MAX_VIEWS];
  uint32_t views, n;
  HmGrid g;              // what the views share; g.cam is not read (HeightmapView::cam is)
  float cell;
  uint32_t out_h, out_w, tiles_x, tiles_y;
  float* hmap;           // [n][out_h][out_w]
  uint8_t* cmap;         // [n][out_h][out_w][3] or null (with rgb)
  uint8_t* smap;         // [n][out_h][out_w] or null (with seg)
  int32_t* src;          // [n][out_h][out_w] or null: the index inside the winning view's image
  uint8_t* view;         // [n][out_h][out_w] or null: the winning view, 255 = empty
};

#if defined(__HIPCC__)
// ---- what k_heightmap and k_heightmap_views share on the device
struct Rect { uint32_t u0, v0, rw, count; };   // first column and row, columns, pixels (0: nothing to scan)

// the source rectangle of the tile whose cells are columns [cx0, cx1) and rows [cy0, cy1)
__device__ __forceinline__ Rect tile_rect(const HeightmapArgs& a, uint32_t cx0, uint32_t cx1, uint32_t cy0, uint32_t cy1) {
  const float wm = (float)(a.w - 1), hm = (float)(a.h - 1);
  bool whole = a.whole_image != 0;
  float umin = 3.0e38f, umax = -3.0e38f, vmin = 3.0e38f, vmax = -3.0e38f;
  const float xs[2] = {a.g.lo[0] + (float)cx0 * a.cell, a.g.lo[0] + (float)cx1 * a.cell};
  const float ys[2] = {a.g.lo[1] + (float)cy0 * a.cell, a.g.lo[1] + (float)cy1 * a.cell};
  const float zs[2] = {a.g.lo[2], a.g.hi[2]};
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const float px = xs[c & 1] - a.g.cam[9], py = ys[(c >> 1) & 1] - a.g.cam[10], pz = zs[c >> 2] - a.g.cam[11];
    const float q0 = a.inv[0] * px + a.inv[1] * py + a.inv[2] * pz;
    const float q1 = a.inv[3] * px + a.inv[4] * py + a.inv[5] * pz;
    const float q2 = a.inv[6] * px + a.inv[7] * py + a.inv[8] * pz;   // the corner's depth: minus its camera-frame z
    if (!(q2 >= 1e-3f)) whole = true;
    const float r = 1.0f / q2;
    const float u = q0 * r, v = q1 * r;
    umin = fminf(umin, u); umax = fmaxf(umax, u);   // fminf / fmaxf drop a NaN
    vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
  }
  float u0 = 0.f, u1 = wm, v0 = 0.f, v1 = hm;
  if (!whole) {
    u0 = fmaxf(floorf(umin) - 2.f, 0.f); u1 = fminf(ceilf(umax) + 2.f, wm);
    v0 = fmaxf(floorf(vmin) - 2.f, 0.f); v1 = fminf(ceilf(vmax) + 2.f, hm);
  }
  Rect r = {0u, 0u, 1u, 0u};
  if (u0 <= u1 && v0 <= v1) {   // all four are now inside the image
    r.u0 = (uint32_t)u0; r.v0 = (uint32_t)v0;
    r.rw = (uint32_t)u1 - r.u0 + 1u;
    r.count = r.rw * ((uint32_t)v1 - r.v0 + 1u);   // <= h * w < 2^31
  }
  return r;
}
#endif

// one launch on `stream`; every element of every non-null output is written exactly once
extern "C" void mre_launch_heightmap(const HeightmapArgs* a, hipStream_t stream);
extern "C" void mre_launch_heightmap_views(const HeightmapViewsArgs* a, hipStream_t stream);
#endif

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

// What the two launches share: the grid of the maps, its tiling and the outputs.  mre_stream_api.cpp fills it once.
struct HmMaps {
  HmGrid g;              // g.cam is the camera of mre_heightmap; mre_heightmap_views reads HeightmapView::cam instead
  float cell;            // 1 / inv_cell
  uint32_t out_h, out_w, tiles_x, tiles_y;
  float* hmap;           // [n][out_h][out_w]
  uint8_t* cmap;         // [n][out_h][out_w][3] or null (with rgb)
  uint8_t* smap;         // [n][out_h][out_w] or null (with seg)
  int32_t* src;          // [n][out_h][out_w] or null: the index inside the winning image
};

struct HeightmapArgs {
  const float* depth;    // [n][h][w]
  const uint8_t* rgb;    // [n][h][w][3] or null
  const uint8_t* seg;    // [n][h][w] or null
  uint32_t n, h, w;      // h * w < 2^31
  float inv[9];          // the inverse of A, row-major: inv * (P - pos) = depth * (u, v, 1)
  uint32_t whole_image;  // A has no usable inverse: every workgroup scans the whole image
  HmMaps m;
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
  HmMaps m;              // m.src is the index inside the winning view's image
  uint8_t* view;         // [n][out_h][out_w] or null: the winning view, 255 = empty
};

// workgroups of a launch over n envs: one per (env, tile) up to HM_MAX_GRID, the kernels loop over the rest
inline uint32_t hm_launch_grid(uint32_t n, const HmMaps& m) {
  const size_t items = (size_t)n * m.tiles_x * m.tiles_y;
  return (uint32_t)(items < HM_MAX_GRID ? items : HM_MAX_GRID);
}

#if defined(__HIPCC__)
// ---- what k_heightmap and k_heightmap_views share on the device: everything but the loop over views and the choice of
// the winner's images
constexpr int HM_NT = 256;     // threads per workgroup
constexpr int HM_UNROLL = 4;   // depth loads a lane has in flight

struct HmTile { uint32_t e, cx0, cy0, cx1, cy1; };   // the env, and the tile's cells: columns [cx0, cx1), rows [cy0, cy1)
struct Rect { uint32_t u0, v0, rw, count; };         // first column and row, columns, pixels (0: nothing to scan)

// work item `item` of a launch: tiles_x * tiles_y tiles per env, row by row
__device__ __forceinline__ HmTile hm_tile(const HmMaps& m, size_t item) {
  const uint32_t tiles = m.tiles_x * m.tiles_y;
  HmTile tl;
  tl.e = (uint32_t)(item / tiles);
  const uint32_t tile = (uint32_t)(item - (size_t)tl.e * tiles);
  const uint32_t ty = tile / m.tiles_x, tx = tile - ty * m.tiles_x;
  tl.cx0 = tx * HM_TILE; tl.cy0 = ty * HM_TILE;
  tl.cx1 = min(tl.cx0 + HM_TILE, m.out_w); tl.cy1 = min(tl.cy0 + HM_TILE, m.out_h);
  return tl;
}

// the source rectangle of tile tl in an h x w image seen through g.cam, whose inverse is inv
__device__ __forceinline__ Rect tile_rect(const HmGrid& g, const float* inv, float cell, uint32_t h, uint32_t w,
                                          uint32_t whole_image, const HmTile& tl) {
  const float wm = (float)(w - 1), hm = (float)(h - 1);
  bool whole = whole_image != 0;
  float umin = 3.0e38f, umax = -3.0e38f, vmin = 3.0e38f, vmax = -3.0e38f;
  const float xs[2] = {g.lo[0] + (float)tl.cx0 * cell, g.lo[0] + (float)tl.cx1 * cell};
  const float ys[2] = {g.lo[1] + (float)tl.cy0 * cell, g.lo[1] + (float)tl.cy1 * cell};
  const float zs[2] = {g.lo[2], g.hi[2]};
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const float px = xs[c & 1] - g.cam[9], py = ys[(c >> 1) & 1] - g.cam[10], pz = zs[c >> 2] - g.cam[11];
    const float q0 = inv[0] * px + inv[1] * py + inv[2] * pz;
    const float q1 = inv[3] * px + inv[4] * py + inv[5] * pz;
    const float q2 = inv[6] * px + inv[7] * py + inv[8] * pz;   // the corner's depth: minus its camera-frame z
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

// lane t of the workgroup scans rectangle rc of the image dimg (w columns, seen through g.cam): one LDS atomicMax into
// `keys` for every pixel that lands in tile tl, keyed as view `view` (hm_key_view; view 0 gives hm_key).  g travels by value:
// through a reference the compiler keeps hm_point's validity test as a chain of branches per pixel, which measured 3 %
// slower in k_heightmap; by value the test folds into one branch, as it did when this loop stood in the kernel
__device__ __forceinline__ void hm_scan(unsigned long long* keys, const HmGrid g, const float* dimg, uint32_t w,
                                        const Rect& rc, uint32_t view, const HmTile& tl, uint32_t t) {
  for (uint32_t i0 = t; i0 < rc.count; i0 += HM_NT * HM_UNROLL) {
    uint32_t idx[HM_UNROLL], uu[HM_UNROLL], vv[HM_UNROLL];
    float d[HM_UNROLL];
#pragma unroll
    for (int j = 0; j < HM_UNROLL; j++) {   // a pixel past the rectangle re-reads its last one and is not used
      const uint32_t i = min(i0 + j * HM_NT, rc.count - 1u);
      const uint32_t row = i / rc.rw;
      uu[j] = rc.u0 + (i - row * rc.rw);
      vv[j] = rc.v0 + row;
      idx[j] = vv[j] * w + uu[j];
      d[j] = dimg[idx[j]];
    }
#pragma unroll
    for (int j = 0; j < HM_UNROLL; j++) {
      if (i0 + j * HM_NT >= rc.count) break;
      const HmPoint p = hm_point(g, (float)uu[j], (float)vv[j], d[j]);
      if (p.valid) {   // 0 <= cx < out_w and 0 <= cy < out_h: the casts are exact
        const uint32_t ix = (uint32_t)p.cx - tl.cx0, iy = (uint32_t)p.cy - tl.cy0;
        if (ix < (uint32_t)HM_TILE && iy < (uint32_t)HM_TILE)
          atomicMax(&keys[iy * HM_TILE + ix], hm_key_view(__float_as_uint(p.hz), view, idx[j]));
      }
    }
  }
}

// the output element of cell i of tile tl's keys; false where the cell lies outside the map
__device__ __forceinline__ bool hm_cell(const HmMaps& m, const HmTile& tl, uint32_t i, size_t* o) {
  const uint32_t ox = tl.cx0 + i % HM_TILE, oy = tl.cy0 + i / HM_TILE;
  *o = ((size_t)tl.e * m.out_h + oy) * m.out_w + ox;
  return ox < m.out_w && oy < m.out_h;
}

// output element o from its cell's key: `index` is the winner's pixel as the kernel decodes it, rgb and seg are the
// winner's images and s that pixel in them (read for a filled cell only)
__device__ __forceinline__ void hm_write_cell(const HmMaps& m, size_t o, unsigned long long key, uint32_t index,
                                              const uint8_t* rgb, const uint8_t* seg, size_t s) {
  const bool filled = key != 0ull;
  m.hmap[o] = filled ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
  if (m.src) m.src[o] = filled ? (int32_t)index : -1;
  if (m.smap) m.smap[o] = filled ? seg[s] : (uint8_t)255;
  if (m.cmap) {
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    if (filled) { c0 = rgb[3 * s]; c1 = rgb[3 * s + 1]; c2 = rgb[3 * s + 2]; }
    m.cmap[3 * o] = c0; m.cmap[3 * o + 1] = c1; m.cmap[3 * o + 2] = c2;
  }
}
#endif

// one launch on `stream`; every element of every non-null output is written exactly once
extern "C" void mre_launch_heightmap(const HeightmapArgs* a, hipStream_t stream);
extern "C" void mre_launch_heightmap_views(const HeightmapViewsArgs* a, hipStream_t stream);
#endif

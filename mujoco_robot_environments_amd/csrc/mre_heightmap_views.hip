// Orthographic heightmaps from several cameras in one pass: the maps of csrc/mre_heightmap.hip with
// every view's pixels competing for the same cells.  A cell takes the valid pixel (hm_point, unchanged) with the largest
// height over all views, among equal heights the smallest view, inside it the smallest index -- the merge of the views'
// own mre_heightmap maps, without those maps ever being written.
//
//   k_heightmap_views   k_heightmap's shape: one workgroup per (env, tile of T x T cells), the tile's 64-bit keys in LDS
//                       ((height bits << 32) | ~(view << 28 | index): hm_key_view), 0 = empty.  For each view in turn the
//                       workgroup projects the tile's box into that view (tile_rect), scans the rectangle and does one LDS
//                       atomicMax per pixel that lands in the tile; no barrier separates the views, because max commutes.
//                       One epilogue writes the tile: rgb and seg are read for the winners only, from the winning view.
//
// No global atomic, no init pass, no workspace; every output element is written exactly once by the workgroup that owns
// its tile, and the outputs are the same bits whatever order lanes and views arrive in.  What differs per view (pointers,
// sizes, camera, inverse) is read from the kernel arguments: the view of the scan is the same in every lane (scalar loads),
// the winner's view in the epilogue is not (a vector load from the argument segment).
#include "mre_heightmap.h"

namespace {

constexpr int NT = 256;     // threads per workgroup
constexpr int UNROLL = 4;   // depth loads a lane has in flight
constexpr int T = HM_TILE;

__global__ void __launch_bounds__(NT) k_heightmap_views(HeightmapViewsArgs a) {
  __shared__ unsigned long long keys[T * T];
  const uint32_t t = threadIdx.x;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  const size_t cells = (size_t)a.out_h * a.out_w;
  const size_t items = (size_t)a.n * tiles;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = (uint32_t)(item / tiles), tile = (uint32_t)(item - (size_t)e * tiles);
    const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const uint32_t cx0 = tx * T, cy0 = ty * T;
    const uint32_t cx1 = min(cx0 + T, a.out_w), cy1 = min(cy0 + T, a.out_h);
    for (uint32_t i = t; i < T * T; i += NT) keys[i] = 0ull;
    __syncthreads();
    for (uint32_t view = 0; view < a.views; view++) {
      const HeightmapView& vw = a.v[view];
      HeightmapArgs s;   // this view as k_heightmap sees one: what tile_rect and hm_point read, nothing else
      s.g = a.g;
#pragma unroll
      for (int k = 0; k < 12; k++) s.g.cam[k] = vw.cam[k];
#pragma unroll
      for (int k = 0; k < 9; k++) s.inv[k] = vw.inv[k];
      s.h = vw.h; s.w = vw.w; s.cell = a.cell; s.whole_image = vw.whole_image;
      const Rect rc = tile_rect(s, cx0, cx1, cy0, cy1);   // the same in every lane
      const float* dimg = vw.depth + (size_t)e * vw.hw;
      for (uint32_t i0 = t; i0 < rc.count; i0 += NT * UNROLL) {
        uint32_t idx[UNROLL], uu[UNROLL], vv[UNROLL];
        float d[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {   // a pixel past the rectangle re-reads its last one and is not used
          const uint32_t i = min(i0 + j * NT, rc.count - 1u);
          const uint32_t row = i / rc.rw;
          uu[j] = rc.u0 + (i - row * rc.rw);
          vv[j] = rc.v0 + row;
          idx[j] = vv[j] * s.w + uu[j];
          d[j] = dimg[idx[j]];
        }
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
          if (i0 + j * NT >= rc.count) break;
          const HmPoint p = hm_point(s.g, (float)uu[j], (float)vv[j], d[j]);
          if (p.valid) {   // 0 <= cx < out_w and 0 <= cy < out_h: the casts are exact
            const uint32_t ix = (uint32_t)p.cx - cx0, iy = (uint32_t)p.cy - cy0;
            if (ix < (uint32_t)T && iy < (uint32_t)T)
              atomicMax(&keys[iy * T + ix], hm_key_view(__float_as_uint(p.hz), view, idx[j]));
          }
        }
      }
    }
    __syncthreads();
    for (uint32_t i = t; i < T * T; i += NT) {
      const uint32_t ox = cx0 + i % T, oy = cy0 + i / T;
      if (ox >= a.out_w || oy >= a.out_h) continue;
      const unsigned long long key = keys[i];
      const bool filled = key != 0ull;
      const uint32_t which = filled ? hm_key_which(key) : 0u;   // < views: only a view's own scan wrote the key
      const uint32_t index = hm_key_index(key);
      // the winner's images: a load from the kernel arguments at a per-lane view.  (Selecting among all eight views'
      // pointers held in SGPRs measured 4 % faster at three views, at the price of 16 spilled SGPRs: DESIGN.md 8f.11.)
      const HeightmapView& win = a.v[which];
      const size_t o = (size_t)e * cells + (size_t)oy * a.out_w + ox, s = (size_t)e * win.hw + index;
      a.hmap[o] = filled ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
      if (a.src) a.src[o] = filled ? (int32_t)index : -1;
      if (a.view) a.view[o] = filled ? (uint8_t)which : (uint8_t)255;
      if (a.smap) a.smap[o] = filled ? win.seg[s] : (uint8_t)255;
      if (a.cmap) {
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (filled) { const uint8_t* px = win.rgb + 3 * s; c0 = px[0]; c1 = px[1]; c2 = px[2]; }
        a.cmap[3 * o] = c0; a.cmap[3 * o + 1] = c1; a.cmap[3 * o + 2] = c2;
      }
    }
    __syncthreads();   // the keys are cleared for the next item
  }
}

}  // namespace

extern "C" void mre_launch_heightmap_views(const HeightmapViewsArgs* a, hipStream_t stream) {
  const size_t items = (size_t)a->n * a->tiles_x * a->tiles_y;
  hipLaunchKernelGGL(k_heightmap_views, dim3((uint32_t)(items < HM_MAX_GRID ? items : HM_MAX_GRID)), dim3(NT), 0,
                     stream, *a);
}

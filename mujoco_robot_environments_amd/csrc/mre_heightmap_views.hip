// Orthographic heightmaps from several cameras in one pass: the maps of csrc/mre_heightmap.hip with
// every view's pixels competing for the same cells.  A cell takes the valid pixel (hm_point, unchanged) with the largest
// height over all views, among equal heights the smallest view, inside it the smallest index -- the merge of the views'
// own mre_heightmap maps, without those maps ever being written.
//
//   k_heightmap_views   k_heightmap's shape: one workgroup per (env, tile of T x T cells), the tile's 64-bit keys in LDS
//                       ((height bits << 32) | ~(view << 28 | index): hm_key_view), 0 = empty.  For each view in turn the
//                       workgroup projects the tile's box into that view (tile_rect), scans the rectangle and does one LDS
//                       atomicMax per pixel that lands in the tile (hm_scan); no barrier separates the views, because max
//                       commutes.  One epilogue writes the tile: rgb and seg are read for the winners only, from the
//                       winning view.  The steps are k_heightmap's, from csrc/mre_heightmap.h; here is the loop over
//                       views and the choice of the winner's images.
//
// No global atomic, no init pass, no workspace; every output element is written exactly once by the workgroup that owns
// its tile, and the outputs are the same bits whatever order lanes and views arrive in.  What differs per view (pointers,
// sizes, camera, inverse) is read from the kernel arguments: the view of the scan is the same in every lane (scalar loads),
// the winner's view in the epilogue is not (a vector load from the argument segment).
#include "mre_heightmap.h"

namespace {

constexpr int T = HM_TILE;

__global__ void __launch_bounds__(HM_NT) k_heightmap_views(HeightmapViewsArgs a) {
  __shared__ unsigned long long keys[T * T];
  const uint32_t t = threadIdx.x;
  const size_t items = (size_t)a.n * a.m.tiles_x * a.m.tiles_y;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const HmTile tl = hm_tile(a.m, item);
    for (uint32_t i = t; i < T * T; i += HM_NT) keys[i] = 0ull;
    __syncthreads();
    for (uint32_t view = 0; view < a.views; view++) {
      const HeightmapView& vw = a.v[view];
      HmGrid g = a.m.g;   // the grid as this view's hm_point reads it
#pragma unroll
      for (int k = 0; k < 12; k++) g.cam[k] = vw.cam[k];
      const Rect rc = tile_rect(g, vw.inv, a.m.cell, vw.h, vw.w, vw.whole_image, tl);   // the same in every lane
      hm_scan(keys, g, vw.depth + (size_t)tl.e * vw.hw, vw.w, rc, view, tl, t);
    }
    __syncthreads();
    for (uint32_t i = t; i < T * T; i += HM_NT) {
      size_t o;
      if (!hm_cell(a.m, tl, i, &o)) continue;
      const unsigned long long key = keys[i];
      const uint32_t which = key != 0ull ? hm_key_which(key) : 0u;   // < views: only a view's own scan wrote the key
      const uint32_t index = hm_key_index(key);
      // the winner's images: a load from the kernel arguments at a per-lane view.  (Selecting among all eight views'
      // pointers held in SGPRs measured 4 % faster at three views, at the price of 16 spilled SGPRs: DESIGN.md 8f.11.)
      const HeightmapView& win = a.v[which];
      hm_write_cell(a.m, o, key, index, win.rgb, win.seg, (size_t)tl.e * win.hw + index);
      if (a.view) a.view[o] = key != 0ull ? (uint8_t)which : (uint8_t)255;
    }
    __syncthreads();   // the keys are cleared for the next item
  }
}

}  // namespace

extern "C" void mre_launch_heightmap_views(const HeightmapViewsArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(k_heightmap_views, dim3(hm_launch_grid(a->n, a->m)), dim3(HM_NT), 0, stream, *a);
}

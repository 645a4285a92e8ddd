// Orthographic heightmaps on the device: what a Transporter network is trained on, from the frames the batched camera
// (csrc/mre_render.hip) left in HBM.  Every depth pixel is pushed back through the pinhole model (hm_point,
// csrc/mre_heightmap_point.h) and a cell of the map takes the highest point that lands in it, the smallest source index
// among equal heights: hmap its height, cmap its colour, smap its label, src its index.
//
//   k_heightmap   one workgroup per (env, tile of T x T cells, T = HM_TILE).  The tile's cells are 64-bit keys in LDS
//                 ((height bits << 32) | ~index: hm_key), 0 = empty.  The workgroup projects the 8 corners of the
//                 tile's box [x range] x [y range] x [lo_z, hi_z] into the image (tile_rect), scans the bounding rectangle
//                 of the projections widened by 2 pixels (the whole image when a corner is not in front of the camera;
//                 hm_scan), does one LDS atomicMax for every pixel that lands in its own tile, and then writes the tile
//                 (hm_write_cell): rgb and seg are read for the winners only.  The steps are the device functions of
//                 csrc/mre_heightmap.h, which csrc/mre_heightmap_views.hip calls once per view; here is the order of
//                 the steps for one view, and the decode of its key.
//
// No global atomic, no init pass, no workspace: every output element is written exactly once, by the workgroup that owns
// its tile, and max of integers commutes, so the outputs are the same bits whatever order the lanes arrive in.  The
// rectangle only bounds the work: a pixel is binned by hm_point alone, and a point of the tile's box projects inside the
// hull of the box's projected corners (the rounding of hm_point moves it by far less than the 2 pixels).  The price is
// that neighbouring tiles re-read the pixels their boxes share through parallax.
#include "mre_heightmap.h"

namespace {

constexpr int T = HM_TILE;

__global__ void __launch_bounds__(HM_NT) k_heightmap(HeightmapArgs a) {
  __shared__ unsigned long long keys[T * T];
  const uint32_t t = threadIdx.x;
  const uint32_t hw = a.h * a.w;
  const size_t items = (size_t)a.n * a.m.tiles_x * a.m.tiles_y;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const HmTile tl = hm_tile(a.m, item);
    for (uint32_t i = t; i < T * T; i += HM_NT) keys[i] = 0ull;
    const Rect rc = tile_rect(a.m.g, a.inv, a.m.cell, a.h, a.w, a.whole_image, tl);   // the same in every lane
    __syncthreads();
    hm_scan(keys, a.m.g, a.depth + (size_t)tl.e * hw, a.w, rc, 0u, tl, t);   // view 0: hm_key
    __syncthreads();
    for (uint32_t i = t; i < T * T; i += HM_NT) {
      size_t o;
      if (!hm_cell(a.m, tl, i, &o)) continue;
      const unsigned long long key = keys[i];
      // not hm_key_index: one view has up to 2^31 - 1 pixels, and its key keeps all 32 bits for the index
      const uint32_t index = 0xFFFFFFFFu - (uint32_t)key;
      hm_write_cell(a.m, o, key, index, a.rgb, a.seg, (size_t)tl.e * hw + index);
    }
    __syncthreads();   // the keys are cleared for the next item
  }
}

}  // namespace

extern "C" void mre_launch_heightmap(const HeightmapArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(k_heightmap, dim3(hm_launch_grid(a->n, a->m)), dim3(HM_NT), 0, stream, *a);
}

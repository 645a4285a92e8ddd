// Orthographic heightmaps on the device: what a Transporter network is trained on, from the frames the batched camera
// (csrc/mre_render.hip) left in HBM.  Every depth pixel is pushed back through the pinhole model (hm_point,
// csrc/mre_heightmap_point.h) and a cell of the map takes the highest point that lands in it, the smallest source index
// among equal heights: hmap its height, cmap its colour, smap its label, src its index.
//
//   k_heightmap   one workgroup per (env, tile of T x T cells, T = HM_TILE).  The tile's cells are 64-bit keys in LDS
//                 ((height bits << 32) | ~index: hm_key), 0 = empty.  The workgroup projects the 8 corners of the
//                 tile's box [x range] x [y range] x [lo_z, hi_z] into the image (tile_rect of csrc/mre_heightmap.h, which
//                 csrc/mre_heightmap_views.hip shares), scans the bounding rectangle of the
//                 projections widened by 2 pixels (the whole image when a corner is not in front of the camera), does
//                 one LDS atomicMax for every pixel that lands in its own tile, and then writes the tile: rgb and seg
//                 are read for the winners only.
//
// No global atomic, no init pass, no workspace: every output element is written exactly once, by the workgroup that owns
// its tile, and max of integers commutes, so the outputs are the same bits whatever order the lanes arrive in.  The
// rectangle only bounds the work: a pixel is binned by hm_point alone, and a point of the tile's box projects inside the
// hull of the box's projected corners (the rounding of hm_point moves it by far less than the 2 pixels).  The price is
// that neighbouring tiles re-read the pixels their boxes share through parallax.
#include "mre_heightmap.h"

namespace {

constexpr int NT = 256;     // threads per workgroup
constexpr int UNROLL = 4;   // depth loads a lane has in flight
constexpr int T = HM_TILE;

__global__ void __launch_bounds__(NT) k_heightmap(HeightmapArgs a) {
  __shared__ unsigned long long keys[T * T];
  const uint32_t t = threadIdx.x;
  const uint32_t hw = a.h * a.w, tiles = a.tiles_x * a.tiles_y;
  const size_t cells = (size_t)a.out_h * a.out_w;
  const size_t items = (size_t)a.n * tiles;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = (uint32_t)(item / tiles), tile = (uint32_t)(item - (size_t)e * tiles);
    const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const uint32_t cx0 = tx * T, cy0 = ty * T;
    const uint32_t cx1 = min(cx0 + T, a.out_w), cy1 = min(cy0 + T, a.out_h);
    for (uint32_t i = t; i < T * T; i += NT) keys[i] = 0ull;
    const Rect rc = tile_rect(a, cx0, cx1, cy0, cy1);   // the same in every lane
    __syncthreads();
    const float* dimg = a.depth + (size_t)e * hw;
    for (uint32_t i0 = t; i0 < rc.count; i0 += NT * UNROLL) {
      uint32_t idx[UNROLL], uu[UNROLL], vv[UNROLL];
      float d[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; j++) {   // a pixel past the rectangle re-reads its last one and is not used
        const uint32_t i = min(i0 + j * NT, rc.count - 1u);
        const uint32_t row = i / rc.rw;
        uu[j] = rc.u0 + (i - row * rc.rw);
        vv[j] = rc.v0 + row;
        idx[j] = vv[j] * a.w + uu[j];
        d[j] = dimg[idx[j]];
      }
#pragma unroll
      for (int j = 0; j < UNROLL; j++) {
        if (i0 + j * NT >= rc.count) break;
        const HmPoint p = hm_point(a.g, (float)uu[j], (float)vv[j], d[j]);
        if (p.valid) {   // 0 <= cx < out_w and 0 <= cy < out_h: the casts are exact
          const uint32_t ix = (uint32_t)p.cx - cx0, iy = (uint32_t)p.cy - cy0;
          if (ix < (uint32_t)T && iy < (uint32_t)T) atomicMax(&keys[iy * T + ix], hm_key(__float_as_uint(p.hz), idx[j]));
        }
      }
    }
    __syncthreads();
    for (uint32_t i = t; i < T * T; i += NT) {
      const uint32_t ox = cx0 + i % T, oy = cy0 + i / T;
      if (ox >= a.out_w || oy >= a.out_h) continue;
      const unsigned long long key = keys[i];
      const bool filled = key != 0ull;
      const uint32_t index = 0xFFFFFFFFu - (uint32_t)key;
      const size_t o = (size_t)e * cells + (size_t)oy * a.out_w + ox, s = (size_t)e * hw + index;
      a.hmap[o] = filled ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
      if (a.src) a.src[o] = filled ? (int32_t)index : -1;
      if (a.smap) a.smap[o] = filled ? a.seg[s] : (uint8_t)255;
      if (a.cmap) {
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (filled) { c0 = a.rgb[3 * s]; c1 = a.rgb[3 * s + 1]; c2 = a.rgb[3 * s + 2]; }
        a.cmap[3 * o] = c0; a.cmap[3 * o + 1] = c1; a.cmap[3 * o + 2] = c2;
      }
    }
    __syncthreads();   // the keys are cleared for the next item
  }
}

}  // namespace

extern "C" void mre_launch_heightmap(const HeightmapArgs* a, hipStream_t stream) {
  const size_t items = (size_t)a->n * a->tiles_x * a->tiles_y;
  hipLaunchKernelGGL(k_heightmap, dim3((uint32_t)(items < HM_MAX_GRID ? items : HM_MAX_GRID)), dim3(NT), 0,
                     stream, *a);
}

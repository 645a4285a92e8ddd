// The gather that the map warp (csrc/mre_warp.hip) and the network inputs (csrc/mre_warp_inputs.hip) share, stated once.
// Device only: the two kernels' translation units include it, the C ABI does not.
//
//   wp_for_each_lane   one workgroup of 256 lanes per (sample, tile of 16 rows x 64 columns), further items in a grid-stride
//                      loop; a lane owns 4 consecutive columns of one row, and a lane whose row or first column lies
//                      outside the output does nothing.  The six floats and the map index of the sample are the same in
//                      every lane of the workgroup.  The source cell of each of the 4 cells is wp_cell / wp_from
//                      (csrc/mre_warp_point.h).  A lane issues all its gathers (4 heights, 12 colour bytes, 4 labels)
//                      before the body uses the first; an invalid cell reads cell 0 of map 0 (n >= 1), which exists, and
//                      the body drops it.  COLOUR, LABEL: the maps that are read; compiled in, so that no branch stands
//                      between the gathers and a lane has all of them in flight at once.
//
// The source footprint of a tile is a rotated rectangle of about the tile's own size, which the vector cache and L2
// serve; no LDS, no atomics, no workspace.
#ifndef MRE_WARP_GATHER_H
#define MRE_WARP_GATHER_H
#include "mre_warp.h"

constexpr int WP_NT = 256;   // threads per workgroup: WP_TILE_H rows x (WP_TILE_W / 4) lanes
static_assert(WP_NT == WP_TILE_H * (WP_TILE_W / 4), "a lane owns 4 columns of one row of the tile");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// a lane's 4 cells: output cell (row, col0 + j) of sample s, and what its source cell holds
struct WpLane {
  uint32_t s, row, col0;
  bool valid[4];     // the source cell exists; where it does not, off is 0 and the values are those of map 0's cell 0
  uint32_t off[4];   // wp_from: the source cell inside its map
  float hz[4];
  uint8_t rgb[12] = {};   // zeros without COLOUR
  uint8_t lab[4] = {};    // zeros without LABEL
};

// body(const WpLane&) once for every lane of every (sample, tile) item that has a cell inside the output
template <bool COLOUR, bool LABEL, class Body>
__device__ __forceinline__ void wp_for_each_lane(const WarpSource& a, const uint8_t* smap, Body body) {
  const uint32_t t = threadIdx.x;
  const uint32_t lr = t / (WP_TILE_W / 4), lc = (t % (WP_TILE_W / 4)) * 4;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  const size_t hw = (size_t)a.in_h * a.in_w;
  const size_t items = (size_t)a.samples * tiles;
  const float in_w = (float)a.in_w, in_h = (float)a.in_h;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    WpLane g;
    g.s = (uint32_t)(item / tiles);
    const uint32_t tile = (uint32_t)(item - (size_t)g.s * tiles);
    const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    g.row = ty * WP_TILE_H + lr;
    g.col0 = tx * WP_TILE_W + lc;
    if (g.row >= a.out_h || g.col0 >= a.out_w) continue;
    float m[6];
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = a.mats[(size_t)g.s * 6 + k];
    const int32_t e = a.index ? a.index[g.s] : (int32_t)g.s;
    const bool map_ok = e >= 0 && (uint32_t)e < a.n;
    const size_t base = map_ok ? (size_t)e * hw : 0;   // an invalid cell reads cell 0 of a map that exists
    const float r = (float)g.row;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const WpCell p = wp_cell(m, (float)(g.col0 + j), r, in_w, in_h, map_ok);
      g.valid[j] = p.valid;
      g.off[j] = p.valid ? (uint32_t)wp_from(p, (int32_t)a.in_w) : 0u;
    }
    // every gather is issued before the first use
#pragma unroll
    for (int j = 0; j < 4; j++) g.hz[j] = a.hmap[base + g.off[j]];
    if (COLOUR) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint8_t* px = a.cmap + 3 * (base + g.off[j]);
        g.rgb[3 * j] = px[0]; g.rgb[3 * j + 1] = px[1]; g.rgb[3 * j + 2] = px[2];
      }
    }
    if (LABEL) {
#pragma unroll
      for (int j = 0; j < 4; j++) g.lab[j] = smap[base + g.off[j]];
    }
    body(g);
  }
}

// one launch on `stream` of the instantiation `kernel` of a kernel built on wp_for_each_lane
template <class Args>
inline void wp_launch(void (*kernel)(Args), const Args& a, hipStream_t stream) {
  const size_t items = (size_t)a.source.samples * a.source.tiles_x * a.source.tiles_y;
  const dim3 grid((uint32_t)(items < WP_MAX_GRID ? items : WP_MAX_GRID));
  hipLaunchKernelGGL(kernel, grid, dim3(WP_NT), 0, stream, a);
}
#endif

// Warped and cropped maps on the device: what a Transporter learner does to every sample before the network sees it.
// An output cell (row r, column c) of sample s takes height, colour and label of the source cell its matrix sends it to
// (wp_cell, csrc/mre_warp_point.h), rounded to the nearest cell, in the source map index[s] -- or the empty values of
// mre_heightmap when that cell, or the map, does not exist.  The SE(2) perturbation of a whole map and the rotated crops
// around a pick cell are both calls of it.
//
//   k_warp_maps        one workgroup of 256 lanes per (sample, tile of 16 rows x 64 columns); a lane owns 4 consecutive
//                      columns of one row.  The six floats and the map index of the sample are the same in every lane of
//                      the workgroup.  A lane issues all its gathers (4 heights, 12 colour bytes, 4 labels) before it uses
//                      the first; an invalid cell reads cell 0 of map 0 (n >= 1), which exists, and drops it.
//                      VEC: out_w % 4 == 0 and the output bases are aligned, so a lane's 4 cells are all inside the
//                      output or all outside, and it stores 16 B of heights, 3 dwords of colour, 1 dword of labels and
//                      16 B of source indices.  Otherwise every element is stored on its own, at any byte offset.
//                      COLOUR, LABEL: the maps that are given; compiled in, so that no branch stands between the
//                      gathers and a lane has all of them in flight at once.
//
// The kernel is bound by memory: 8 B read and 8 B (12 B with `from`) written per cell.  The source footprint of a tile is
// a rotated rectangle of about the tile's own size, which the vector cache and L2 serve; no LDS, no atomics, no
// workspace.  Every output element is written exactly once, by the lane that owns it.
#include "mre_warp.h"

namespace {

constexpr int NT = 256;   // threads per workgroup: WP_TILE_H rows x (WP_TILE_W / 4) lanes
static_assert(NT == WP_TILE_H * (WP_TILE_W / 4), "a lane owns 4 columns of one row of the tile");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <bool VEC, bool COLOUR, bool LABEL>
__global__ void __launch_bounds__(NT) k_warp_maps(WarpArgs a) {
  const uint32_t t = threadIdx.x;
  const uint32_t lr = t / (WP_TILE_W / 4), lc = (t % (WP_TILE_W / 4)) * 4;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  const size_t cells = (size_t)a.out_h * a.out_w, hw = (size_t)a.in_h * a.in_w;
  const size_t items = (size_t)a.samples * tiles;
  const float in_w = (float)a.in_w, in_h = (float)a.in_h;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t s = (uint32_t)(item / tiles), tile = (uint32_t)(item - (size_t)s * tiles);
    const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const uint32_t row = ty * WP_TILE_H + lr, col0 = tx * WP_TILE_W + lc;
    if (row >= a.out_h || col0 >= a.out_w) continue;
    float m[6];
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = a.mats[(size_t)s * 6 + k];
    const int32_t e = a.index ? a.index[s] : (int32_t)s;
    const bool map_ok = e >= 0 && (uint32_t)e < a.n;
    const size_t base = map_ok ? (size_t)e * hw : 0;   // an invalid cell reads cell 0 of a map that exists
    bool valid[4];
    uint32_t off[4];
    const float r = (float)row;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const WpCell p = wp_cell(m, (float)(col0 + j), r, in_w, in_h, map_ok);
      valid[j] = p.valid;
      off[j] = p.valid ? (uint32_t)wp_from(p, (int32_t)a.in_w) : 0u;
    }
    // every gather is issued before the first use
    float hz[4];
    uint8_t lab[4] = {}, rgb[12] = {};
#pragma unroll
    for (int j = 0; j < 4; j++) hz[j] = a.hmap[base + off[j]];
    if (COLOUR) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint8_t* px = a.cmap + 3 * (base + off[j]);
        rgb[3 * j] = px[0]; rgb[3 * j + 1] = px[1]; rgb[3 * j + 2] = px[2];
      }
    }
    if (LABEL) {
#pragma unroll
      for (int j = 0; j < 4; j++) lab[j] = a.smap[base + off[j]];
    }
    int32_t src[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      hz[j] = valid[j] ? hz[j] : 0.f;
      src[j] = valid[j] ? (int32_t)off[j] : -1;
      lab[j] = valid[j] ? lab[j] : (uint8_t)255;
      rgb[3 * j] = valid[j] ? rgb[3 * j] : (uint8_t)0;
      rgb[3 * j + 1] = valid[j] ? rgb[3 * j + 1] : (uint8_t)0;
      rgb[3 * j + 2] = valid[j] ? rgb[3 * j + 2] : (uint8_t)0;
    }
    const size_t o = (size_t)s * cells + (size_t)row * a.out_w + col0;
    if (VEC) {   // col0 + 3 < out_w and o % 4 == 0
      f32x4 h4 = {hz[0], hz[1], hz[2], hz[3]};
      *reinterpret_cast<f32x4*>(a.out_h_ + o) = h4;
      if (a.from) {
        i32x4 s4 = {src[0], src[1], src[2], src[3]};
        *reinterpret_cast<i32x4*>(a.from + o) = s4;
      }
      if (LABEL)
        *reinterpret_cast<uint32_t*>(a.out_s + o) =
            (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
      if (COLOUR) {
        uint32_t* c = reinterpret_cast<uint32_t*>(a.out_c + 3 * o);
#pragma unroll
        for (int k = 0; k < 3; k++)
          c[k] = (uint32_t)rgb[4 * k] | ((uint32_t)rgb[4 * k + 1] << 8) | ((uint32_t)rgb[4 * k + 2] << 16) |
                 ((uint32_t)rgb[4 * k + 3] << 24);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (col0 + j >= a.out_w) break;
        a.out_h_[o + j] = hz[j];
        if (a.from) a.from[o + j] = src[j];
        if (LABEL) a.out_s[o + j] = lab[j];
        if (COLOUR) {
          a.out_c[3 * (o + j)] = rgb[3 * j]; a.out_c[3 * (o + j) + 1] = rgb[3 * j + 1]; a.out_c[3 * (o + j) + 2] = rgb[3 * j + 2];
        }
      }
    }
  }
}

}  // namespace

extern "C" void mre_launch_warp_maps(const WarpArgs* a, hipStream_t stream) {
  const size_t items = (size_t)a->samples * a->tiles_x * a->tiles_y;
  const dim3 grid((uint32_t)(items < WP_MAX_GRID ? items : WP_MAX_GRID));
  typedef void (*Kernel)(WarpArgs);
  static const Kernel table[8] = {k_warp_maps<false, false, false>, k_warp_maps<false, false, true>,
                                  k_warp_maps<false, true, false>,  k_warp_maps<false, true, true>,
                                  k_warp_maps<true, false, false>,  k_warp_maps<true, false, true>,
                                  k_warp_maps<true, true, false>,   k_warp_maps<true, true, true>};
  const Kernel k = table[(a->vec ? 4 : 0) + (a->cmap ? 2 : 0) + (a->smap ? 1 : 0)];
  hipLaunchKernelGGL(k, grid, dim3(NT), 0, stream, *a);
}

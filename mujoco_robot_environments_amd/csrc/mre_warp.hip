// Warped and cropped maps on the device: what a Transporter learner does to every sample before the network sees it.
// An output cell (row r, column c) of sample s takes height, colour and label of the source cell its matrix sends it to
// (wp_cell, csrc/mre_warp_point.h), rounded to the nearest cell, in the source map index[s] -- or the empty values of
// mre_heightmap when that cell, or the map, does not exist.  The SE(2) perturbation of a whole map and the rotated crops
// around a pick cell are both calls of it.
//
//   k_warp_maps        the gather of csrc/mre_warp_gather.h (a lane: 4 consecutive cells of one output row), then the
//                      empty values where the source cell does not exist, and the stores.
//                      VEC: out_w % 4 == 0 and the output bases are aligned, so a lane's 4 cells are all inside the
//                      output or all outside, and it stores 16 B of heights, 3 dwords of colour, 1 dword of labels and
//                      16 B of source indices.  Otherwise every element is stored on its own, at any byte offset.
//                      COLOUR, LABEL: the maps that are given.
//
// The kernel is bound by memory: 8 B read and 8 B (12 B with `from`) written per cell.  Every output element is written
// exactly once, by the lane that owns it.
#include "mre_warp_gather.h"

namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <bool VEC, bool COLOUR, bool LABEL>
__global__ void __launch_bounds__(WP_NT) k_warp_maps(WarpArgs a) {
  const size_t cells = (size_t)a.source.out_h * a.source.out_w;
  wp_for_each_lane<COLOUR, LABEL>(a.source, a.smap, [&](const WpLane& g) {
    float hz[4];
    int32_t src[4];
    uint8_t lab[4], rgb[12];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      hz[j] = g.valid[j] ? g.hz[j] : 0.f;
      src[j] = g.valid[j] ? (int32_t)g.off[j] : -1;
      lab[j] = g.valid[j] ? g.lab[j] : (uint8_t)255;
#pragma unroll
      for (int q = 0; q < 3; q++) rgb[3 * j + q] = g.valid[j] ? g.rgb[3 * j + q] : (uint8_t)0;
    }
    const size_t o = (size_t)g.s * cells + (size_t)g.row * a.source.out_w + g.col0;
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
        if (g.col0 + j >= a.source.out_w) break;
        a.out_h_[o + j] = hz[j];
        if (a.from) a.from[o + j] = src[j];
        if (LABEL) a.out_s[o + j] = lab[j];
        if (COLOUR) {
          a.out_c[3 * (o + j)] = rgb[3 * j]; a.out_c[3 * (o + j) + 1] = rgb[3 * j + 1]; a.out_c[3 * (o + j) + 2] = rgb[3 * j + 2];
        }
      }
    }
  });
}

}  // namespace

extern "C" void mre_launch_warp_maps(const WarpArgs* a, hipStream_t stream) {
  typedef void (*Kernel)(WarpArgs);
  static const Kernel table[8] = {k_warp_maps<false, false, false>, k_warp_maps<false, false, true>,
                                  k_warp_maps<false, true, false>,  k_warp_maps<false, true, true>,
                                  k_warp_maps<true, false, false>,  k_warp_maps<true, false, true>,
                                  k_warp_maps<true, true, false>,   k_warp_maps<true, true, true>};
  wp_launch(table[(a->vec ? 4 : 0) + (a->source.cmap ? 2 : 0) + (a->smap ? 1 : 0)], *a, stream);
}

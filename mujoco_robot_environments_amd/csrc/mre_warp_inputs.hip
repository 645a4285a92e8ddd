// Network-ready inputs on the device: the gather of mre_warp_maps (csrc/mre_warp_gather.h: the same text, so bit for bit)
// written as the tensor a convolution consumes -- planar [samples][channels][out_h][out_w], every channel a colour byte or
// the height of the source cell times a scale plus a bias (wi_value, csrc/mre_warp_input_point.h), in float32 or bfloat16
// (wi_bf16) -- in one launch, with no intermediate.
//
//   k_warp_inputs      the gather (a lane: 4 consecutive cells of one output row; a cell whose source does not exist is
//                      a raw 0.0f), then a walk over the channels in a rolled loop -- a trip reads its entry of the
//                      channel table (by value in the kernel's arguments, the same in every lane) by scalar loads;
//                      unrolled, the table's 48 scalars were hoisted and spilled, and it was slower --
//                      that stores a lane's 4 cells of each plane.
//                      VEC: out_w % 4 == 0 and out aligned, so a lane's 4 cells are all inside the output or all outside
//                      and it stores 16 B (float32) or 8 B (bfloat16) per channel.  Otherwise every element is stored on
//                      its own, at any element offset.
//                      COLOUR: a channel names a colour byte.
//                      BF16: the element type of out.
//
// Bound by memory: 8 B (4 B without colour) read per valid cell, channels x element size written per cell.  Output
// offsets are formed in 64 bits: 147 456 crops x 6 channels x 64 x 64 is 3.6e9 elements.  Every output element is written
// exactly once, by the lane that owns it.
#include "mre_warp_gather.h"
#include "mre_warp_inputs.h"

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool VEC, bool COLOUR, bool BF16>
__global__ void __launch_bounds__(WP_NT) k_warp_inputs(WarpInputArgs a) {
  const size_t cells = (size_t)a.source.out_h * a.source.out_w;
  wp_for_each_lane<COLOUR, false>(a.source, nullptr, [&](const WpLane& g) {
    // raw values, as bits: the colour bytes as floats (exact), the height; 0.0f where the source cell does not exist
    uint32_t raw[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int q = 0; q < 3; q++) raw[q][j] = g.valid[j] ? __float_as_uint((float)g.rgb[3 * j + q]) : 0u;
      raw[3][j] = g.valid[j] ? __float_as_uint(g.hz[j]) : 0u;
    }
    // channel 0; plane k is k * cells on
    const size_t o = (size_t)g.s * a.channels * cells + (size_t)g.row * a.source.out_w + g.col0;
#pragma unroll 1
    for (uint32_t k = 0; k < a.channels; k++) {
      // the channel's source by four uniform masks, one of them all ones: no branch, and a copy of the bits
      const uint32_t sk = a.src[k];
      const uint32_t m0 = sk == 0 ? ~0u : 0u, m1 = sk == 1 ? ~0u : 0u, m2 = sk == 2 ? ~0u : 0u, m3 = sk == 3 ? ~0u : 0u;
      const float scale = a.scale[k], bias = a.bias[k];
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        uint32_t x = raw[3][j];
        if (COLOUR) x = (raw[0][j] & m0) | (raw[1][j] & m1) | (raw[2][j] & m2) | (x & m3);
        v[j] = wi_value(__uint_as_float(x), scale, bias);
      }
      const size_t ok = o + (size_t)k * cells;
      if (BF16) {
        uint16_t* out = reinterpret_cast<uint16_t*>(a.out);
        uint16_t b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = wi_bf16(v[j]);
        if (VEC) {   // col0 + 3 < out_w and ok % 4 == 0
          u32x2 w = {(uint32_t)b[0] | ((uint32_t)b[1] << 16), (uint32_t)b[2] | ((uint32_t)b[3] << 16)};
          *reinterpret_cast<u32x2*>(out + ok) = w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (g.col0 + j < a.source.out_w) out[ok + j] = b[j];
        }
      } else {
        float* out = reinterpret_cast<float*>(a.out);
        if (VEC) {
          f32x4 w = {v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(out + ok) = w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (g.col0 + j < a.source.out_w) out[ok + j] = v[j];
        }
      }
    }
  });
}

}  // namespace

extern "C" void mre_launch_warp_inputs(const WarpInputArgs* a, hipStream_t stream) {
  typedef void (*Kernel)(WarpInputArgs);
  static const Kernel table[8] = {k_warp_inputs<false, false, false>, k_warp_inputs<false, false, true>,
                                  k_warp_inputs<false, true, false>,  k_warp_inputs<false, true, true>,
                                  k_warp_inputs<true, false, false>,  k_warp_inputs<true, false, true>,
                                  k_warp_inputs<true, true, false>,   k_warp_inputs<true, true, true>};
  wp_launch(table[(a->vec ? 4 : 0) + (a->colour ? 2 : 0) + (a->bf16 ? 1 : 0)], *a, stream);
}

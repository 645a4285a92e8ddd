// Network-ready inputs on the device: the gather of mre_warp_maps (wp_cell, csrc/mre_warp_point.h, bit for bit) written
// as the tensor a convolution consumes -- planar [samples][channels][out_h][out_w], every channel a colour byte or the
// height of the source cell times a scale plus a bias (wi_value, csrc/mre_warp_input_point.h), in float32 or bfloat16
// (wi_bf16) -- in one launch, with no intermediate.
//
//   k_warp_inputs      the decomposition of k_warp_maps: one workgroup of 256 lanes per (sample, tile of 16 rows x 64
//                      columns); a lane owns 4 consecutive columns of one row.  The six floats, the map index and the
//                      channel table (by value in the kernel's arguments) are the same in every lane of the workgroup.
//                      A lane issues all its gathers (4 heights, 12 colour bytes) before it uses the first; an invalid
//                      cell reads cell 0 of map 0 (n >= 1), which exists, and drops it for a raw 0.0f.  Then it walks
//                      the channels in a rolled loop -- a trip reads its entry of the table by scalar loads from the
//                      kernel's arguments; unrolled, the table's 48 scalars were hoisted and spilled, and it was slower
//                       -- and stores a lane's 4 cells of each plane.
//                      VEC: out_w % 4 == 0 and out aligned, so a lane's 4 cells are all inside the output or all outside
//                      and it stores 16 B (float32) or 8 B (bfloat16) per channel.  Otherwise every element is stored on
//                      its own, at any element offset.
//                      COLOUR: a channel names a colour byte; compiled in, so that no branch stands among the gathers.
//                      BF16: the element type of out.
//
// Bound by memory: 8 B (4 B without colour) read per valid cell, channels x element size written per cell.  Output
// offsets are formed in 64 bits: 147 456 crops x 6 channels x 64 x 64 is 3.6e9 elements.  No LDS, no atomics, no
// workspace.  Every output element is written exactly once, by the lane that owns it.
#include "mre_warp_inputs.h"

namespace {

constexpr int NT = 256;   // threads per workgroup: WP_TILE_H rows x (WP_TILE_W / 4) lanes
static_assert(NT == WP_TILE_H * (WP_TILE_W / 4), "a lane owns 4 columns of one row of the tile");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool VEC, bool COLOUR, bool BF16>
__global__ void __launch_bounds__(NT) k_warp_inputs(WarpInputArgs a) {
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
    uint8_t rgb[12] = {};
#pragma unroll
    for (int j = 0; j < 4; j++) hz[j] = a.hmap[base + off[j]];
    if (COLOUR) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint8_t* px = a.cmap + 3 * (base + off[j]);
        rgb[3 * j] = px[0]; rgb[3 * j + 1] = px[1]; rgb[3 * j + 2] = px[2];
      }
    }
    // raw values, as bits: the colour bytes as floats (exact), the height; 0.0f where the source cell does not exist
    uint32_t raw[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int q = 0; q < 3; q++) raw[q][j] = valid[j] ? __float_as_uint((float)rgb[3 * j + q]) : 0u;
      raw[3][j] = valid[j] ? __float_as_uint(hz[j]) : 0u;
    }
    const size_t o = (size_t)s * a.channels * cells + (size_t)row * a.out_w + col0;   // channel 0; plane k is k * cells on
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
            if (col0 + j < a.out_w) out[ok + j] = b[j];
        }
      } else {
        float* out = reinterpret_cast<float*>(a.out);
        if (VEC) {
          f32x4 w = {v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(out + ok) = w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (col0 + j < a.out_w) out[ok + j] = v[j];
        }
      }
    }
  }
}

}  // namespace

extern "C" void mre_launch_warp_inputs(const WarpInputArgs* a, hipStream_t stream) {
  const size_t items = (size_t)a->samples * a->tiles_x * a->tiles_y;
  const dim3 grid((uint32_t)(items < WP_MAX_GRID ? items : WP_MAX_GRID));
  typedef void (*Kernel)(WarpInputArgs);
  static const Kernel table[8] = {k_warp_inputs<false, false, false>, k_warp_inputs<false, false, true>,
                                  k_warp_inputs<false, true, false>,  k_warp_inputs<false, true, true>,
                                  k_warp_inputs<true, false, false>,  k_warp_inputs<true, false, true>,
                                  k_warp_inputs<true, true, false>,   k_warp_inputs<true, true, true>};
  const Kernel k = table[(a->vec ? 4 : 0) + (a->colour ? 2 : 0) + (a->bf16 ? 1 : 0)];
  hipLaunchKernelGGL(k, grid, dim3(NT), 0, stream, *a);
}

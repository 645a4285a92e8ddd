// The Transporter place head on the device (include/mre.h, mre_correlate): per env an implicit GEMM
//   logit[r][y][x] = sum_d sum_i sum_j scene[d][y + i - crop/2][x + j - crop/2] * kern[r][d][i][j]
// on v_mfma_f32_16x16x32_bf16, and the largest sum of the env with its flat index.  The main loop described below is
// cr_forward / cr_slice of mre_correlate_core.h, which the training kernels (mre_correlate_grad.hip) share; with the pivot
// at crop - 1 - crop/2 and flipped kernels this kernel is also grad_scene.
//
//   k_correlate<RT, VK>   one workgroup of 256 lanes (4 waves) per (env, tile of 16 pixel rows x 32 pixel columns); a wave
//                      owns 8 consecutive columns of the 16 rows.
//                      A rows are rotations, RT tiles of 16 (R padded; a padded row repeats the last one and reaches no output).
//                      The 32 reduction indices of one MFMA are 32 taps j at fixed (d, i); a lane's 8 taps of `kern` are
//                      16 contiguous bytes, loaded from global memory (they are the same for every workgroup of the env
//                      and stay in the L2).  VK: crop % 8 == 0 and kern 16-byte aligned, so they are one load; otherwise
//                      eight 2-byte loads, masked past the row's end pair by pair (crop is even), with the same values.
//                      The 16 B columns of an MFMA are the 16 pixel ROWS of the tile at one pixel column x, not 16
//                      columns: the B fragment of lane (row lr, k group g) is then patch[lr + i][x + j0 + 8 g .. + 7] of
//                      the scene patch in LDS, and its offset inside an aligned 16-byte slot, x mod 8, is the same in
//                      every lane.  A wave's 8 columns x = 0 .. 7 therefore take their 8 fragments from ONE window of 16
//                      elements per lane -- two aligned ds_read_b128 -- shifted by a compile-time x: the even x are
//                      register quadruples of the window as they lie, the odd ones quadruples of the 7 dwords
//                      (win[t], win[t + 1]) >> 16.  No 2-byte LDS read, no second copy.  Per (d, i, j0) a wave issues
//                      2 LDS reads, RT global loads (one step ahead of their use), 7 shifts and 8 RT MFMAs.
//                      The patch of one depth slice (16 + crop - 1 rows x 96 columns, zero outside the scene) is staged
//                      per d; its row pitch of 14 slots of 16 bytes puts the 16 lanes that ds_read_b128 serves in one
//                      cycle on 16 different slots.  Rows i and chunks j0 whose every tap lies outside the scene are
//                      skipped: their terms are exact zeros.
//                      Epilogue: the logits, if asked for (8 consecutive columns per lane and rotation: two 16-byte
//                      stores, or one in bfloat16, where the width and the alignment allow, else element by element),
//                      and the workgroup's best (value, flat index) to its own slot of the workspace.
//   k_correlate_best   one wave per env reduces that env's slots.
//
// The reductions go by `better` (csrc/mre_head.h).  No atomics; every output element and every slot is written exactly once.
// Offsets into logits and kern are formed in 64 bits.
#include "mre_correlate_core.h"

namespace {

template <int RT, bool VK>
__global__ void __launch_bounds__(NT, 2) k_correlate(CorrelateArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t patch[PROWS * PITCH];
  __shared__ Best red[NT / 64];
  const CrLane l = cr_lane();
  const uint32_t t = l.t, lane = l.lane, lr = l.lr, g = l.g;
  const int wv = l.wv;
  const int R = (int)a.rot, H = (int)a.h, W = (int)a.w;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  // one workgroup per (tile, env): blockIdx.x the tile, y and z the env (no loop over items: what it would keep alive
  // across the body does not fit the scalar registers)
  const uint32_t e = env_index(), tile = blockIdx.x;
  if (e >= a.n) return;
  {
    const int y0 = (int)(tile / a.tiles_x) * CR_TILE_H, x0 = (int)(tile % a.tiles_x) * CR_TILE_W;
    const int xw = x0 + 8 * wv;   // the wave's first pixel column
    f32x4 acc[RT][8];
    cr_forward<RT, VK>(acc, patch, a, e, y0, x0, t, wv, lr, g);
    // epilogue: lane (lr, g) holds rotations 16 rt + 4 g + q, pixel row y0 + lr, columns xw .. xw + 7
    const int y = y0 + (int)lr;
    Best b = {-__builtin_inff(), NO_INDEX};
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * rt + 4 * (int)g + q;
        if (r >= R || y >= H || xw >= W) continue;
        float v[8];
#pragma unroll
        for (int p = 0; p < 8; p++) v[p] = acc[rt][p][q];
        const int flat = (r * H + y) * W + xw;
        if (a.logits) {
          const size_t o = ((size_t)e * R * H + (size_t)(r * H + y)) * W + xw;
          if (a.bf16) {
            uint16_t* out = reinterpret_cast<uint16_t*>(a.logits) + o;
            if (a.vec_out) {
              const u32x4 u = {(uint32_t)wi_bf16(v[0]) | ((uint32_t)wi_bf16(v[1]) << 16),
                               (uint32_t)wi_bf16(v[2]) | ((uint32_t)wi_bf16(v[3]) << 16),
                               (uint32_t)wi_bf16(v[4]) | ((uint32_t)wi_bf16(v[5]) << 16),
                               (uint32_t)wi_bf16(v[6]) | ((uint32_t)wi_bf16(v[7]) << 16)};
              *reinterpret_cast<u32x4*>(out) = u;
            } else {
#pragma unroll
              for (int p = 0; p < 8; p++)
                if (xw + p < W) out[p] = wi_bf16(v[p]);
            }
          } else {
            float* out = reinterpret_cast<float*>(a.logits) + o;
            if (a.vec_out) {
              *reinterpret_cast<f32x4*>(out) = f32x4{v[0], v[1], v[2], v[3]};
              *reinterpret_cast<f32x4*>(out + 4) = f32x4{v[4], v[5], v[6], v[7]};
            } else {
#pragma unroll
              for (int p = 0; p < 8; p++)
                if (xw + p < W) out[p] = v[p];
            }
          }
        }
#pragma unroll
        for (int p = 0; p < 8; p++)
          if (xw + p < W && better(v[p], flat + p, b.v, b.i)) { b.v = v[p]; b.i = flat + p; }
      }
    }
    if (a.best_index) {
      b = wave_best(b);
      if (lane == 0) red[wv] = b;
      __syncthreads();
      if (t == 0) {
#pragma unroll
        for (int k = 1; k < NT / 64; k++)
          if (better(red[k].v, red[k].i, b.v, b.i)) b = red[k];
        reinterpret_cast<Best*>(a.workspace)[(size_t)e * tiles + tile] = b;
      }
    }
  }
}

// the slots of an env in strided partials per lane, then the butterfly
__global__ void __launch_bounds__(64) k_correlate_best(CorrelateArgs a) {
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  for (uint32_t e = blockIdx.x; e < a.n; e += gridDim.x) {
    const Best* slots = reinterpret_cast<const Best*>(a.workspace) + (size_t)e * tiles;
    Best b = {-__builtin_inff(), NO_INDEX};
    for (uint32_t s = threadIdx.x; s < tiles; s += 64) b = best_merge(b, slots[s]);
    b = wave_best(b);
    if (threadIdx.x == 0) {
      // no cell was better than the start only if every sum is a NaN: the first cell stands, as the statement has it, with
      // NaN as its value (the pick head returns the first logit there: -inf is a valid logit for it)
      const bool none = b.i == NO_INDEX;
      a.best_index[e] = none ? 0 : (int64_t)b.i;
      a.best_value[e] = none ? __builtin_nanf("") : b.v;
    }
  }
}

}  // namespace

extern "C" void mre_launch_correlate(const CorrelateArgs* a, hipStream_t stream) {
#define CR_FORWARD(RT, VK) k_correlate<RT, VK>
  static void (*const table[8])(CorrelateArgs) = CR_TABLE(CR_FORWARD);
  hipLaunchKernelGGL(table[cr_which(a->rot, a->vec_kern)], env_grid(a->tiles_x * a->tiles_y, a->n), dim3(NT), 0, stream, *a);   // at most 32 768 tiles
  if (a->best_index) hipLaunchKernelGGL(k_correlate_best, wave_per_env_grid(a->n), dim3(64), 0, stream, *a);
}

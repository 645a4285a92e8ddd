// Training the Transporter place head on the device (include/mre.h, mre_correlate_loss and after it): the
// softmax cross-entropy of every env's logits against a target cell, its gradient g with respect to the logits, and the
// gradients of any g with respect to the scene and the kernels.  All of them are the implicit GEMM of
// csrc/mre_correlate_core.h with the operands in different roles; no logits are ever stored.
//
//   k_correlate_soft<RT, VK, G>   the forward's launch shape and sums (cr_forward), with another epilogue.
//                      G = false: each lane keeps (max, sum of exp(l - max)) of its sums; merged across the wave by
//                      shuffles, across the 4 waves in LDS, into the workgroup's 8-byte slot.  The one lane that holds
//                      cell `target` writes target_logit.
//                      G = true: the sums are computed again and g = weight * (exp(l - lse) - [cell == target]) stored as
//                      bfloat16 by the rule of the forward's bfloat16 logits.
//   k_correlate_lse    one wave per env merges that env's slots in a fixed order: lse, loss, and NaN for a target outside.
//   k_correlate_flip   kt[e][d][r][i][j] = kern[e][r][d][c - 1 - i][c - 1 - j] into the workspace; grad_scene is then the
//                      FORWARD kernel (mre_launch_correlate) with g as the scene of depth R, kt as the D "rotations" and
//                      the pivot at c - 1 - c/2.  One A tile of which D rows are real.
//   k_correlate_grad_kern<RT, VK>   one workgroup per (env, d, tile of 16 tap rows x 32 tap columns, split).  The A rows
//                      are rotations again, but the reduction runs over PIXELS: the A operand of a slice is a block of at
//                      most 64 x 64 cells of g[e][r] (row pitch w, rotation stride h w), and the patch is the scene plane
//                      d with its origin moved by the block, so that tap (I, J) meets scene[yb + y + I - c/2][xb + x + J - c/2]
//                      at cell (y, x) of the block.  Where the forward loops over depth slices this loops over the blocks.
//                      A workgroup takes the block rows split, split + S, ...  with S = cr_split(h) workgroups per tile, so
//                      that a small batch still fills the card.  S = 1 writes grad_kern itself; otherwise the partial tiles
//                      go to the workspace and
//   k_correlate_sum    adds the S partials of every element in the order 0 .. S - 1.
//
// S depends on h alone and every workgroup serves one env: an env's bytes do not depend on n or on its place in the batch.
// No atomics; every output element, slot and workspace element that is read is written exactly once.
#include <string.h>

#include "mre_correlate_core.h"

namespace {

// NOT the pick head's merge (acc_merge of csrc/mre_attend.hip).  sa and sb are formed in statements of their own and then
// added: two multiplies and an add under -ffp-contract=on, where the pick head's single expression is a multiply and a fused
// multiply-add; one shared merge would change the last bit of one head's lse.  An empty pair returns (m, 0) early; non-finite
// sums are left unspecified here (the pick head substitutes 0 for a -inf max, -inf being a valid logit there).
__device__ __forceinline__ Soft soft_merge(Soft a, Soft b) {
  const float m = fmaxf(a.m, b.m);
  if (m == -__builtin_inff()) return Soft{m, 0.f};
  const float sa = a.s * ex2((a.m - m) * L2E), sb = b.s * ex2((b.m - m) * L2E);
  return Soft{m, sa + sb};
}

__device__ __forceinline__ Soft wave_soft(Soft v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = soft_merge(v, Soft{__shfl_xor(v.m, m, 64), __shfl_xor(v.s, m, 64)});
  return v;
}

template <int RT, bool VK, bool G>
__global__ void __launch_bounds__(NT, 2) k_correlate_soft(CorrelateLossArgs s) {
  __shared__ __attribute__((aligned(16))) uint16_t patch[PROWS * PITCH];
  __shared__ Soft red[NT / 64];
  const CorrelateArgs& a = s.fwd;
  const CrLane l = cr_lane();
  const uint32_t t = l.t, lane = l.lane, lr = l.lr, g = l.g;
  const int wv = l.wv;
  const int R = (int)a.rot, H = (int)a.h, W = (int)a.w;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  const uint32_t e = env_index(), tile = blockIdx.x;
  if (e >= a.n) return;
  const int y0 = (int)(tile / a.tiles_x) * CR_TILE_H, x0 = (int)(tile % a.tiles_x) * CR_TILE_W;
  const int xw = x0 + 8 * wv;
  f32x4 acc[RT][8];
  cr_forward<RT, VK>(acc, patch, a, e, y0, x0, t, wv, lr, g);
  // lane (lr, g) holds rotations 16 rt + 4 g + q, pixel row y0 + lr, columns xw .. xw + 7
  const int y = y0 + (int)lr;
  const int64_t tgt = s.target[e];
  if (G) {
    const float lse = s.lse_in[e], wgt = s.weight ? s.weight[e] : 1.f;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * rt + 4 * (int)g + q;
        if (r >= R || y >= H || xw >= W) continue;
        const int flat = (r * H + y) * W + xw;
        uint16_t v[8];
#pragma unroll
        for (int p = 0; p < 8; p++) {
          const float hit = (int64_t)(flat + p) == tgt ? 1.f : 0.f;
          v[p] = wi_bf16(wgt * (ex2((acc[rt][p][q] - lse) * L2E) - hit));
        }
        uint16_t* out = s.g + ((size_t)e * R * H + (size_t)(r * H + y)) * W + xw;
        if (s.vec_g) {
          const u32x4 u = {(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                           (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16)};
          *reinterpret_cast<u32x4*>(out) = u;
        } else {
#pragma unroll
          for (int p = 0; p < 8; p++)
            if (xw + p < W) out[p] = v[p];
        }
      }
    }
  } else {
    Soft b = {-__builtin_inff(), 0.f};
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * rt + 4 * (int)g + q;
        if (r >= R || y >= H || xw >= W) continue;
#pragma unroll
        for (int p = 0; p < 8; p++)
          if (xw + p < W) b.m = fmaxf(b.m, acc[rt][p][q]);
      }
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * rt + 4 * (int)g + q;
        if (r >= R || y >= H || xw >= W) continue;
        const int flat = (r * H + y) * W + xw;
#pragma unroll
        for (int p = 0; p < 8; p++)
          if (xw + p < W) {
            b.s += ex2((acc[rt][p][q] - b.m) * L2E);
            if ((int64_t)(flat + p) == tgt) s.target_logit[e] = acc[rt][p][q];
          }
      }
    b = wave_soft(b);
    if (lane == 0) red[wv] = b;
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int k = 1; k < NT / 64; k++) b = soft_merge(b, red[k]);
      reinterpret_cast<Soft*>(a.workspace)[(size_t)e * tiles + tile] = b;
    }
  }
}

// the slots of an env in strided partials per lane, then the butterfly (the pick head's k_attend_merge goes 0 .. S - 1)
__global__ void __launch_bounds__(64) k_correlate_lse(CorrelateLossArgs s) {
  const CorrelateArgs& a = s.fwd;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  const int64_t cells = (int64_t)a.rot * a.h * a.w;
  for (uint32_t e = blockIdx.x; e < a.n; e += gridDim.x) {
    const Soft* slots = reinterpret_cast<const Soft*>(a.workspace) + (size_t)e * tiles;
    Soft b = {-__builtin_inff(), 0.f};
    for (uint32_t k = threadIdx.x; k < tiles; k += 64) b = soft_merge(b, slots[k]);
    b = wave_soft(b);
    if (threadIdx.x == 0) {
      // the lane that held the target cell has written its logit; nobody has for a target outside: what is read then is
      // never used (soft_finish answers NaN), and the NaN is stored over it
      const SoftEnd f = soft_finish(b, s.target[e], cells, s.target_logit[e]);
      s.lse[e] = f.lse;
      s.target_logit[e] = f.target_logit;
      s.loss[e] = f.loss;
    }
  }
}

__global__ void __launch_bounds__(256) k_correlate_flip(CorrelateGradArgs a, uint16_t* kt) {
  const size_t R = a.rot, D = a.depth, c = a.crop, total = (size_t)a.n * R * D * c * c;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const size_t j = o % c, i = (o / c) % c, r = (o / (c * c)) % R, d = (o / (c * c * R)) % D, e = o / (c * c * R * D);
    kt[o] = a.kern[(((e * R + r) * D + d) * c + (c - 1 - i)) * c + (c - 1 - j)];
  }
}

template <int RT, bool VK>
__global__ void __launch_bounds__(NT, 2) k_correlate_grad_kern(CorrelateGradArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t patch[PROWS * PITCH];
  const uint32_t t = threadIdx.x, lane = t & 63;   // (not cr_lane: its order of lr and g renames this kernel's registers)
  const int wv = __builtin_amdgcn_readfirstlane((int)(t >> 6));
  const uint32_t lr = lane & 15, g = lane >> 4;
  const int R = (int)a.rot, D = (int)a.depth, H = (int)a.h, W = (int)a.w, c = (int)a.crop, half = c / 2;
  const uint32_t e = env_index();
  if (e >= a.n) return;
  const uint32_t tj = cr_tiles(a.crop, CR_TILE_W), ntile = tj * cr_tiles(a.crop, CR_TILE_H), split = cr_split(a.h);
  const uint32_t tile = blockIdx.x % ntile;
  const int d = (int)((blockIdx.x / ntile) % a.depth), sp = (int)(blockIdx.x / (ntile * a.depth));
  const int I0 = (int)(tile / tj) * CR_TILE_H, J0 = (int)(tile % tj) * CR_TILE_W;   // the tile's first tap
  const uint16_t* plane = a.scene + ((size_t)e * D + d) * H * W;
  const uint16_t* g_e = a.g + (size_t)e * R * H * W;
  f32x4 acc[RT][8];
  cr_zero<RT>(acc);
  size_t rot_off[RT];
#pragma unroll
  for (int rt = 0; rt < RT; rt++) rot_off[rt] = (size_t)min(16 * rt + (int)lr, R - 1) * H * W;
  const int brows = (H + CR_BLOCK - 1) / CR_BLOCK, bcols = (W + CR_BLOCK - 1) / CR_BLOCK;
  for (int by = sp; by < brows; by += (int)split) {
    const int yb = by * CR_BLOCK, bh = min(CR_BLOCK, H - yb), oy = I0 + yb - half;
    int i_lo, i_hi;
    cr_rows(oy, bh, H, i_lo, i_hi);
    for (int bx = 0; bx < bcols; bx++) {
      const int xb = bx * CR_BLOCK, bw = min(CR_BLOCK, W - xb);
      cr_slice<RT, VK, false>(acc, patch, plane, H, W, oy, J0 + xb - half, g_e + (size_t)yb * W + xb, rot_off, W, bh, bw,
                              i_lo, i_hi, t, wv, lr, g);
    }
  }
  // lane (lr, g) holds rotations 16 rt + 4 g + q, tap row I0 + lr, tap columns J0 + 8 wv .. + 7
  const size_t per = (size_t)R * D * c * c;
  float* dst = split > 1 ? reinterpret_cast<float*>(a.workspace) + ((size_t)e * split + sp) * per : a.out + (size_t)e * per;
  const int I = I0 + (int)lr, Jw = J0 + 8 * wv;
#pragma unroll
  for (int rt = 0; rt < RT; rt++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int r = 16 * rt + 4 * (int)g + q;
      if (r >= R || I >= c) continue;
      float* row = dst + (((size_t)r * D + d) * c + I) * c + Jw;
#pragma unroll
      for (int p = 0; p < 8; p++)
        if (Jw + p < c) row[p] = acc[rt][p][q];
    }
}

__global__ void __launch_bounds__(256) k_correlate_sum(CorrelateGradArgs a) {
  const size_t per = (size_t)a.rot * a.depth * a.crop * a.crop, total = (size_t)a.n * per;
  const uint32_t split = cr_split(a.h);
  const float* ws = reinterpret_cast<const float*>(a.workspace);
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const size_t e = o / per, k = o - e * per;
    float v = ws[e * split * per + k];
    for (uint32_t sp = 1; sp < split; sp++) v += ws[(e * split + sp) * per + k];
    a.out[o] = v;
  }
}

uint32_t flat_grid(size_t total) {
  const size_t b = (total + 255) / 256;
  return (uint32_t)(b < MAX_GRID ? b : MAX_GRID);
}

template <bool G>
void launch_soft(const CorrelateLossArgs* s, hipStream_t stream) {
  const CorrelateArgs& a = s->fwd;
#define CR_SOFT(RT, VK) k_correlate_soft<RT, VK, G>
  static void (*const table[8])(CorrelateLossArgs) = CR_TABLE(CR_SOFT);
  hipLaunchKernelGGL(table[cr_which(a.rot, a.vec_kern)], env_grid(a.tiles_x * a.tiles_y, a.n), dim3(NT), 0, stream, *s);
}

}  // namespace

extern "C" void mre_launch_correlate_loss(const CorrelateLossArgs* s, hipStream_t stream) {
  launch_soft<false>(s, stream);
  hipLaunchKernelGGL(k_correlate_lse, wave_per_env_grid(s->fwd.n), dim3(64), 0, stream, *s);
}

extern "C" void mre_launch_correlate_dlogits(const CorrelateLossArgs* s, hipStream_t stream) { launch_soft<true>(s, stream); }

extern "C" void mre_launch_correlate_grad_scene(const CorrelateGradArgs* a, hipStream_t stream) {
  uint16_t* kt = reinterpret_cast<uint16_t*>(a->workspace);
  hipLaunchKernelGGL(k_correlate_flip, dim3(flat_grid((size_t)a->n * a->rot * a->depth * a->crop * a->crop)), dim3(256), 0,
                     stream, *a, kt);
  CorrelateArgs f;
  memset(&f, 0, sizeof(f));
  f.scene = a->g; f.kern = kt; f.logits = a->out;
  f.n = a->n; f.rot = a->depth; f.depth = a->rot; f.h = a->h; f.w = a->w; f.crop = a->crop;
  f.pivot = a->crop - 1 - a->crop / 2;
  f.tiles_x = cr_tiles(a->w, CR_TILE_W); f.tiles_y = cr_tiles(a->h, CR_TILE_H);
  f.vec_kern = a->crop % 8 == 0 ? 1u : 0u;   // the workspace is 16-byte aligned
  f.vec_out = a->vec_out;
  mre_launch_correlate(&f, stream);
}

extern "C" void mre_launch_correlate_grad_kern(const CorrelateGradArgs* a, hipStream_t stream) {
#define CR_GRAD_KERN(RT, VK) k_correlate_grad_kern<RT, VK>
  static void (*const table[8])(CorrelateGradArgs) = CR_TABLE(CR_GRAD_KERN);
  const uint32_t split = cr_split(a->h);
  const uint32_t x = cr_tiles(a->crop, CR_TILE_W) * cr_tiles(a->crop, CR_TILE_H) * a->depth * split;
  hipLaunchKernelGGL(table[cr_which(a->rot, a->vec_g)], env_grid(x, a->n), dim3(NT), 0, stream, *a);
  if (split > 1)
    hipLaunchKernelGGL(k_correlate_sum, dim3(flat_grid((size_t)a->n * a->rot * a->depth * a->crop * a->crop)), dim3(256), 0,
                       stream, *a);
}

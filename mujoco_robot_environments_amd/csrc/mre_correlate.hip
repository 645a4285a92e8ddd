// The Transporter place head on the device (include/mre.h, mre_correlate): per env an implicit GEMM
//   logit[r][y][x] = sum_d sum_i sum_j scene[d][y + i - crop/2][x + j - crop/2] * kern[r][d][i][j]
// on v_mfma_f32_16x16x32_bf16, and the largest sum of the env with its flat index.
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
// `Better` is a total order on (value, index) -- greater value, then lower index -- so the reductions give the first
// occurrence of the maximum in whatever order they combine; a NaN is never better than anything.  No atomics; every
// output element and every slot is written exactly once.  Offsets into logits and kern are formed in 64 bits.
#include "mre_correlate.h"

#include "mre_warp_input_point.h"

namespace {

constexpr int NT = 256;
constexpr int PITCH = 112;                              // bf16 elements of a patch row: 14 slots of 16 bytes
constexpr int PCOLS = 96;                               // staged columns: 24 (wave) + 32 (j0) + 24 (g) + 15 (window) + 1
constexpr int PROWS = CR_TILE_H + CR_MAX_CROP - 1;      // 79
constexpr int NO_INDEX = 0x7FFFFFFF;
constexpr uint32_t MAX_GRID_Y = 65535, MAX_GRID = 1u << 20;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Best {
  float v;
  int i;
};

__device__ __forceinline__ bool better(float v2, int i2, float v1, int i1) { return v2 > v1 || (v2 == v1 && i2 < i1); }

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float v = __shfl_xor(b.v, m, 64);
    const int i = __shfl_xor(b.i, m, 64);
    if (better(v, i, b.v, b.i)) { b.v = v; b.i = i; }
  }
  return b;
}

__device__ __forceinline__ bf16x8 frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const u32x4 u = {a, b, c, d};
  return __builtin_bit_cast(bf16x8, u);
}

// A fragments of one step: the lane's 8 taps j .. j + 7 of row `krow` of each of its RT rotations.  A tap past the row's
// end is zero (the scene values it would meet are real).  A padded rotation reads the last real one's row, clamped by
// rot_off: its sums reach no output, so they need not be zero.
template <int RT, bool VK>
__device__ __forceinline__ void load_rows(bf16x8 (&fa)[RT], const uint16_t* krow, const size_t (&rot_off)[RT], int j, int c) {
#pragma unroll
  for (int rt = 0; rt < RT; rt++) {
    if (VK) {
      const bool ok = j < c;
      const u32x4 v = *reinterpret_cast<const u32x4*>(krow + rot_off[rt] + (ok ? j : 0));
      fa[rt] = frag(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
    } else {
      // c and j are even: the taps of a pair are inside the row together or not at all (four masks, not eight)
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool ok = j + 2 * k < c;
        const uint16_t* src = krow + rot_off[rt] + (ok ? j + 2 * k : 0);
        const uint32_t lo = src[0], hi = src[1];
        v[k] = ok ? (lo | (hi << 16)) : 0u;
      }
      fa[rt] = frag(v[0], v[1], v[2], v[3]);
    }
  }
}

template <int RT, bool VK>
__global__ void __launch_bounds__(NT, 2) k_correlate(CorrelateArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t patch[PROWS * PITCH];
  __shared__ Best red[NT / 64];
  const uint32_t t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(t >> 6));   // the same in every lane of a wave: scalar
  const uint32_t lr = lane & 15, g = lane >> 4;
  const int R = (int)a.rot, D = (int)a.depth, H = (int)a.h, W = (int)a.w, c = (int)a.crop, half = c / 2;
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  const int prow_n = CR_TILE_H + c - 1;
  // one workgroup per (tile, env): blockIdx.x the tile, y and z the env (no loop over items: what it would keep alive
  // across the body does not fit the scalar registers)
  const uint32_t e = blockIdx.z * gridDim.y + blockIdx.y, tile = blockIdx.x;
  if (e >= a.n) return;
  {
    const int y0 = (int)(tile / a.tiles_x) * CR_TILE_H, x0 = (int)(tile % a.tiles_x) * CR_TILE_W;
    const int xw = x0 + 8 * wv;   // the wave's first pixel column
    const uint16_t* scene_e = a.scene + (size_t)e * D * H * W;
    const uint16_t* kern_e = a.kern + (size_t)e * R * D * c * c;
    // taps that can meet the scene: rows i of the tile, chunks j0 of the wave
    const int i_lo = max(0, half - y0 - (CR_TILE_H - 1)), i_hi = min(c, H + half - y0);
    f32x4 acc[RT][8];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int p = 0; p < 8; p++) acc[rt][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    // rows of kern of this lane's rotations (clamped: a padded rotation reads a real row)
    size_t rot_off[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) rot_off[rt] = (size_t)min(16 * rt + (int)lr, R - 1) * D * c * c;
    for (int d = 0; d < D; d++) {
      __syncthreads();   // the patch of the slice before is no longer read
      const uint16_t* plane = scene_e + (size_t)d * H * W;
      for (int q = (int)t; q < prow_n * (PCOLS / 2); q += NT) {
        const int pr = q / (PCOLS / 2), pc = 2 * (q - pr * (PCOLS / 2));
        const int y = y0 - half + pr, x = x0 - half + pc;
        const bool row_in = y >= 0 && y < H;
        const bool in0 = row_in && x >= 0 && x < W, in1 = row_in && x + 1 >= 0 && x + 1 < W;
        const uint16_t* src = plane + (size_t)(row_in ? y : 0) * W;   // a cell outside reads cell 0 of a row that exists
        const uint32_t lo = src[in0 ? x : 0], hi = src[in1 ? x + 1 : 0];
        *reinterpret_cast<uint32_t*>(patch + pr * PITCH + pc) = (in0 ? lo : 0u) | ((in1 ? hi : 0u) << 16);
      }
      __syncthreads();
      const uint16_t* kd = kern_e + (size_t)d * c * c;
      // the steps (i, j0) of this slice, flattened, so that the kernel rows of a step are loaded one step ahead of the
      // MFMAs that use them (a chunk the wave skips still loads: the loads stay in bounds and cost nothing beside it)
      const int chunks = (c + 31) / 32, steps = (i_hi - i_lo) * chunks;
      bf16x8 fa[RT];
      if (steps > 0) load_rows<RT, VK>(fa, kd + (size_t)i_lo * c, rot_off, 8 * (int)g, c);
      for (int s = 0, i = i_lo, j0 = 0; s < steps; s++) {
        int i_next = i, j_next = j0 + 32;
        if (j_next >= c) { j_next = 0; i_next = i + 1; }
        bf16x8 fn[RT];
        load_rows<RT, VK>(fn, kd + (size_t)min(i_next, i_hi - 1) * c, rot_off, j_next + 8 * (int)g, c);
        // the chunk's taps meet columns xw + j0 - half .. + 38 of the scene
        if (xw + j0 - half + 38 >= 0 && xw + j0 - half < W) {
          const uint16_t* prow = patch + ((int)lr + i) * PITCH + 8 * wv + 8 * (int)g + j0;
          const u32x4 w0 = *reinterpret_cast<const u32x4*>(prow);
          const u32x4 w1 = *reinterpret_cast<const u32x4*>(prow + 8);
          const uint32_t win[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
          for (int p = 0; p < 8; p++) {
            const int q = p >> 1;
            bf16x8 fb;
            if (p & 1)
              fb = frag(__builtin_amdgcn_alignbit(win[q + 1], win[q], 16), __builtin_amdgcn_alignbit(win[q + 2], win[q + 1], 16),
                        __builtin_amdgcn_alignbit(win[q + 3], win[q + 2], 16), __builtin_amdgcn_alignbit(win[q + 4], win[q + 3], 16));
            else
              fb = frag(win[q], win[q + 1], win[q + 2], win[q + 3]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
              acc[rt][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[rt], fb, acc[rt][p], 0, 0, 0);
          }
        }
#pragma unroll
        for (int rt = 0; rt < RT; rt++) fa[rt] = fn[rt];
        i = i_next; j0 = j_next;
      }
    }
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

__global__ void __launch_bounds__(64) k_correlate_best(CorrelateArgs a) {
  const uint32_t tiles = a.tiles_x * a.tiles_y;
  for (uint32_t e = blockIdx.x; e < a.n; e += gridDim.x) {
    const Best* slots = reinterpret_cast<const Best*>(a.workspace) + (size_t)e * tiles;
    Best b = {-__builtin_inff(), NO_INDEX};
    for (uint32_t s = threadIdx.x; s < tiles; s += 64) {
      const Best o = slots[s];
      if (better(o.v, o.i, b.v, b.i)) b = o;
    }
    b = wave_best(b);
    if (threadIdx.x == 0) {
      // no cell was better than the start only if every sum is a NaN: the first cell stands, as the statement has it
      const bool none = b.i == NO_INDEX;
      a.best_index[e] = none ? 0 : (int64_t)b.i;
      a.best_value[e] = none ? __builtin_nanf("") : b.v;
    }
  }
}

}  // namespace

extern "C" void mre_launch_correlate(const CorrelateArgs* a, hipStream_t stream) {
  const uint32_t gy = a->n < MAX_GRID_Y ? a->n : MAX_GRID_Y;
  const dim3 grid(a->tiles_x * a->tiles_y, gy, (a->n + gy - 1) / gy);   // at most 32 768 tiles; n < 2^31 envs
  typedef void (*Kernel)(CorrelateArgs);
  static const Kernel table[8] = {k_correlate<1, false>, k_correlate<1, true>, k_correlate<2, false>, k_correlate<2, true>,
                                  k_correlate<3, false>, k_correlate<3, true>, k_correlate<4, false>, k_correlate<4, true>};
  const int rt = ((int)a->rot + 15) / 16;
  hipLaunchKernelGGL(table[2 * (rt - 1) + (a->vec_kern ? 1 : 0)], grid, dim3(NT), 0, stream, *a);
  if (a->best_index)
    hipLaunchKernelGGL(k_correlate_best, dim3(a->n < MAX_GRID ? a->n : MAX_GRID), dim3(64), 0, stream, *a);
}

// The inner loop of the place head's implicit GEMM (csrc/mre_correlate.hip has the layout in full), shared by the forward
// correlation, the softmax epilogues and both gradients (csrc/mre_correlate_grad.hip).  One call of cr_slice adds
//   acc[rt][p][q] += sum_{i < rows} sum_{j < cols} plane[oy + lr + i][ox + 8 wv + p + j] * A[16 rt + 4 g + q][i][j]
// for the workgroup's tile of 16 output rows (lr) x 32 output columns (8 per wave wv, p of them per lane), where
//   plane   a bf16 map [H][W]; cells outside count as 0.  (oy, ox) is the patch origin: the cell the tile's first output
//           meets at tap (0, 0).  The forward passes tile origin - pivot.
//   A       the lane's RT operand rows, A[m][i][j] = a0[rot_off[rt] + i * pitch + j]: `rot_off` the rotation stride times
//           the (clamped) row index, `pitch` the row pitch, rows x cols (each at most 64) the valid extent.
// Patch staging, the 16-element window, the alignbit fragments, the one-step-ahead A rows and the skipping of steps that
// meet only zeros are the same for every user, and so is the order of the additions.
#ifndef MRE_CORRELATE_CORE_H
#define MRE_CORRELATE_CORE_H
#include "mre_correlate.h"
#include "mre_head.h"

namespace {

constexpr int NT = 256;
constexpr int PITCH = 112;                              // bf16 elements of a patch row: 14 slots of 16 bytes
constexpr int PCOLS = 96;                               // staged columns: 24 (wave) + 32 (j0) + 24 (g) + 15 (window) + 1
constexpr int PROWS = CR_TILE_H + CR_MAX_CROP - 1;      // 79

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const u32x4 u = {a, b, c, d};
  return __builtin_bit_cast(bf16x8, u);
}

// A fragments of one step: the lane's 8 taps j .. j + 7 of row `krow` of each of its RT rotations.  A tap past the row's
// end is zero (the scene values it would meet are real).  A padded rotation reads the last real one's row, clamped by
// rot_off: its sums reach no output, so they need not be zero.
// VK: c % 8 == 0 and the row 16-byte aligned: one load.  PAIRS: c is even, so the taps of a pair (j is even) are inside
// the row together or not at all (four masks, not eight).
template <int RT, bool VK, bool PAIRS>
__device__ __forceinline__ void load_rows(bf16x8 (&fa)[RT], const uint16_t* krow, const size_t (&rot_off)[RT], int j, int c) {
#pragma unroll
  for (int rt = 0; rt < RT; rt++) {
    if (VK) {
      const bool ok = j < c;
      const u32x4 v = *reinterpret_cast<const u32x4*>(krow + rot_off[rt] + (ok ? j : 0));
      fa[rt] = frag(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
    } else {
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool ok = j + 2 * k < c;
        const uint16_t* src = krow + rot_off[rt] + (ok ? j + 2 * k : 0);
        if (PAIRS) {
          const uint32_t lo = src[0], hi = src[1];
          v[k] = ok ? (lo | (hi << 16)) : 0u;
        } else {   // the second element of a pair may lie past an odd row's end: it reads the first again
          const bool ok1 = j + 2 * k + 1 < c;
          const uint32_t lo = src[0], hi = src[ok1 ? 1 : 0];
          v[k] = (ok ? lo : 0u) | ((ok1 ? hi : 0u) << 16);
        }
      }
      fa[rt] = frag(v[0], v[1], v[2], v[3]);
    }
  }
}

// i_lo .. i_hi: the rows i whose taps can meet the plane (cr_rows); every lane of the workgroup calls this together
template <int RT, bool VK, bool PAIRS>
__device__ __forceinline__ void cr_slice(f32x4 (&acc)[RT][8], uint16_t* patch, const uint16_t* plane, int H, int W, int oy,
                                         int ox, const uint16_t* a0, const size_t (&rot_off)[RT], int pitch, int rows,
                                         int cols, int i_lo, int i_hi, uint32_t t, int wv, uint32_t lr, uint32_t g) {
  const int prow_n = CR_TILE_H + rows - 1;
  const int xo = ox + 8 * wv;   // the cell the wave's first column meets at tap column 0
  __syncthreads();   // the patch of the slice before is no longer read
  for (int q = (int)t; q < prow_n * (PCOLS / 2); q += NT) {
    const int pr = q / (PCOLS / 2), pc = 2 * (q - pr * (PCOLS / 2));
    const int y = oy + pr, x = ox + pc;
    const bool row_in = y >= 0 && y < H;
    const bool in0 = row_in && x >= 0 && x < W, in1 = row_in && x + 1 >= 0 && x + 1 < W;
    const uint16_t* src = plane + (size_t)(row_in ? y : 0) * W;   // a cell outside reads cell 0 of a row that exists
    const uint32_t lo = src[in0 ? x : 0], hi = src[in1 ? x + 1 : 0];
    *reinterpret_cast<uint32_t*>(patch + pr * PITCH + pc) = (in0 ? lo : 0u) | ((in1 ? hi : 0u) << 16);
  }
  __syncthreads();
  // the steps (i, j0) of this slice, flattened, so that the A rows of a step are loaded one step ahead of the
  // MFMAs that use them (a chunk the wave skips still loads: the loads stay in bounds and cost nothing beside it)
  const int chunks = (cols + 31) / 32, steps = (i_hi - i_lo) * chunks;
  bf16x8 fa[RT];
  if (steps > 0) load_rows<RT, VK, PAIRS>(fa, a0 + (size_t)i_lo * pitch, rot_off, 8 * (int)g, cols);
  for (int s = 0, i = i_lo, j0 = 0; s < steps; s++) {
    int i_next = i, j_next = j0 + 32;
    if (j_next >= cols) { j_next = 0; i_next = i + 1; }
    bf16x8 fn[RT];
    load_rows<RT, VK, PAIRS>(fn, a0 + (size_t)min(i_next, i_hi - 1) * pitch, rot_off, j_next + 8 * (int)g, cols);
    // the chunk's taps meet columns xo + j0 .. + 38 of the plane
    if (xo + j0 + 38 >= 0 && xo + j0 < W) {
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

// The rows i < rows whose taps can meet a plane of H rows from a tile whose patch origin is oy: some output row lr < 16
// has 0 <= oy + lr + i < H.
__device__ __forceinline__ void cr_rows(int oy, int rows, int H, int& i_lo, int& i_hi) {
  i_lo = max(0, -oy - (CR_TILE_H - 1));
  i_hi = min(rows, H - oy);
}

template <int RT>
__device__ __forceinline__ void cr_zero(f32x4 (&acc)[RT][8]) {
#pragma unroll
  for (int rt = 0; rt < RT; rt++)
#pragma unroll
    for (int p = 0; p < 8; p++) acc[rt][p] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The forward sums of env e for the tile at (y0, x0): lane (lr, g) of wave wv ends with acc[rt][p][q], the sum of rotation
// 16 rt + 4 g + q at pixel row y0 + lr and column x0 + 8 wv + p.  The patch of one depth slice is staged per d.
template <int RT, bool VK>
__device__ __forceinline__ void cr_forward(f32x4 (&acc)[RT][8], uint16_t* patch, const CorrelateArgs& a, uint32_t e, int y0,
                                           int x0, uint32_t t, int wv, uint32_t lr, uint32_t g) {
  const int R = (int)a.rot, D = (int)a.depth, H = (int)a.h, W = (int)a.w, c = (int)a.crop, half = (int)a.pivot;
  const uint16_t* scene_e = a.scene + (size_t)e * D * H * W;
  const uint16_t* kern_e = a.kern + (size_t)e * R * D * c * c;
  // taps that can meet the scene: rows i of the tile (chunks j0 of the wave: cr_slice)
  int i_lo, i_hi;
  cr_rows(y0 - half, c, H, i_lo, i_hi);
  cr_zero<RT>(acc);
  // rows of kern of this lane's rotations (clamped: a padded rotation reads a real row)
  size_t rot_off[RT];
#pragma unroll
  for (int rt = 0; rt < RT; rt++) rot_off[rt] = (size_t)min(16 * rt + (int)lr, R - 1) * D * c * c;
  for (int d = 0; d < D; d++)
    cr_slice<RT, VK, true>(acc, patch, scene_e + (size_t)d * H * W, H, W, y0 - half, x0 - half, kern_e + (size_t)d * c * c,
                           rot_off, c, c, c, i_lo, i_hi, t, wv, lr, g);
}

// Where a lane stands in its workgroup of 4 waves: lane (lr, g) of wave wv holds rows 16 rt + 4 g + q of the A operand at
// output row lr and the wave's 8 output columns.
struct CrLane {
  uint32_t t, lane, lr, g;
  int wv;   // the same in every lane of a wave: scalar
};

__device__ __forceinline__ CrLane cr_lane(void) {
  const uint32_t t = threadIdx.x, lane = t & 63, g = lane >> 4, lr = lane & 15;
  return CrLane{t, lane, lr, g, __builtin_amdgcn_readfirstlane((int)(t >> 6))};
}

// The eight instantiations K(RT, VK) of a kernel template (K a macro that names one, as CR_SOFT of csrc/mre_correlate_grad.hip
// does), and which of them serves `rot` rows of A (RT tiles of 16) with the wide access or without
#define CR_TABLE(K) {K(1, false), K(1, true), K(2, false), K(2, true), K(3, false), K(3, true), K(4, false), K(4, true)}
inline int cr_which(uint32_t rot, uint32_t vk) { return 2 * (((int)rot + 15) / 16 - 1) + (vk ? 1 : 0); }

}  // namespace
#endif

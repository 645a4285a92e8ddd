// The Transporter pick head on the device (include/mre.h, mre_attend and after it): from the logits
// [n][K][h][w] an attention network has written, per env the best cell, the softmax cross-entropy against a target cell,
// and the gradient of that loss with respect to the logits.  One read of the logits for the first two, one read and one
// write for the third.
//
//   k_attend<BF16, BEST, SOFT>   one workgroup per (split, env).  An env's cells are cut into chunks of AT_CHUNK = 2048; lane t
//                      owns the cells 8 t .. 8 t + 7 of every chunk as 16-byte vectors (one of bfloat16; of float32 two,
//                      cells 4 t .. and 1024 + 4 t ..), whatever the env's address.  The S = at_split(cells) workgroups of an
//                      env take contiguous runs of chunks (at_first).  A vector is ONE 16-byte load where the env's first
//                      byte is 16-byte aligned and the vector lies inside the env; any other vector is read element by
//                      element, cells past the end counting as -inf, into the same registers: the same bits.  The loads of
//                      AT_AHEAD = 3 chunks (a whole split at the workload's 320 x 240) are issued before the first is used;
//                      they are non-temporal, the logits being read once.  Each lane
//                      carries (max, sum of exp2((l - max) log2 e)) and (best value, best index) over its vectors in order;
//                      they are merged across the wave by __shfl_xor, across the 4 waves in LDS, into the workgroup's
//                      16-byte slot of the workspace.
//   k_attend_merge     one wave per env merges the env's slots in the order 0 .. S - 1 and writes every output.
//   k_attend_dlogits<BF16>   the launch shape and the loads of k_attend; g = weight * (exp(l - lse) - [cell == target])
//                      stored by the rule of the loads (a 16-byte store where g's env is aligned, else element by element).
//
// S depends on the number of cells alone, every workgroup serves one env and a lane's cells do not depend on an address: an
// env's bytes depend neither on n nor on its place in the batch nor on its alignment.  No atomics; every output element and
// every slot is written exactly once.  `better` is the total order of csrc/mre_head.h (greater value, then lower index).
//
// -inf is a valid logit (a masked cell).  The running max of a lane that has met nothing finite is -inf, and -inf - -inf
// would be a NaN: every rescale subtracts `ms`, the max with -inf replaced by 0, so that an all -inf prefix contributes
// exp2(-inf) = 0 and nothing else.
#include "mre_attend.h"
#include "mre_head.h"

namespace {

constexpr uint32_t NINF_F32 = 0xFF800000u, NINF_BF16 = 0xFF80u;

__device__ __forceinline__ float as_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t as_u32(float f) { return __builtin_bit_cast(uint32_t, f); }

struct Acc {   // what a lane, a wave, a workgroup and a 16-byte slot hold: ((-inf, 0), (-inf, NO_INDEX)) is the empty set
  Soft s;
  Best b;
};
constexpr Acc ACC_EMPTY = {{-__builtin_inff(), 0.f}, {-__builtin_inff(), NO_INDEX}};

// BEST / SOFT: which half is live; the other keeps the empty set and costs nothing.
// The SOFT half is NOT the place head's soft_merge (csrc/mre_correlate_grad.hip): the sum is ONE expression, a multiply and a
// fused multiply-add under -ffp-contract=on, where soft_merge rounds both products; and a -inf max is replaced by 0, not
// returned early.  One shared merge would change the last bit of one head's lse.
template <bool BEST, bool SOFT>
__device__ __forceinline__ Acc acc_merge(Acc a, Acc b) {
  Acc r = a;
  if (SOFT) {
    const float m = fmaxf(a.s.m, b.s.m);
    const float ms = m == -__builtin_inff() ? 0.f : m;
    r.s.m = m;
    r.s.s = a.s.s * ex2((a.s.m - ms) * L2E) + b.s.s * ex2((b.s.m - ms) * L2E);
  }
  if (BEST) r.b = best_merge(a.b, b.b);
  return r;
}

template <bool XOR, typename T>
__device__ __forceinline__ T from_lane(T v, int from) { return XOR ? __shfl_xor(v, from, 64) : __shfl(v, from, 64); }

template <bool BEST, bool SOFT, bool XOR>
__device__ __forceinline__ Acc acc_lane(Acc v, int from) {
  Acc o = v;
  if (SOFT) o.s = Soft{from_lane<XOR>(v.s.m, from), from_lane<XOR>(v.s.s, from)};
  if (BEST) o.b = Best{from_lane<XOR>(v.b.v, from), from_lane<XOR>(v.b.i, from)};
  return o;
}

// the 16 bytes of the vector that starts at cell i0 of the env at `base`: -inf where a cell lies past the env's end
template <bool BF16>
__device__ __forceinline__ u32x4 at_raw(const char* base, bool aligned, uint32_t i0, uint32_t cells) {
  constexpr uint32_t VEC = BF16 ? 8 : 4;
  if (aligned && i0 + VEC <= cells) {
    const u32x4* src = reinterpret_cast<const u32x4*>(base + (size_t)i0 * (BF16 ? 2 : 4));
    return __builtin_nontemporal_load(src);   // read once: measured 7 % faster at n = 4096 than the default policy
  }
  u32x4 u;
  if (BF16) {
    const uint16_t* src = reinterpret_cast<const uint16_t*>(base);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t k = i0 + 2 * q;
      const uint32_t lo = k < cells ? (uint32_t)src[k] : NINF_BF16, hi = k + 1 < cells ? (uint32_t)src[k + 1] : NINF_BF16;
      u[q] = lo | (hi << 16);
    }
  } else {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(base);
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] = i0 + q < cells ? src[i0 + q] : NINF_F32;
  }
  return u;
}

template <bool BF16>
__device__ __forceinline__ void at_values(float (&v)[BF16 ? 8 : 4], u32x4 u) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    if (BF16) {
      v[2 * q] = as_f32(u[q] << 16);
      v[2 * q + 1] = as_f32(u[q] & 0xFFFF0000u);
    } else {
      v[q] = as_f32(u[q]);
    }
  }
}

// the first cell of vector j of lane t in chunk c (below 2^31 + AT_CHUNK: unsigned)
template <bool BF16>
__device__ __forceinline__ uint32_t at_cell(uint32_t c, uint32_t j, uint32_t t) {
  return c * AT_CHUNK + (j * AT_NT + t) * (BF16 ? 8 : 4);
}

// online, per vector (the place head makes two passes over its registers)
template <int VEC, bool BEST, bool SOFT>
__device__ __forceinline__ void at_update(Acc& a, const float (&v)[VEC], uint32_t i0) {
  float vm = v[0];
#pragma unroll
  for (int p = 1; p < VEC; p++) vm = fmaxf(vm, v[p]);
  if (BEST && vm > a.b.v) {   // rare after a lane's first vectors; the cells in rising order, so strictly greater is enough
#pragma unroll
    for (int p = 0; p < VEC; p++)
      if (v[p] > a.b.v) { a.b.v = v[p]; a.b.i = (int)(i0 + p); }
  }
  if (SOFT) {
    const float m = fmaxf(a.s.m, vm);
    const float ms = m == -__builtin_inff() ? 0.f : m;
    float s = a.s.s * ex2((a.s.m - ms) * L2E);
#pragma unroll
    for (int p = 0; p < VEC; p++) s += ex2((v[p] - ms) * L2E);
    a.s.m = m;
    a.s.s = s;
  }
}

constexpr uint32_t AT_AHEAD = 3;   // chunks whose loads a lane issues before it uses the first: a whole split of the workload

template <bool BF16, bool BEST, bool SOFT>
__global__ void __launch_bounds__(AT_NT) k_attend(AttendArgs a) {
  constexpr int VEC = BF16 ? 8 : 4, VPL = AT_LANE / VEC;
  __shared__ Acc red[AT_NT / 64];
  const uint32_t t = threadIdx.x, e = env_index(), sp = blockIdx.x;
  if (e >= a.n) return;
  const uint32_t cells = a.cells, chunks = at_chunks(cells), S = at_split(cells);
  const uint32_t c0 = at_first(chunks, S, sp), c1 = at_first(chunks, S, sp + 1);
  const char* base = reinterpret_cast<const char*>(a.logits) + (size_t)e * cells * (BF16 ? 2 : 4);
  const bool aligned = ((uintptr_t)base & 15) == 0;
  Acc acc = ACC_EMPTY;
  for (uint32_t c = c0; c < c1; c += AT_AHEAD) {
    u32x4 raw[AT_AHEAD][VPL];
#pragma unroll
    for (uint32_t k = 0; k < AT_AHEAD; k++)
#pragma unroll
      for (uint32_t j = 0; j < VPL; j++) {
        const uint32_t i0 = at_cell<BF16>(c + k, j, t);
        if (c + k < c1 && i0 < cells) raw[k][j] = at_raw<BF16>(base, aligned, i0, cells);
      }
#pragma unroll
    for (uint32_t k = 0; k < AT_AHEAD; k++)
#pragma unroll
      for (uint32_t j = 0; j < VPL; j++) {
        const uint32_t i0 = at_cell<BF16>(c + k, j, t);
        if (c + k < c1 && i0 < cells) {
          float v[VEC];
          at_values<BF16>(v, raw[k][j]);
          at_update<VEC, BEST, SOFT>(acc, v, i0);
        }
      }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc = acc_merge<BEST, SOFT>(acc, acc_lane<BEST, SOFT, true>(acc, m));
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 1; k < AT_NT / 64; k++) acc = acc_merge<BEST, SOFT>(acc, red[k]);
    reinterpret_cast<Acc*>(a.workspace)[(size_t)e * S + sp] = acc;
  }
}

__device__ __forceinline__ float at_elem(const void* logits, bool bf16, size_t i) {
  if (bf16) return as_f32((uint32_t)reinterpret_cast<const uint16_t*>(logits)[i] << 16);
  return reinterpret_cast<const float*>(logits)[i];
}

template <bool BEST, bool SOFT>
__global__ void __launch_bounds__(64) k_attend_merge(AttendArgs a) {
  const uint32_t S = at_split(a.cells);
  for (uint32_t e = blockIdx.x; e < a.n; e += gridDim.x) {
    const Acc* slots = reinterpret_cast<const Acc*>(a.workspace) + (size_t)e * S;
    const Acc mine = threadIdx.x < S ? slots[threadIdx.x] : ACC_EMPTY;
    Acc b = ACC_EMPTY;
    // in the order 0 .. S - 1, each slot broadcast from its lane (the place head takes strided partials, then a butterfly)
    for (uint32_t k = 0; k < S; k++) b = acc_merge<BEST, SOFT>(b, acc_lane<BEST, SOFT, false>(mine, (int)k));
    if (threadIdx.x == 0) {
      const size_t first = (size_t)e * a.cells;
      if (BEST) {
        // no cell was better than the start only if none is above -inf: the first cell stands, as the statement has it, with
        // its own logit as the value (the place head returns NaN there)
        const bool none = b.b.i == NO_INDEX;
        a.best_index[e] = none ? 0 : (int64_t)b.b.i;
        a.best_value[e] = none ? at_elem(a.logits, a.bf16, first) : b.b.v;
      }
      if (SOFT) {
        const int64_t tgt = a.target[e];
        const size_t at = soft_inside(tgt, a.cells) ? (size_t)tgt : 0;   // (a target outside reads the first cell, on purpose and unused)
        const SoftEnd f = soft_finish(b.s, tgt, a.cells, at_elem(a.logits, a.bf16, first + at));
        a.lse[e] = f.lse;
        a.target_logit[e] = f.target_logit;
        a.loss[e] = f.loss;
      }
    }
  }
}

template <bool BF16>
__global__ void __launch_bounds__(AT_NT) k_attend_dlogits(AttendGradArgs a) {
  constexpr int VEC = BF16 ? 8 : 4, VPL = AT_LANE / VEC, ESIZE = BF16 ? 2 : 4;
  const uint32_t t = threadIdx.x, e = env_index(), sp = blockIdx.x;
  if (e >= a.n) return;
  const uint32_t cells = a.cells, chunks = at_chunks(cells), S = at_split(cells);
  const uint32_t c0 = at_first(chunks, S, sp), c1 = at_first(chunks, S, sp + 1);
  const char* base = reinterpret_cast<const char*>(a.logits) + (size_t)e * cells * ESIZE;
  char* out = reinterpret_cast<char*>(a.g) + (size_t)e * cells * ESIZE;
  const bool aligned = ((uintptr_t)base & 15) == 0, out_aligned = ((uintptr_t)out & 15) == 0;
  const int64_t tgt = a.target[e];
  const uint32_t hit_cell = tgt >= 0 && tgt < (int64_t)cells ? (uint32_t)tgt : 0xFFFFFFFFu;
  const float lse = a.lse[e], wgt = a.weight ? a.weight[e] : 1.f;
  const bool dead = lse == -__builtin_inff();   // every cell is -inf: g = 0, not exp(-inf + inf)
  for (uint32_t c = c0; c < c1; c += AT_AHEAD) {
    u32x4 raw[AT_AHEAD][VPL];
#pragma unroll
    for (uint32_t k = 0; k < AT_AHEAD; k++)
#pragma unroll
      for (uint32_t j = 0; j < VPL; j++) {
        const uint32_t i0 = at_cell<BF16>(c + k, j, t);
        if (c + k < c1 && i0 < cells) raw[k][j] = at_raw<BF16>(base, aligned, i0, cells);
      }
#pragma unroll
    for (uint32_t k = 0; k < AT_AHEAD; k++)
#pragma unroll
      for (uint32_t j = 0; j < VPL; j++) {
        const uint32_t i0 = at_cell<BF16>(c + k, j, t);
        if (!(c + k < c1 && i0 < cells)) continue;
        float v[VEC];
        at_values<BF16>(v, raw[k][j]);
#pragma unroll
        for (int p = 0; p < VEC; p++) {
          const float pr = dead ? 0.f : ex2((v[p] - lse) * L2E);   // (`dead` is this head's alone: -inf is no sum of the place head)
          const float hit = !dead && i0 + p == hit_cell ? 1.f : 0.f;
          v[p] = wgt * (pr - hit);
        }
        u32x4 u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (BF16) u[q] = (uint32_t)wi_bf16(v[2 * q]) | ((uint32_t)wi_bf16(v[2 * q + 1]) << 16);
          else u[q] = as_u32(v[q]);
        }
        if (out_aligned && i0 + VEC <= cells) {
          *reinterpret_cast<u32x4*>(out + (size_t)i0 * ESIZE) = u;
        } else if (BF16) {
          uint16_t* dst = reinterpret_cast<uint16_t*>(out);
#pragma unroll
          for (int p = 0; p < VEC; p++)
            if (i0 + p < cells) dst[i0 + p] = (uint16_t)(u[p >> 1] >> (16 * (p & 1)));
        } else {
          uint32_t* dst = reinterpret_cast<uint32_t*>(out);
#pragma unroll
          for (int p = 0; p < VEC; p++)
            if (i0 + p < cells) dst[i0 + p] = u[p];
        }
      }
  }
}

}  // namespace

extern "C" void mre_launch_attend(const AttendArgs* a, hipStream_t stream) {
  typedef void (*Kernel)(AttendArgs);
  // [bf16][which]: the decision alone, the loss alone, both
  static const Kernel table[2][3] = {{k_attend<false, true, false>, k_attend<false, false, true>, k_attend<false, true, true>},
                                     {k_attend<true, true, false>, k_attend<true, false, true>, k_attend<true, true, true>}};
  const int which = !a->target ? 0 : (!a->best_index ? 1 : 2);
  hipLaunchKernelGGL(table[a->bf16 ? 1 : 0][which], env_grid(at_split(a->cells), a->n), dim3(AT_NT), 0, stream, *a);
  static const Kernel merge[3] = {k_attend_merge<true, false>, k_attend_merge<false, true>, k_attend_merge<true, true>};
  hipLaunchKernelGGL(merge[which], wave_per_env_grid(a->n), dim3(64), 0, stream, *a);
}

extern "C" void mre_launch_attend_dlogits(const AttendGradArgs* a, hipStream_t stream) {
  const dim3 grid = env_grid(at_split(a->cells), a->n);
  if (a->bf16) hipLaunchKernelGGL(k_attend_dlogits<true>, grid, dim3(AT_NT), 0, stream, *a);
  else hipLaunchKernelGGL(k_attend_dlogits<false>, grid, dim3(AT_NT), 0, stream, *a);
}

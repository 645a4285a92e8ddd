// Frame labels on the device: what props_info (tasks/rearrangement.py:227-295 of the reference) takes from a segmentation
// image, for every env and every label of a small id range in one pass over the image -- the PASCAL-VOC box of the
// label's pixels (get_bbox, :254-268), their count, the sums of their coordinates (the centroid) and the smallest depth
// among them.
//
//   k_labels_init   every output element: box -1, count and sums 0, zmin +inf
//   k_seg_labels    one workgroup per piece of one env's image.  A lane reads 16 label bytes with one aligned 16-byte
//                   load (the env's first and last bytes up to the 16-byte boundaries are read as bytes by the
//                   workgroup of piece 0); a dword with no byte in id0 .. id0 + nid - 1 -- almost all of them -- costs
//                   nine integer instructions and a skipped branch.  The pixels that hit go to per-workgroup
//                   accumulators in LDS (integer atomics), depth is fetched for them alone (the hits of a vector
//                   together), and a workgroup that saw a label adds its accumulators to the outputs with integer
//                   global atomics.
//
// Nothing is summed in floating point and min / max / add of integers commute, so the outputs are the same bits
// whatever order the workgroups arrive in.  The outputs double as the cross-workgroup accumulators: -1 is the largest
// unsigned value, so an unsigned atomic min into xmin / ymin and a signed atomic max into xmax / ymax leave -1 exactly
// where no pixel was seen; a finite non-negative float orders like its bit pattern, so zmin is an unsigned min below
// the bits of +inf.
#include "mre_labels.h"

namespace {

constexpr int NT = 256;   // threads per workgroup
constexpr int UNROLL = 4; // 16-byte loads a lane has in flight

// 0x80 in every byte of v that lies in id0 .. id0 + nid - 1 (1 <= nid <= 128), 0 elsewhere: a bytewise v - id0 without
// borrows between bytes (Hacker's Delight 2-18), then bytewise d < nid.  c = id0 in every byte, k = 0x80 - nid likewise.
__device__ __forceinline__ uint32_t bytes_in_range(uint32_t v, uint32_t c, uint32_t k) {
  constexpr uint32_t H = 0x80808080u;
  const uint32_t d = ((v | H) - (c & ~H)) ^ ((v ^ ~c) & H);
  const uint32_t t = (d & ~H) + k;   // bit 7 of a byte: its low seven bits are >= nid
  return ~(t | d) & H;
}

struct Acc {   // one workgroup's accumulators
  uint32_t xmin[LAB_MAX_IDS], ymin[LAB_MAX_IDS], xmax[LAB_MAX_IDS], ymax[LAB_MAX_IDS], count[LAB_MAX_IDS], z[LAB_MAX_IDS];
  unsigned long long sx[LAB_MAX_IDS], sy[LAB_MAX_IDS];
};

// zbits: the pixel's depth as bits (read only when the call has depth)
__device__ __forceinline__ void add_pixel(Acc& s, const LabelArgs& a, uint32_t k, uint32_t x, uint32_t y, uint32_t zbits) {
  atomicMin(&s.xmin[k], x);
  atomicMin(&s.ymin[k], y);
  atomicMax(&s.xmax[k], x);
  atomicMax(&s.ymax[k], y);
  atomicAdd(&s.count[k], 1u);
  atomicAdd(&s.sx[k], (unsigned long long)x);
  atomicAdd(&s.sy[k], (unsigned long long)y);
  if (a.depth) atomicMin(&s.z[k], zbits);
}

// the four pixels p .. p + 3 of an env's image, their depths in zb[0 .. 3]
__device__ __forceinline__ void add_word(Acc& s, const LabelArgs& a, uint32_t v, uint32_t p, const uint32_t* zb) {
  uint32_t y = p / a.w, x = p - y * a.w;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t k = ((v >> (8 * j)) & 0xFFu) - a.id0;
    if (k < a.nid) add_pixel(s, a, k, x, y, zb[j]);
    if (++x == a.w) { x = 0; ++y; }
  }
}

__global__ void __launch_bounds__(NT) k_labels_init(LabelArgs a) {
  const size_t total = (size_t)a.n * a.nid;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    unsigned long long* st = a.stats + i * 7;
    st[0] = st[1] = st[2] = st[3] = ~0ull;
    st[4] = st[5] = st[6] = 0ull;
    if (a.zmin) a.zmin[i] = 0x7F800000u;
  }
}

__global__ void __launch_bounds__(NT) k_seg_labels(LabelArgs a) {
  __shared__ Acc s;
  const uint32_t t = threadIdx.x;
  const uint32_t c = a.id0 * 0x01010101u, kk = (0x80u - a.nid) * 0x01010101u;
  const size_t items = (size_t)a.n * a.chunks;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = (uint32_t)(item / a.chunks), piece = (uint32_t)(item - (size_t)e * a.chunks);
    if (t < LAB_MAX_IDS) {
      s.xmin[t] = s.ymin[t] = ~0u;
      s.xmax[t] = s.ymax[t] = s.count[t] = 0u;
      s.z[t] = 0x7F800000u;
      s.sx[t] = s.sy[t] = 0ull;
    }
    __syncthreads();
    const size_t base = (size_t)e * a.hw;
    const uint8_t* img = a.seg + base;
    // pixels [0, head) and [tail, hw) are read as bytes, [head, tail) as nv aligned 16-byte vectors
    uint32_t head = (uint32_t)((16u - ((uintptr_t)img & 15u)) & 15u);
    if (head > a.hw) head = a.hw;
    const uint32_t nv = (a.hw - head) >> 4, tail = head + 16u * nv;
    const uint32_t per = (nv + a.chunks - 1) / a.chunks;
    const uint32_t v0 = piece * per, v1 = min(v0 + per, nv);
    for (uint32_t v = v0 + t; v < v1; v += NT * UNROLL) {
      uint4 q[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; u++)   // a vector past the piece re-reads the piece's last one and is not used
        q[u] = *reinterpret_cast<const uint4*>(img + head + 16u * (size_t)min(v + u * NT, v1 - 1));
#pragma unroll
      for (int u = 0; u < UNROLL; u++) {
        if (v + u * NT >= v1) break;
        const uint32_t m0 = bytes_in_range(q[u].x, c, kk), m1 = bytes_in_range(q[u].y, c, kk),
                       m2 = bytes_in_range(q[u].z, c, kk), m3 = bytes_in_range(q[u].w, c, kk);
        if (m0 | m1 | m2 | m3) {
          const uint32_t p = head + 16u * (v + u * NT);
          const uint32_t wv[4] = {q[u].x, q[u].y, q[u].z, q[u].w}, mv[4] = {m0, m1, m2, m3};
          uint32_t zb[16];   // the depths of the vector's hits, loaded together: one wait, not one per pixel
#pragma unroll
          for (int j = 0; j < 16; j++)
            zb[j] = (a.depth && ((mv[j >> 2] >> (8 * (j & 3) + 7)) & 1u)) ? __float_as_uint(a.depth[base + p + j]) : 0x7F800000u;
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (mv[i]) add_word(s, a, wv[i], p + 4 * i, &zb[4 * i]);
        }
      }
    }
    if (piece == 0) {   // at most 15 bytes before the first vector and 15 after the last
      uint32_t p = a.hw;
      if (t < head) p = t;
      else if (t >= 32 && t - 32 < a.hw - tail) p = tail + (t - 32);
      if (p < a.hw) {
        const uint32_t k = (uint32_t)img[p] - a.id0;
        if (k < a.nid) add_pixel(s, a, k, p % a.w, p / a.w, a.depth ? __float_as_uint(a.depth[base + p]) : 0u);
      }
    }
    __syncthreads();
    if (t < a.nid && s.count[t]) {
      unsigned long long* st = a.stats + ((size_t)e * a.nid + t) * 7;
      atomicMin(&st[0], (unsigned long long)s.xmin[t]);
      atomicMin(&st[1], (unsigned long long)s.ymin[t]);
      atomicMax(reinterpret_cast<long long*>(&st[2]), (long long)s.xmax[t]);
      atomicMax(reinterpret_cast<long long*>(&st[3]), (long long)s.ymax[t]);
      atomicAdd(&st[4], (unsigned long long)s.count[t]);
      atomicAdd(&st[5], s.sx[t]);
      atomicAdd(&st[6], s.sy[t]);
      if (a.zmin) atomicMin(&a.zmin[(size_t)e * a.nid + t], s.z[t]);
    }
    __syncthreads();   // the accumulators are reset for the next item
  }
}

}  // namespace

extern "C" void mre_launch_seg_labels(const LabelArgs* a, hipStream_t stream) {
  const size_t outs = (size_t)a->n * a->nid, items = (size_t)a->n * a->chunks;
  const size_t g0 = (outs + NT - 1) / NT;
  hipLaunchKernelGGL(k_labels_init, dim3((uint32_t)(g0 < LAB_MAX_GRID ? g0 : LAB_MAX_GRID)), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_seg_labels, dim3((uint32_t)(items < LAB_MAX_GRID ? items : LAB_MAX_GRID)), dim3(NT), 0, stream, *a);
}

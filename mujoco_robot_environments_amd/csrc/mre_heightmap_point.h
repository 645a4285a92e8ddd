// The per-pixel statement of the orthographic heightmap (csrc/mre_heightmap.hip): a depth pixel pushed
// back through the pinhole model (pixel_2_world, tasks/rearrangement.py:505-531 of the reference) and binned into a
// cell of the map.  No HIP header is included: the device kernel and a host harness built with g++
// (tests/heightmap_host) compile the same text.  Every float32 operation is a statement of its own, so that neither
// -ffp-contract=on nor a host compiler forms a fused multiply-add: the result is defined bit for bit.
#ifndef MRE_HEIGHTMAP_POINT_H
#define MRE_HEIGHTMAP_POINT_H
#include <stdint.h>

#if defined(__HIP__)
#define MRE_HM_HD __host__ __device__
#else
#define MRE_HM_HD
#endif

struct HmGrid {
  float cam[12];     // A row-major (world direction of pixel (u, v, 1) per unit depth), then the camera position
  float lo[3], hi[3];
  float inv_cell, max_depth;
  float out_w, out_h;   // columns (x cells) and rows (y cells) of the map, as floats (<= 4096: exact)
};

struct HmPoint {
  float cx, cy;   // column and row of the cell, before any range check (floats: may be huge or NaN)
  float hz;       // height above lo[2]
  bool valid;
};

MRE_HM_HD inline HmPoint hm_point(const HmGrid& g, float u, float v, float d) {
  float P[3];
  for (int k = 0; k < 3; k++) {
    const float t0 = g.cam[3 * k] * u;
    const float t1 = g.cam[3 * k + 1] * v;
    float s = t0 + t1;
    s = s + g.cam[3 * k + 2];
    const float m = d * s;
    P[k] = g.cam[9 + k] + m;
  }
  const float dx = P[0] - g.lo[0];
  const float dy = P[1] - g.lo[1];
  const float sx = dx * g.inv_cell;
  const float sy = dy * g.inv_cell;
  HmPoint r;
  r.cx = __builtin_floorf(sx);
  r.cy = __builtin_floorf(sy);
  r.hz = P[2] - g.lo[2];
  // NaN and infinite depths fail the comparisons
  r.valid = d > 0.f && d < g.max_depth && r.cx >= 0.f && r.cx < g.out_w && r.cy >= 0.f && r.cy < g.out_h &&
            P[2] >= g.lo[2] && P[2] <= g.hi[2];
  return r;
}

// hz >= +0, so it orders like its bits: the largest key is the highest pixel, and among equal heights the smallest
// source index.  No pixel has key 0 (index < 2^31), which therefore marks an empty cell.
MRE_HM_HD inline unsigned long long hm_key(uint32_t hz_bits, uint32_t index) {
  return ((unsigned long long)hz_bits << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}

// The key of a pixel of one of several views (csrc/mre_heightmap_views.hip): the view (< 16) above the
// index (< 2^28) in the low word, so that among equal heights the smallest view wins and inside it the smallest index.
// View 0 gives hm_key; no pixel has key 0.
MRE_HM_HD inline unsigned long long hm_key_view(uint32_t hz_bits, uint32_t view, uint32_t index) {
  return hm_key(hz_bits, (view << 28) | index);
}
MRE_HM_HD inline uint32_t hm_key_which(unsigned long long key) { return (0xFFFFFFFFu - (uint32_t)key) >> 28; }
MRE_HM_HD inline uint32_t hm_key_index(unsigned long long key) { return (0xFFFFFFFFu - (uint32_t)key) & 0x0FFFFFFFu; }
#endif

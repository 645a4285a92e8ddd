// The per-cell statement of the map warp (csrc/mre_warp.hip): the source cell of an output cell under a
// sample's affine matrix M (OUTPUT cell -> SOURCE cell, row-major 2 x 3), rounded to the nearest cell.  No HIP header is
// included: the device kernel and a host harness built with g++ (tests/warp_host) compile the same text.  Every float32
// operation is a statement of its own, so that neither -ffp-contract=on nor a host compiler forms a fused multiply-add:
// the result is defined bit for bit.
#ifndef MRE_WARP_POINT_H
#define MRE_WARP_POINT_H
#include <stdint.h>

#if defined(__HIP__)
#define MRE_WP_HD __host__ __device__
#else
#define MRE_WP_HD
#endif

struct WpCell {
  float fx, fy;   // column and row of the source cell, before any range check (floats: may be huge or NaN)
  bool valid;
};

// m: the sample's six floats; c, r: output column and row; in_w, in_h: columns and rows of a source map, as floats
// (<= 4096: exact); map_ok: the sample's map index lies inside [0, n)
MRE_WP_HD inline WpCell wp_cell(const float* m, float c, float r, float in_w, float in_h, bool map_ok) {
  WpCell o;
  const float ax = m[0] * c;
  const float bx = m[1] * r;
  float x = ax + bx;
  x = x + m[2];
  x = x + 0.5f;
  o.fx = __builtin_floorf(x);
  const float ay = m[3] * c;
  const float by = m[4] * r;
  float y = ay + by;
  y = y + m[5];
  y = y + 0.5f;
  o.fy = __builtin_floorf(y);
  // NaN, infinite and huge coordinates fail the comparisons; only a valid cell is ever converted to an integer
  o.valid = map_ok && o.fx >= 0.f && o.fx < in_w && o.fy >= 0.f && o.fy < in_h;
  return o;
}

// the index of a valid cell inside its map: (int)fy * in_w + (int)fx  (< 2^24)
MRE_WP_HD inline int32_t wp_from(const WpCell& o, int32_t in_w) { return (int32_t)o.fy * in_w + (int32_t)o.fx; }
#endif

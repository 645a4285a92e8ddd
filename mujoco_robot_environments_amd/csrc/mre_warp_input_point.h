// The per-cell statement of the network inputs (csrc/mre_warp_inputs.hip): the value of one channel of
// one cell from its raw value (a colour byte as a float, a height, or 0.0f where the source cell does not exist), and the
// rounding of that value to bfloat16.  No HIP header is included: the device kernel and a host harness built with g++
// (tests/warp_inputs_host) compile the same text.  Every float32 operation is a statement of its own, so that neither
// -ffp-contract=on nor a host compiler forms a fused multiply-add: the result is defined bit for bit.
#ifndef MRE_WARP_INPUT_POINT_H
#define MRE_WARP_INPUT_POINT_H
#include <stdint.h>

#include "mre_warp_point.h"

// channel value of a raw value v: two roundings
MRE_WP_HD inline float wi_value(float v, float scale, float bias) {
  float t = v * scale;
  t = t + bias;
  return t;
}

// t rounded to bfloat16, nearest and ties to even, on the bits; an overflow rounds to +-inf.  A NaN gives a quiet NaN of
// its sign (the rounding carry could otherwise turn a NaN of a small payload into an infinity).
MRE_WP_HD inline uint16_t wi_bf16(float t) {
  uint32_t bits;
  __builtin_memcpy(&bits, &t, 4);
  const uint32_t rounded = (bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16;
  const uint32_t quiet = (bits >> 16) | 0x0040u;
  return (uint16_t)((bits & 0x7FFFFFFFu) > 0x7F800000u ? quiet : rounded);   // a select, not a branch
}
#endif

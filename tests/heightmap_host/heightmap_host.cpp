// Host harness of the heightmap's per-pixel statement: hm_point (csrc/mre_heightmap_point.h) is code without a device in
// it, so g++ compiles the very text the kernel runs (tests/test_heightmap.py builds this with -O2 -ffp-contract=off) and
// the test holds it to the numpy statement bit for bit.
//
//   heightmap_host IN OUT
// IN:  int32 n, h, w; float32 cam[12], lo[3], hi[3], inv_cell, max_depth, out_w, out_h; float32 depth[n][h][w]
// OUT: per pixel uint32 {bits of cx, bits of cy, bits of hz, valid}
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mujoco_robot_environments_amd/csrc/mre_heightmap_point.h"

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  int32_t dims[3];
  float par[22];
  if (fread(dims, 4, 3, fi) != 3 || fread(par, 4, 22, fi) != 22) return 4;
  HmGrid g;
  memcpy(g.cam, par, 48);
  memcpy(g.lo, par + 12, 12);
  memcpy(g.hi, par + 15, 12);
  g.inv_cell = par[18]; g.max_depth = par[19]; g.out_w = par[20]; g.out_h = par[21];
  const size_t hw = (size_t)dims[1] * dims[2], total = hw * dims[0];
  std::vector<float> depth(total);
  if (fread(depth.data(), 4, total, fi) != total) return 5;
  fclose(fi);
  std::vector<uint32_t> out(4 * total);
  for (size_t i = 0; i < total; i++) {
    const size_t p = i % hw;
    const HmPoint r = hm_point(g, (float)(p % dims[2]), (float)(p / dims[2]), depth[i]);
    out[4 * i] = bits(r.cx); out[4 * i + 1] = bits(r.cy); out[4 * i + 2] = bits(r.hz); out[4 * i + 3] = r.valid ? 1u : 0u;
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 6;
  if (fwrite(out.data(), 4, out.size(), fo) != out.size()) return 7;
  fclose(fo);
  return 0;
}

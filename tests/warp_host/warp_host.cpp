// Host harness of the map warp's per-cell statement: wp_cell and wp_from (csrc/mre_warp_point.h) are code without a
// device in it, so g++ compiles the very text the kernel runs (tests/test_warp.py builds this with -O2 -ffp-contract=off)
// and the test holds it to the numpy statement bit for bit.
//
//   warp_host IN OUT
// IN:  int32 n, in_h, in_w, samples, out_h, out_w; float32 mats[samples][6]; int32 index[samples]
// OUT: per output cell of every sample uint32 {bits of fx, bits of fy, valid, from (-1 where not valid)}
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mujoco_robot_environments_amd/csrc/mre_warp_point.h"

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  int32_t d[6];
  if (fread(d, 4, 6, fi) != 6) return 4;
  const int32_t n = d[0], in_h = d[1], in_w = d[2], samples = d[3], out_h = d[4], out_w = d[5];
  std::vector<float> mats(6 * (size_t)samples);
  std::vector<int32_t> index(samples);
  if (fread(mats.data(), 4, mats.size(), fi) != mats.size()) return 5;
  if (fread(index.data(), 4, index.size(), fi) != index.size()) return 5;
  fclose(fi);
  std::vector<uint32_t> out;
  out.reserve(4 * (size_t)samples * out_h * out_w);
  for (int32_t s = 0; s < samples; s++) {
    const bool map_ok = index[s] >= 0 && index[s] < n;
    for (int32_t r = 0; r < out_h; r++)
      for (int32_t c = 0; c < out_w; c++) {
        const WpCell p = wp_cell(&mats[6 * (size_t)s], (float)c, (float)r, (float)in_w, (float)in_h, map_ok);
        out.push_back(bits(p.fx));
        out.push_back(bits(p.fy));
        out.push_back(p.valid ? 1u : 0u);
        out.push_back(p.valid ? (uint32_t)wp_from(p, in_w) : 0xFFFFFFFFu);
      }
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 6;
  if (fwrite(out.data(), 4, out.size(), fo) != out.size()) return 7;
  fclose(fo);
  return 0;
}

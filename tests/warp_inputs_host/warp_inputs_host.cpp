// Host harness of the network inputs' per-cell statement: wp_cell / wp_from (csrc/mre_warp_point.h) and wi_value /
// wi_bf16 (csrc/mre_warp_input_point.h) are code without a device in it, so g++ compiles the very text the kernel runs
// (tests/test_warp_inputs.py builds this with -O2 -ffp-contract=off) and the test holds it to the numpy statement bit for
// bit.  The loops around them are this file's own: the whole of mre_warp_inputs on the host.
//
//   warp_inputs_host warp IN OUT
// IN:  int32 n, in_h, in_w, samples, out_h, out_w, channels, dtype (0 float32, 1 bfloat16), colour (cmap follows);
//      float32 mats[samples][6]; int32 index[samples]; int32 chan_src[channels]; float32 chan_scale[channels];
//      float32 chan_bias[channels]; float32 hmap[n][in_h][in_w]; uint8 cmap[n][in_h][in_w][3] if colour
// OUT: [samples][channels][out_h][out_w] of float32 or of bfloat16 bits
//
//   warp_inputs_host bf16 IN OUT
// IN: uint32 bit patterns of float32 values.  OUT: uint16 wi_bf16 of each.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mujoco_robot_environments_amd/csrc/mre_warp_input_point.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

static int put(const char* path, const void* p, size_t bytes) {
  FILE* fo = fopen(path, "wb");
  if (!fo) return 6;
  if (bytes && fwrite(p, 1, bytes, fo) != bytes) return 7;
  fclose(fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* fi = fopen(argv[2], "rb");
  if (!fi) return 3;
  if (!strcmp(argv[1], "bf16")) {
    fseek(fi, 0, SEEK_END);
    std::vector<uint32_t> in((size_t)ftell(fi) / 4);
    fseek(fi, 0, SEEK_SET);
    if (!get(fi, in)) return 5;
    std::vector<uint16_t> out(in.size());
    for (size_t i = 0; i < in.size(); i++) {
      float t;
      memcpy(&t, &in[i], 4);
      out[i] = wi_bf16(t);
    }
    return put(argv[3], out.data(), 2 * out.size());
  }
  if (strcmp(argv[1], "warp")) return 2;
  int32_t d[9];
  if (fread(d, 4, 9, fi) != 9) return 4;
  const int32_t n = d[0], in_h = d[1], in_w = d[2], samples = d[3], out_h = d[4], out_w = d[5], channels = d[6];
  const bool bf16 = d[7] != 0, colour = d[8] != 0;
  std::vector<float> mats(6 * (size_t)samples), scale(channels), bias(channels), hmap((size_t)n * in_h * in_w);
  std::vector<int32_t> index(samples), src(channels);
  std::vector<uint8_t> cmap(colour ? 3 * hmap.size() : 0);
  if (!get(fi, mats) || !get(fi, index) || !get(fi, src) || !get(fi, scale) || !get(fi, bias) || !get(fi, hmap) || !get(fi, cmap))
    return 5;
  fclose(fi);
  const size_t cells = (size_t)out_h * out_w, hw = (size_t)in_h * in_w;
  std::vector<float> f32(bf16 ? 0 : (size_t)samples * channels * cells);
  std::vector<uint16_t> b16(bf16 ? (size_t)samples * channels * cells : 0);
  for (int32_t s = 0; s < samples; s++) {
    const bool map_ok = index[s] >= 0 && index[s] < n;
    for (int32_t r = 0; r < out_h; r++)
      for (int32_t c = 0; c < out_w; c++) {
        const WpCell p = wp_cell(&mats[6 * (size_t)s], (float)c, (float)r, (float)in_w, (float)in_h, map_ok);
        const size_t from = p.valid ? (size_t)index[s] * hw + (size_t)wp_from(p, in_w) : 0;
        for (int32_t k = 0; k < channels; k++) {
          float v = 0.f;
          if (p.valid) v = src[k] == 3 ? hmap[from] : (float)cmap[3 * from + src[k]];
          const float t = wi_value(v, scale[k], bias[k]);
          const size_t o = ((size_t)s * channels + k) * cells + (size_t)r * out_w + c;
          if (bf16) b16[o] = wi_bf16(t);
          else f32[o] = t;
        }
      }
  }
  return bf16 ? put(argv[3], b16.data(), 2 * b16.size()) : put(argv[3], f32.data(), 4 * f32.size());
}

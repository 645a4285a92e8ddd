// Host harness of the fused heightmap's key: hm_key_view and its two decoders (csrc/mre_heightmap_point.h) are code without
// a device in it, so g++ compiles the very text the kernel runs (tests/test_heightmap_views.py builds this with -O2
// -ffp-contract=off) and the test checks the order of the keys against the order the statement gives the triples.
//
//   heightmap_views_host IN OUT
// IN:  uint32 {hz bits, view, index} per triple
// OUT: per triple uint64 {hm_key_view, hm_key_which, hm_key_index, hm_key of (hz bits, index)}
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../mujoco_robot_environments_amd/csrc/mre_heightmap_point.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  std::vector<uint32_t> in;
  uint32_t t[3];
  while (fread(t, 4, 3, fi) == 3) in.insert(in.end(), t, t + 3);
  fclose(fi);
  std::vector<unsigned long long> out;
  for (size_t i = 0; i < in.size(); i += 3) {
    const unsigned long long key = hm_key_view(in[i], in[i + 1], in[i + 2]);
    out.push_back(key);
    out.push_back(hm_key_which(key));
    out.push_back(hm_key_index(key));
    out.push_back(hm_key(in[i], in[i + 2]));
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 6;
  if (fwrite(out.data(), 8, out.size(), fo) != out.size()) return 7;
  fclose(fo);
  return 0;
}

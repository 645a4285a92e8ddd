// narrow_host.cpp -- box_box (csrc/mre_collide.h) compiled for the CPU: the register path of an unclipped face
// contact against the clipped path, on the same inputs, bit for bit.
//
//   g++ -O2 -ffp-contract=on -std=c++17 narrow_host.cpp -o narrow_host
//   narrow_host POSES.f32 RESULT.i32
//
// POSES: float32 records of 24 words -- p1[3] quat1[4] half1[3] p2[3] quat2[4] half2[3] margin pad[3].
// RESULT: int32 records of 4 words -- took the register path, candidates, mismatch, owner -- one per pose.
// owner: the box whose face is the reference face (1 or 2; 0: edge contact or none), read off the normal, which is
// plus or minus a column of that box's frame, bit for bit (both boxes' columns alike: box 1, which the SAT prefers).
// A pose is a mismatch when the two paths differ in the number of candidates, in a bit of the normal or in a bit
// of a candidate's position or distance (same order), or when the register path wrote to its clip buffer.
// Prints "poses P hits H mismatches M"; the exit status is 1 when M > 0.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define MRE_DEV static inline
#include "../../mujoco_robot_environments_amd/csrc/mre_collide.h"

using namespace mre;

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: narrow_host POSES.f32 RESULT.i32\n"); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 2; }
  std::vector<float> in;
  float rec[24];
  while (fread(rec, sizeof(rec), 1, fi) == 1) in.insert(in.end(), rec, rec + 24);
  fclose(fi);
  const size_t P = in.size() / 24;
  std::vector<int32_t> out(4 * P);
  const float SENT = -12345.5f;   // what a clip buffer holds before the call
  size_t hits = 0, bad = 0;
  for (size_t i = 0; i < P; i++) {
    const float* r = &in[24 * i];
    float q1[4] = {r[3], r[4], r[5], r[6]}, q2[4] = {r[13], r[14], r[15], r[16]}, R1[9], R2[9];
    qnormalize(q1); qnormalize(q2);
    q2mat(R1, q1); q2mat(R2, q2);
    const float margin = r[20];
    float bufA[COLL_BUF], bufB[COLL_BUF], nA[3] = {0.f, 0.f, 1.f}, nB[3] = {0.f, 0.f, 1.f};
    for (int k = 0; k < COLL_BUF; k++) bufA[k] = bufB[k] = SENT;
    FaceCand rcA, rcB;
    memset(&rcA, 0, sizeof(rcA)); memset(&rcB, 0, sizeof(rcB));
    unsigned rmA = 0u, rmB = 0u;
    const int cA = box_box(r, R1, r + 7, r + 10, R2, r + 17, margin, nA, bufA, false, rcA, rmA);
    const int cB = box_box(r, R1, r + 7, r + 10, R2, r + 17, margin, nB, bufB, true, rcB, rmB);
    const bool hit = (rmA & FACE_IN_REGS) != 0u;
    bool mis = cA != cB || (rmB & FACE_IN_REGS) != 0u;
    for (int k = 0; k < 3; k++) mis = mis || bits(nA[k]) != bits(nB[k]);
    if (!mis) {
      float ca[8][4];
      int m = 0;
      if (hit) {
        for (int v = 0; v < 4; v++)
          if ((rmA >> v) & 1u) { ca[m][0] = rcA.x[v]; ca[m][1] = rcA.y[v]; ca[m][2] = rcA.z[v]; ca[m][3] = rcA.d[v]; m++; }
        for (int k = 0; k < COLL_BUF; k++) mis = mis || bits(bufA[k]) != bits(SENT);
      } else {
        for (; m < cA; m++) { for (int k = 0; k < 3; k++) ca[m][k] = cand_xyz(bufA, m)[k]; ca[m][3] = cand_dist(bufA, m); }
      }
      mis = mis || m != cB;
      for (int c = 0; c < cB && !mis; c++) {
        for (int k = 0; k < 3; k++) mis = mis || bits(ca[c][k]) != bits(cand_xyz(bufB, c)[k]);
        mis = mis || bits(ca[c][3]) != bits(cand_dist(bufB, c));
      }
    }
    int owner = 0;
    if (cB > 0)
      for (int b = 2; b >= 1; b--) {
        const float* R = b == 1 ? R1 : R2;
        for (int c = 0; c < 3; c++)
          if (bits(fabsf(nB[0])) == bits(fabsf(R[c])) && bits(fabsf(nB[1])) == bits(fabsf(R[3 + c])) &&
              bits(fabsf(nB[2])) == bits(fabsf(R[6 + c]))) owner = b;
      }
    out[4 * i] = hit; out[4 * i + 1] = cB; out[4 * i + 2] = mis; out[4 * i + 3] = owner;
    hits += hit; bad += mis;
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  fwrite(out.data(), sizeof(int32_t), out.size(), fo);
  fclose(fo);
  printf("poses %zu hits %zu mismatches %zu\n", P, hits, bad);
  return bad ? 1 : 0;
}

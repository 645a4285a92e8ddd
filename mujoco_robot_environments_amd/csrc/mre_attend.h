// The Transporter pick head on the device (csrc/mre_attend.hip; include/mre.h, mre_attend): the best cell,
// the softmax cross-entropy against a target cell and its gradient, from logits [n][K][h][w] that a network has written.
// Shared between the kernel's translation unit and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here
// is launched by the step or the camera.
#ifndef MRE_ATTEND_H
#define MRE_ATTEND_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr int AT_NT = 256;              // lanes of a workgroup
constexpr int AT_LANE = 8;              // cells of a lane per chunk: one 16-byte vector of bfloat16, two of float32
constexpr int AT_CHUNK = AT_NT * AT_LANE;   // 2048 cells: what a workgroup takes in one step
constexpr int AT_MAX_SPLIT = 16;        // workgroups that share one env at most
constexpr size_t AT_SLOT_BYTES = 16;    // a workgroup's (max, sum of exp2, best value, best index) in the workspace
constexpr int AT_MAX_ROT = 64, AT_MAX_DIM = 4096;

constexpr uint32_t at_chunks(uint32_t cells) { return (cells + AT_CHUNK - 1) / AT_CHUNK; }
// S: the workgroups of one env.  It depends on the number of cells alone.
constexpr uint32_t at_split(uint32_t cells) { return at_chunks(cells) < AT_MAX_SPLIT ? at_chunks(cells) : AT_MAX_SPLIT; }
// split s of S takes the chunks [at_first(chunks, S, s), at_first(chunks, S, s + 1)): contiguous, none empty, the first
// chunks % S of them one chunk longer
constexpr uint32_t at_first(uint32_t chunks, uint32_t S, uint32_t s) {
  return s * (chunks / S) + (s < chunks % S ? s : chunks % S);
}

struct AttendArgs {
  const void* logits;      // f32 or bf16 [n][cells]
  const int64_t* target;   // [n] or null: no lse, target_logit, loss
  int64_t* best_index;     // [n] or null (with best_value)
  float* best_value;       // [n]
  float* lse;              // [n] (with target)
  float* target_logit;     // [n]
  float* loss;             // [n]
  void* workspace;         // [n][S] slots
  uint32_t n, cells;       // cells = K * h * w < 2^31
  uint32_t bf16;           // logits hold bfloat16, else float32
};

struct AttendGradArgs {
  const void* logits;      // f32 or bf16 [n][cells]
  const int64_t* target;   // [n], any value
  const float* lse;        // [n], what mre_attend wrote
  const float* weight;     // [n] or null (1)
  void* g;                 // [n][cells] of the logits' type
  uint32_t n, cells, bf16;
};

extern "C" void mre_launch_attend(const AttendArgs* a, hipStream_t stream);
extern "C" void mre_launch_attend_dlogits(const AttendGradArgs* a, hipStream_t stream);
#endif

// The Transporter place head on the device (csrc/mre_correlate.hip): every env's scene feature map cross-correlated with
// that env's own rotated crop feature maps on the bf16 matrix cores, and the best (rotation, row, column) per env.
// Shared between the kernel's translation unit and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here
// is launched by the step or the camera.
#ifndef MRE_CORRELATE_H
#define MRE_CORRELATE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr int CR_TILE_H = 16;        // pixel rows of a workgroup's tile: the 16 columns of one MFMA result
constexpr int CR_TILE_W = 32;        // pixel columns of a workgroup's tile: 8 per wave, 4 waves
constexpr int CR_MAX_ROT = 64, CR_MAX_DEPTH = 16, CR_MAX_CROP = 64, CR_MAX_DIM = 4096;
constexpr size_t CR_SLOT_BYTES = 8;  // a workgroup's (value f32, flat index i32) in the workspace

struct CorrelateArgs {
  const uint16_t* scene;   // bf16 [n][depth][h][w]
  const uint16_t* kern;    // bf16 [n][rot][depth][crop][crop]
  void* logits;            // f32 or bf16 [n][rot][h][w], or null
  int64_t* best_index;     // [n] or null (with best_value)
  float* best_value;       // [n]
  void* workspace;         // [n][tiles_y * tiles_x] slots
  uint32_t n, rot, depth, h, w, crop;
  uint32_t tiles_x, tiles_y;
  uint32_t bf16;           // logits hold bfloat16, else float32
  uint32_t vec_kern;       // crop % 8 == 0 and kern 16-byte aligned: a lane's 8 taps are one 16-byte load
  uint32_t vec_out;        // a lane's 8 logits of a row are stored at once: w % 8 == 0 and logits aligned to 8 elements
  uint32_t pivot;          // the crop index that lies on the output cell: crop / 2 (crop - 1 - crop / 2 for grad_scene)
};

constexpr uint32_t cr_tiles(uint32_t x, uint32_t tile) { return (x + tile - 1) / tile; }

// The softmax epilogues and the gradients (csrc/mre_correlate_grad.hip; include/mre.h, mre_correlate_loss and after it).
struct CorrelateLossArgs {
  CorrelateArgs fwd;       // scene, kern, the shape, workspace (the slots), vec_kern, pivot; logits and best_* unused
  const int64_t* target;   // [n] flat cell, any value
  const float* weight;     // [n] or null (1)
  const float* lse_in;     // dlogits: [n], what the loss call wrote
  float* lse;              // loss: [n]
  float* target_logit;     // loss: [n]
  float* loss;             // loss: [n]
  uint16_t* g;             // dlogits: bf16 [n][rot][h][w]
  uint32_t vec_g;          // w % 8 == 0 and g 16-byte aligned
};

constexpr int CR_BLOCK = 64;         // pixel block of grad_kern: the A operand is at most 64 x 64 cells of g[e][r]
constexpr int CR_MAX_SPLIT = 4;      // workgroups that share the pixel-block rows of one grad_kern tile
constexpr uint32_t cr_split(uint32_t h) { return cr_tiles(h, CR_BLOCK) < CR_MAX_SPLIT ? cr_tiles(h, CR_BLOCK) : CR_MAX_SPLIT; }

struct CorrelateGradArgs {
  const uint16_t* g;       // bf16 [n][rot][h][w]
  const uint16_t* scene;   // grad_kern: bf16 [n][depth][h][w]
  const uint16_t* kern;    // grad_scene: bf16 [n][rot][depth][crop][crop]
  float* out;              // grad_kern: [n][rot][depth][crop][crop]; grad_scene: [n][depth][h][w]
  void* workspace;         // grad_kern: f32 [n][split][rot][depth][crop][crop] when split > 1; grad_scene: bf16 kt
  uint32_t n, rot, depth, h, w, crop;
  uint32_t vec_g;          // grad_kern: w % 8 == 0 and g 16-byte aligned: a lane's 8 cells of a g row are one load
  uint32_t vec_out;        // grad_scene: w % 8 == 0 and out 16-byte aligned
};

extern "C" void mre_launch_correlate_loss(const CorrelateLossArgs* a, hipStream_t stream);
extern "C" void mre_launch_correlate_dlogits(const CorrelateLossArgs* a, hipStream_t stream);
extern "C" void mre_launch_correlate_grad_scene(const CorrelateGradArgs* a, hipStream_t stream);
extern "C" void mre_launch_correlate_grad_kern(const CorrelateGradArgs* a, hipStream_t stream);

// the correlation and, when best_* are asked for, the reduction of the workgroups' slots per env; both on `stream`
extern "C" void mre_launch_correlate(const CorrelateArgs* a, hipStream_t stream);
#endif

// Frame labels on the device (csrc/mre_labels.hip): per env and per label of a segmentation image, the box, the pixel
// count, the coordinate sums and the nearest depth of the label's pixels.  Shared between the kernels' translation unit
// and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here is launched by the step or the camera.
#ifndef MRE_LABELS_H
#define MRE_LABELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr uint32_t LAB_MAX_IDS = 8;        // labels of one call (LDS accumulators of a workgroup)
constexpr uint32_t LAB_UNIT = 4096;        // bytes one workgroup reads per sweep: 256 lanes x 16 bytes
constexpr uint32_t LAB_TARGET_WGS = 8192;  // work items aimed at: 256 CUs x 8 workgroups x 4 rounds
constexpr uint32_t LAB_MAX_GRID = 1u << 20;   // workgroups of a launch at most; work items beyond are looped over

struct LabelArgs {
  const uint8_t* seg;      // [n][hw] bytes, any alignment
  const float* depth;      // [n][hw] or null
  uint32_t n;
  uint32_t hw;             // pixels of one env's image (< 2^31)
  uint32_t w;              // its width
  uint32_t id0, nid;       // labels id0 .. id0 + nid - 1
  uint32_t chunks;         // workgroups' worth of pieces one env's image is cut into
  unsigned long long* stats;   // [n][nid][7]: xmin, ymin, xmax, ymax, count, sum_x, sum_y
  uint32_t* zmin;          // [n][nid] float bits, or null
};

// pieces per env: enough work items to fill the machine when n is small, one per env when n is large, and never a
// piece below one sweep
inline uint32_t label_chunks(uint32_t n, uint32_t hw) {
  const uint32_t units = (hw + LAB_UNIT - 1) / LAB_UNIT;
  const uint32_t want = (LAB_TARGET_WGS + n - 1) / n;
  return want < 1 ? 1 : (want > units ? units : want);
}

// init (every output element) + accumulate, in this order on `stream`
extern "C" void mre_launch_seg_labels(const LabelArgs* a, hipStream_t stream);
#endif

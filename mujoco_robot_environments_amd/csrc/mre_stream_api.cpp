// mre_stream_api.cpp -- the entry points of the C ABI (include/mre.h) that take a stream and no handle: CRC-32C and the
// episode records, frame labels, heightmaps, the map warp, the network inputs, the place head and the pick head.  They check their
// arguments, fill the unit's argument struct and enqueue its launch on the caller's stream; they own no buffer and never
// see an mre_env (mre_api.cpp has those that do).  No torch types; plain pointers and sizes only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <algorithm>

#include "../../include/mre.h"
#include "mre_host.h"
#include "mre_records.h"
#include "mre_labels.h"
#include "mre_heightmap.h"
#include "mre_warp.h"
#include "mre_warp_inputs.h"
#include "mre_correlate.h"
#include "mre_attend.h"

using namespace mre;

// CRC-32C (Castagnoli) of a host buffer: the checksum of TFRecord framing (dataset.py writes the
// reference's RLDS episodes, transporter_network_data_generation.py:56-111); slicing-by-8 tables
namespace {
struct Crc32cTables {   // built once, by the C++ runtime's thread-safe initialisation of the function-local static
  uint32_t T[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
      T[0][i] = c;
    }
    for (int k = 1; k < 8; k++)
      for (uint32_t i = 0; i < 256; i++) T[k][i] = (T[k - 1][i] >> 8) ^ T[0][T[k - 1][i] & 0xFFu];
  }
};
}  // namespace
extern "C" uint32_t mre_crc32c(const void* data, size_t n) {
  static const Crc32cTables tables;
  const uint32_t (*T)[256] = tables.T;
  const unsigned char* p = (const unsigned char*)data;
  uint32_t crc = 0xFFFFFFFFu;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
    lo ^= crc;
    crc = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^ T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^
          T[3][hi & 0xFF] ^ T[2][(hi >> 8) & 0xFF] ^ T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
    p += 8; n -= 8;
  }
  while (n--) crc = T[0][(crc ^ *p++) & 0xFFu] ^ (crc >> 8);
  return crc ^ 0xFFFFFFFFu;
}

// ---- episode records on the device (csrc/mre_records.hip): packed varints and CRC-32C of byte rows
extern "C" uint32_t mre_crc32c_combine(uint32_t crc_a, uint32_t crc_b, size_t len_b) {
  return mre_rec_crc32c_combine(crc_a, crc_b, len_b);
}

static size_t rec_segments(size_t row_bytes) { return (row_bytes + REC_PACK_SEG - 1) / REC_PACK_SEG; }

extern "C" size_t mre_records_workspace_bytes(int rows, size_t row_bytes) {
  if (rows <= 0 || row_bytes == 0 || row_bytes > REC_MAX_ROW_BYTES) return 0;
  return 2 * (size_t)rows * rec_segments(row_bytes) * sizeof(uint32_t);   // segment offsets + segment CRCs
}

// the checks the two calls share; fills the row interface of RecArgs (nseg for `seg` bytes per segment)
static int rec_args(const char* who, RecArgs& a, const uint8_t* src, size_t row_stride, size_t row_bytes,
                    const int32_t* rows_idx, int src_rows, int rows, void* workspace, size_t workspace_bytes, size_t seg) {
  const std::string w(who);
  if (!src || rows <= 0 || src_rows <= 0 || row_bytes == 0 || !workspace)
    return fail(MRE_ERR_ARG, w + ": null argument or empty row set");
  if (row_bytes > REC_MAX_ROW_BYTES) return fail(MRE_ERR_ARG, w + ": row_bytes above 2^30");
  if (row_stride < row_bytes && src_rows > 1) return fail(MRE_ERR_ARG, w + ": row_stride below row_bytes");
  if (!rows_idx && rows > src_rows) return fail(MRE_ERR_ARG, w + ": more rows than the source holds and no index list");
  const size_t nseg = (row_bytes + seg - 1) / seg;
  if ((size_t)rows * nseg > 0x7FFFFFFFull) return fail(MRE_ERR_ARG, w + ": rows x segments above 2^31 - 1");
  if (workspace_bytes < mre_records_workspace_bytes(rows, row_bytes) || ((uintptr_t)workspace & 3))
    return fail(MRE_ERR_ARG, w + ": workspace smaller than mre_records_workspace_bytes() or not 4-byte aligned");
  if (!is_device_ptr(src) || !is_device_ptr(workspace) || (rows_idx && !is_device_ptr(rows_idx)))
    return fail(MRE_ERR_ARG, w + ": src, rows_idx and workspace must be device pointers");
  memset(&a, 0, sizeof(a));
  a.src = src; a.stride = row_stride; a.row_bytes = (uint32_t)row_bytes; a.idx = rows_idx;
  a.src_rows = (uint32_t)src_rows; a.rows = (uint32_t)rows; a.nseg = (uint32_t)nseg;
  a.segoff = (uint32_t*)workspace;
  a.segcrc = a.segoff + (size_t)rows * rec_segments(row_bytes);
  return MRE_OK;
}

extern "C" int mre_varint_pack_rows(void* stream, const uint8_t* src, size_t row_stride, size_t row_bytes,
                                    const int32_t* rows_idx, int src_rows, int rows, uint8_t* out, size_t out_capacity,
                                    int64_t* off, uint32_t* len, uint32_t* crc, void* workspace, size_t workspace_bytes) {
  RecArgs a;
  int rc = rec_args("mre_varint_pack_rows", a, src, row_stride, row_bytes, rows_idx, src_rows, rows, workspace,
                    workspace_bytes, REC_PACK_SEG);
  if (rc) return rc;
  if (!off || !len || !is_device_ptr(off) || !is_device_ptr(len) || ((uintptr_t)off & 7) || ((uintptr_t)len & 3))
    return fail(MRE_ERR_ARG, "mre_varint_pack_rows: off / len must be aligned device pointers");
  if (out) {
    // the worst case, not the actual length: the length is only known on the device, and nothing may be written
    // beyond the caller's buffer whatever the rows hold
    if (out_capacity / 2 / (size_t)rows < row_bytes)
      return fail(MRE_ERR_ARG, "mre_varint_pack_rows: out_capacity below the worst case 2 * rows * row_bytes");
    if (!crc || !is_device_ptr(out) || !is_device_ptr(crc) || ((uintptr_t)crc & 3))
      return fail(MRE_ERR_ARG, "mre_varint_pack_rows: out / crc must be device pointers (crc 4-byte aligned)");
  }
  a.out = out; a.off = (long long*)off; a.len = len; a.crc = crc;
  mre_launch_varint_size(&a, (hipStream_t)stream);
  if (out) mre_launch_varint_pack(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

extern "C" int mre_crc32c_rows(void* stream, const uint8_t* src, size_t row_stride, size_t row_bytes,
                               const int32_t* rows_idx, int src_rows, int rows, uint32_t* crc, void* workspace,
                               size_t workspace_bytes) {
  RecArgs a;
  int rc = rec_args("mre_crc32c_rows", a, src, row_stride, row_bytes, rows_idx, src_rows, rows, workspace,
                    workspace_bytes, REC_CRC_SEG);
  if (rc) return rc;
  if (!crc || !is_device_ptr(crc) || ((uintptr_t)crc & 3))
    return fail(MRE_ERR_ARG, "mre_crc32c_rows: crc must be a 4-byte aligned device pointer");
  a.crc = crc;
  mre_launch_crc32c_rows(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

static size_t unpack_segments(size_t max_src_len) { return (max_src_len + REC_UNPACK_SEG - 1) / REC_UNPACK_SEG; }

extern "C" size_t mre_varint_unpack_workspace_bytes(int rows, size_t max_src_len) {
  if (rows <= 0 || max_src_len == 0 || max_src_len > REC_MAX_PACKED_BYTES) return 0;
  return (size_t)rows * unpack_segments(max_src_len) * sizeof(uint32_t);   // start bytes per segment, then their scan
}

extern "C" int mre_varint_unpack_rows(void* stream, const uint8_t* src, size_t src_bytes, const int64_t* src_off,
                                      const int64_t* src_len, const int64_t* nvalues, const int64_t* out_off, int rows,
                                      size_t max_src_len, uint8_t* out, size_t out_capacity, uint32_t* status,
                                      void* workspace, size_t workspace_bytes) {
  const std::string w("mre_varint_unpack_rows");
  if (!src || !src_off || !src_len || !nvalues || !out_off || !out || !status || !workspace || rows <= 0 ||
      src_bytes == 0 || out_capacity == 0)
    return fail(MRE_ERR_ARG, w + ": null argument, empty buffer or empty row set");
  if (max_src_len == 0 || max_src_len > REC_MAX_PACKED_BYTES) return fail(MRE_ERR_ARG, w + ": max_src_len outside 1 .. 2^31");
  const size_t nseg = unpack_segments(max_src_len);
  if ((size_t)rows * nseg > 0x7FFFFFFFull) return fail(MRE_ERR_ARG, w + ": rows x segments above 2^31 - 1");
  if (workspace_bytes < mre_varint_unpack_workspace_bytes(rows, max_src_len) || ((uintptr_t)workspace & 3))
    return fail(MRE_ERR_ARG, w + ": workspace smaller than mre_varint_unpack_workspace_bytes() or not 4-byte aligned");
  if ((((uintptr_t)src_off | (uintptr_t)src_len | (uintptr_t)nvalues | (uintptr_t)out_off) & 7) || ((uintptr_t)status & 3))
    return fail(MRE_ERR_ARG, w + ": descriptors must be 8-byte aligned, status 4-byte aligned");
  if (!is_device_ptr(src) || !is_device_ptr(src_off) || !is_device_ptr(src_len) || !is_device_ptr(nvalues) ||
      !is_device_ptr(out_off) || !is_device_ptr(out) || !is_device_ptr(status) || !is_device_ptr(workspace))
    return fail(MRE_ERR_ARG, w + ": src, the descriptors, out, status and workspace must be device pointers");
  UnpackArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.src_bytes = src_bytes;
  a.src_off = (const long long*)src_off; a.src_len = (const long long*)src_len;
  a.nvalues = (const long long*)nvalues; a.out_off = (const long long*)out_off;
  a.max_src_len = max_src_len; a.rows = (uint32_t)rows; a.nseg = (uint32_t)nseg;
  a.out = out; a.out_capacity = out_capacity; a.status = status; a.segoff = (uint32_t*)workspace;
  mre_launch_varint_unpack(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- frame labels on the device (csrc/mre_labels.hip): boxes, counts, coordinate sums and nearest depth per label
extern "C" int mre_seg_labels(void* stream, const uint8_t* seg, const float* depth, int n, int height, int width,
                              int id0, int nid, int64_t* stats, float* zmin) {
  const std::string w("mre_seg_labels");
  if (n < 0 || height < 1 || width < 1 || (long long)height * width >= (1ll << 31))
    return fail(MRE_ERR_ARG, w + ": n >= 0, height and width >= 1, height * width < 2^31");
  if (nid < 1 || nid > (int)LAB_MAX_IDS || id0 < 0 || id0 + nid > 256)
    return fail(MRE_ERR_ARG, w + ": 1 <= nid <= 8 labels inside 0 .. 255");
  if (!seg || !stats) return fail(MRE_ERR_ARG, w + ": null seg or stats");
  if ((depth == nullptr) != (zmin == nullptr)) return fail(MRE_ERR_ARG, w + ": depth and zmin go together");
  if (((uintptr_t)depth & 3) || ((uintptr_t)zmin & 3) || ((uintptr_t)stats & 7))
    return fail(MRE_ERR_ARG, w + ": depth and zmin must be 4-byte aligned, stats 8-byte aligned");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(seg) || !is_device_ptr(stats) || (depth && (!is_device_ptr(depth) || !is_device_ptr(zmin))))
    return fail(MRE_ERR_ARG, w + ": seg, depth, stats and zmin must be device pointers");
  LabelArgs a;
  memset(&a, 0, sizeof(a));
  a.seg = seg; a.depth = depth; a.n = (uint32_t)n; a.hw = (uint32_t)(height * width); a.w = (uint32_t)width;
  a.id0 = (uint32_t)id0; a.nid = (uint32_t)nid; a.chunks = label_chunks(a.n, a.hw);
  a.stats = (unsigned long long*)stats; a.zmin = (uint32_t*)zmin;
  mre_launch_seg_labels(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- orthographic heightmaps on the device (csrc/mre_heightmap.hip): height, colour, label and source pixel per cell
// the inverse of A (cam[0 .. 9), formed in float64) bounds the pixels a tile can take (the source rectangle); false when
// there is no usable one, and every tile then scans the whole image
static bool heightmap_inverse(const float* cam, float* inv) {
  const double m[9] = {cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7], cam[8]};
  const double co[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                        m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                        m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
  const double det = m[0] * co[0] + m[1] * co[3] + m[2] * co[6];
  double big = 0.0;
  for (int k = 0; k < 9; k++) big = std::max(big, std::fabs(m[k]));
  bool usable = std::isfinite(det) && std::fabs(det) > 1e-12 * big * big * big && std::isfinite(cam[9]) &&
                std::isfinite(cam[10]) && std::isfinite(cam[11]);
  for (int k = 0; k < 9; k++) {
    inv[k] = (float)(co[k] / det);
    usable = usable && std::isfinite(inv[k]);
  }
  return usable;
}

// what mre_heightmap and mre_heightmap_views say of the maps, in the name `w` of the entry point: the checks from the
// map's size to the pairing of the images (depth, rgb, seg: an image, or a list of them) with their outputs, and the
// grid, its tiling and the outputs as the kernels read them (all of *m but m->g.cam)
static int heightmap_maps(const std::string& w, const void* depth, const void* rgb, const void* seg, const float* cam,
                          const float* bounds, float inv_cell, float max_depth, int out_h, int out_w, float* hmap,
                          uint8_t* cmap, uint8_t* smap, int32_t* src, HmMaps* m) {
  if (out_h < 1 || out_w < 1 || out_h > (int)HM_MAX_OUT || out_w > (int)HM_MAX_OUT)
    return fail(MRE_ERR_ARG, w + ": 1 <= out_h, out_w <= 4096");
  if (!(inv_cell > 0.f) || !(max_depth > 0.f) || !std::isfinite(inv_cell) || !std::isfinite(max_depth))
    return fail(MRE_ERR_ARG, w + ": inv_cell and max_depth must be positive and finite");
  if (!cam || !bounds) return fail(MRE_ERR_ARG, w + ": null cam or bounds");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(bounds[k]) || !std::isfinite(bounds[3 + k]) || !(bounds[k] <= bounds[3 + k]))
      return fail(MRE_ERR_ARG, w + ": bounds must be finite with lo <= hi");
  if (!depth || !hmap) return fail(MRE_ERR_ARG, w + ": null depth or hmap");
  if ((rgb == nullptr) != (cmap == nullptr)) return fail(MRE_ERR_ARG, w + ": rgb and cmap go together");
  if ((seg == nullptr) != (smap == nullptr)) return fail(MRE_ERR_ARG, w + ": seg and smap go together");
  for (int k = 0; k < 3; k++) { m->g.lo[k] = bounds[k]; m->g.hi[k] = bounds[3 + k]; }
  m->g.inv_cell = inv_cell; m->g.max_depth = max_depth; m->g.out_w = (float)out_w; m->g.out_h = (float)out_h;
  m->cell = (float)(1.0 / (double)inv_cell);
  m->out_h = (uint32_t)out_h; m->out_w = (uint32_t)out_w;
  m->tiles_x = (m->out_w + HM_TILE - 1) / HM_TILE; m->tiles_y = (m->out_h + HM_TILE - 1) / HM_TILE;
  m->hmap = hmap; m->cmap = cmap; m->smap = smap; m->src = src;
  return MRE_OK;
}

extern "C" int mre_heightmap(void* stream, const float* depth, const uint8_t* rgb, const uint8_t* seg, int n, int height,
                             int width, const float* cam, const float* bounds, float inv_cell, float max_depth, int out_h,
                             int out_w, float* hmap, uint8_t* cmap, uint8_t* smap, int32_t* src) {
  const std::string w("mre_heightmap");
  HeightmapArgs a;
  memset(&a, 0, sizeof(a));
  if (n < 0 || height < 1 || width < 1 || (long long)height * width >= (1ll << 31))
    return fail(MRE_ERR_ARG, w + ": n >= 0, height and width >= 1, height * width < 2^31");
  if (const int rc = heightmap_maps(w, depth, rgb, seg, cam, bounds, inv_cell, max_depth, out_h, out_w, hmap, cmap, smap,
                                    src, &a.m))
    return rc;
  if (((uintptr_t)depth & 3) || ((uintptr_t)hmap & 3) || ((uintptr_t)src & 3))
    return fail(MRE_ERR_ARG, w + ": depth, hmap and src must be 4-byte aligned");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(depth) || !is_device_ptr(hmap) || (rgb && (!is_device_ptr(rgb) || !is_device_ptr(cmap))) ||
      (seg && (!is_device_ptr(seg) || !is_device_ptr(smap))) || (src && !is_device_ptr(src)))
    return fail(MRE_ERR_ARG, w + ": depth, rgb, seg, hmap, cmap, smap and src must be device pointers");
  a.depth = depth; a.rgb = rgb; a.seg = seg; a.n = (uint32_t)n; a.h = (uint32_t)height; a.w = (uint32_t)width;
  memcpy(a.m.g.cam, cam, sizeof(a.m.g.cam));
  a.whole_image = heightmap_inverse(cam, a.inv) ? 0u : 1u;
  mre_launch_heightmap(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- the same maps from several views at once (csrc/mre_heightmap_views.hip): the views' pixels compete for the cells
extern "C" int mre_heightmap_views(void* stream, int views, const float* const* depth, const uint8_t* const* rgb,
                                   const uint8_t* const* seg, int n, const int32_t* height, const int32_t* width,
                                   const float* cam, const float* bounds, float inv_cell, float max_depth, int out_h,
                                   int out_w, float* hmap, uint8_t* cmap, uint8_t* smap, int32_t* src, uint8_t* view) {
  static_assert(HM_MAX_VIEWS == MRE_HM_MAX_VIEWS, "the kernel's argument array holds the header's view count");
  const std::string w("mre_heightmap_views");
  HeightmapViewsArgs a;
  memset(&a, 0, sizeof(a));
  if (views < 1 || views > MRE_HM_MAX_VIEWS) return fail(MRE_ERR_ARG, w + ": 1 <= views <= 8");
  if (n < 0 || !height || !width) return fail(MRE_ERR_ARG, w + ": n >= 0, height and width non-null");
  for (int i = 0; i < views; i++)
    if (height[i] < 1 || width[i] < 1 || (long long)height[i] * width[i] >= (long long)HM_VIEW_PIXELS)
      return fail(MRE_ERR_ARG, w + ": height and width >= 1, height * width < 2^28 in every view");
  if (const int rc = heightmap_maps(w, depth, rgb, seg, cam, bounds, inv_cell, max_depth, out_h, out_w, hmap, cmap, smap,
                                    src, &a.m))
    return rc;
  for (int i = 0; i < views; i++) {
    if (!depth[i] || (rgb && !rgb[i]) || (seg && !seg[i]))
      return fail(MRE_ERR_ARG, w + ": depth, and rgb and seg when given, must be non-null in every view");
    if ((uintptr_t)depth[i] & 3) return fail(MRE_ERR_ARG, w + ": depth, hmap and src must be 4-byte aligned");
  }
  if (((uintptr_t)hmap & 3) || ((uintptr_t)src & 3)) return fail(MRE_ERR_ARG, w + ": depth, hmap and src must be 4-byte aligned");
  if (n == 0) return MRE_OK;
  bool on_device = is_device_ptr(hmap) && (!cmap || is_device_ptr(cmap)) && (!smap || is_device_ptr(smap)) &&
                   (!src || is_device_ptr(src)) && (!view || is_device_ptr(view));
  for (int i = 0; i < views && on_device; i++)
    on_device = is_device_ptr(depth[i]) && (!rgb || is_device_ptr(rgb[i])) && (!seg || is_device_ptr(seg[i]));
  if (!on_device)
    return fail(MRE_ERR_ARG, w + ": depth, rgb, seg, hmap, cmap, smap, src and view must be device pointers");
  for (int i = 0; i < views; i++) {
    HeightmapView& v = a.v[i];
    v.depth = depth[i]; v.rgb = rgb ? rgb[i] : nullptr; v.seg = seg ? seg[i] : nullptr;
    v.h = (uint32_t)height[i]; v.w = (uint32_t)width[i]; v.hw = v.h * v.w;
    memcpy(v.cam, cam + 12 * i, sizeof(v.cam));
    v.whole_image = heightmap_inverse(v.cam, v.inv) ? 0u : 1u;
  }
  a.views = (uint32_t)views; a.n = (uint32_t)n; a.view = view;
  mre_launch_heightmap_views(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- what mre_warp_maps and mre_warp_inputs gather from (csrc/mre_warp_gather.h): the checks on the arguments they
// share, in the name `w` of the entry point, and those arguments as the kernels read them
static int warp_source(const std::string& w, const float* hmap, const uint8_t* cmap, int n, int in_h, int in_w,
                       const int32_t* index, const float* mats, int samples, int out_h, int out_w, WarpSource* s) {
  const int lim = (int)WP_MAX_DIM;
  if (n < 0 || samples < 0) return fail(MRE_ERR_ARG, w + ": n >= 0 and samples >= 0");
  if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || in_h > lim || in_w > lim || out_h > lim || out_w > lim)
    return fail(MRE_ERR_ARG, w + ": 1 <= in_h, in_w, out_h, out_w <= 4096");
  if (!hmap || !mats) return fail(MRE_ERR_ARG, w + ": null hmap or mats");
  if (((uintptr_t)hmap & 3) || ((uintptr_t)mats & 3) || ((uintptr_t)index & 3))
    return fail(MRE_ERR_ARG, w + ": hmap, mats and index must be 4-byte aligned");
  if (!index && samples > n) return fail(MRE_ERR_ARG, w + ": more samples than maps and no index");
  s->hmap = hmap; s->cmap = cmap; s->index = index; s->mats = mats;
  s->n = (uint32_t)n; s->in_h = (uint32_t)in_h; s->in_w = (uint32_t)in_w;
  s->samples = (uint32_t)samples; s->out_h = (uint32_t)out_h; s->out_w = (uint32_t)out_w;
  s->tiles_x = (s->out_w + WP_TILE_W - 1) / WP_TILE_W; s->tiles_y = (s->out_h + WP_TILE_H - 1) / WP_TILE_H;
  return MRE_OK;
}

// ---- warped and cropped maps on the device (csrc/mre_warp.hip): a nearest-neighbour affine gather of the three maps
extern "C" int mre_warp_maps(void* stream, const float* hmap, const uint8_t* cmap, const uint8_t* smap, int n, int in_h,
                             int in_w, const int32_t* index, const float* mats, int samples, int out_h, int out_w,
                             float* out_h_, uint8_t* out_c, uint8_t* out_s, int32_t* from) {
  const std::string w("mre_warp_maps");
  WarpArgs a;
  memset(&a, 0, sizeof(a));
  if (const int rc = warp_source(w, hmap, cmap, n, in_h, in_w, index, mats, samples, out_h, out_w, &a.source)) return rc;
  if (!out_h_) return fail(MRE_ERR_ARG, w + ": null height output");
  if ((cmap == nullptr) != (out_c == nullptr)) return fail(MRE_ERR_ARG, w + ": cmap and its output go together");
  if ((smap == nullptr) != (out_s == nullptr)) return fail(MRE_ERR_ARG, w + ": smap and its output go together");
  if (((uintptr_t)out_h_ & 3) || ((uintptr_t)from & 3))
    return fail(MRE_ERR_ARG, w + ": the height output and from must be 4-byte aligned");
  // no output byte range may overlap an input byte range (n, samples <= 2^31 and maps <= 2^24 cells: no overflow)
  const size_t in_cells = (size_t)n * in_h * in_w, out_cells = (size_t)samples * out_h * out_w;
  const ByteRange ins[5] = {{hmap, 4 * in_cells}, {cmap, 3 * in_cells}, {smap, in_cells},
                            {index, 4 * (size_t)samples}, {mats, 24 * (size_t)samples}};
  const ByteRange outs[4] = {{out_h_, 4 * out_cells}, {out_c, 3 * out_cells}, {out_s, out_cells}, {from, 4 * out_cells}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, w + ": an output overlaps an input");
  if (n == 0 || samples == 0) return MRE_OK;
  if (!is_device_ptr(hmap) || !is_device_ptr(mats) || !is_device_ptr(out_h_) || (index && !is_device_ptr(index)) ||
      (cmap && (!is_device_ptr(cmap) || !is_device_ptr(out_c))) ||
      (smap && (!is_device_ptr(smap) || !is_device_ptr(out_s))) || (from && !is_device_ptr(from)))
    return fail(MRE_ERR_ARG, w + ": the maps, index, mats and the outputs must be device pointers");
  // the wide stores: 4 cells of a row at once need the width a multiple of 4 and bases aligned to what a lane stores
  a.vec = (out_w % 4 == 0 && !((uintptr_t)out_h_ & 15) && !((uintptr_t)from & 15) && !((uintptr_t)out_c & 3) &&
           !((uintptr_t)out_s & 3)) ? 1u : 0u;
  a.smap = smap; a.out_h_ = out_h_; a.out_c = out_c; a.out_s = out_s; a.from = from;
  mre_launch_warp_maps(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- network-ready inputs on the device (csrc/mre_warp_inputs.hip): the same gather, written planar and normalised
extern "C" int mre_warp_inputs(void* stream, const float* hmap, const uint8_t* cmap, int n, int in_h, int in_w,
                               const int32_t* index, const float* mats, int samples, int out_h, int out_w, int channels,
                               const int32_t* chan_src, const float* chan_scale, const float* chan_bias, int dtype,
                               void* out) {
  const std::string w("mre_warp_inputs");
  WarpInputArgs a;
  memset(&a, 0, sizeof(a));
  if (const int rc = warp_source(w, hmap, cmap, n, in_h, in_w, index, mats, samples, out_h, out_w, &a.source)) return rc;
  if (!out) return fail(MRE_ERR_ARG, w + ": null out");
  if (channels < 1 || channels > WI_MAX_CHANNELS) return fail(MRE_ERR_ARG, w + ": 1 <= channels <= 8");
  if (!chan_src || !chan_scale || !chan_bias) return fail(MRE_ERR_ARG, w + ": null chan_src, chan_scale or chan_bias");
  bool colour = false;
  for (int k = 0; k < channels; k++) {
    if (chan_src[k] < MRE_SRC_RED || chan_src[k] > MRE_SRC_HEIGHT)
      return fail(MRE_ERR_ARG, w + ": chan_src must be 0 (red), 1 (green), 2 (blue) or 3 (height)");
    colour = colour || chan_src[k] != MRE_SRC_HEIGHT;
    if (!std::isfinite(chan_scale[k]) || !std::isfinite(chan_bias[k]))
      return fail(MRE_ERR_ARG, w + ": chan_scale and chan_bias must be finite");
  }
  if (colour && !cmap) return fail(MRE_ERR_ARG, w + ": a colour source needs cmap");
  if (dtype != MRE_F32 && dtype != MRE_BF16) return fail(MRE_ERR_ARG, w + ": dtype must be MRE_F32 or MRE_BF16");
  const size_t esize = dtype == MRE_BF16 ? 2 : 4;
  if ((uintptr_t)out & (esize - 1)) return fail(MRE_ERR_ARG, w + ": out must be aligned to its element size");
  // out may overlap no input byte range (samples <= 2^31, 8 channels, maps <= 2^24 cells, 4 B: below 2^60)
  const size_t in_cells = (size_t)n * in_h * in_w;
  const size_t out_bytes = (size_t)samples * channels * out_h * out_w * esize;
  const ByteRange ins[4] = {{hmap, 4 * in_cells}, {cmap, 3 * in_cells}, {index, 4 * (size_t)samples},
                            {mats, 24 * (size_t)samples}};
  const ByteRange outs[1] = {{out, out_bytes}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, w + ": out overlaps an input");
  if (n == 0 || samples == 0) return MRE_OK;
  if (!is_device_ptr(hmap) || !is_device_ptr(mats) || !is_device_ptr(out) || (index && !is_device_ptr(index)) ||
      (colour && !is_device_ptr(cmap)))
    return fail(MRE_ERR_ARG, w + ": the maps, index, mats and out must be device pointers");
  if (!colour) a.source.cmap = nullptr;   // given, but no channel reads it
  // the wide stores: a lane's 4 cells of a channel at once need the width a multiple of 4 (every row and every channel
  // plane then starts at a multiple of 4 elements) and out aligned to those 4 elements
  a.vec = (out_w % 4 == 0 && ((size_t)out_h * out_w) % 4 == 0 && !((uintptr_t)out & (4 * esize - 1))) ? 1u : 0u;
  a.colour = colour ? 1u : 0u; a.bf16 = dtype == MRE_BF16 ? 1u : 0u; a.channels = (uint32_t)channels;
  for (int k = 0; k < channels; k++) {
    a.src[k] = (uint32_t)chan_src[k]; a.scale[k] = chan_scale[k]; a.bias[k] = chan_bias[k];
  }
  a.out = out;
  mre_launch_warp_inputs(&a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- what the entries of the two Transporter heads check alike; `wh` is the entry's name
static size_t element_size(int dtype) { return dtype == MRE_BF16 ? 2 : 4; }

static int workspace_ok(const std::string& wh, const void* workspace, size_t workspace_bytes, size_t need, const char* sizer) {
  if (workspace && !((uintptr_t)workspace & 15) && workspace_bytes >= need) return MRE_OK;
  return fail(MRE_ERR_ARG, wh + ": workspace must be non-NULL, 16-byte aligned and as large as " + sizer + " says");
}

static int best_pair_ok(const std::string& wh, const int64_t* best_index, const float* best_value) {
  if (!best_index != !best_value) return fail(MRE_ERR_ARG, wh + ": best_index and best_value are NULL together or not at all");
  if (((uintptr_t)best_index & 7) || ((uintptr_t)best_value & 3))
    return fail(MRE_ERR_ARG, wh + ": best_index must be 8-byte and best_value 4-byte aligned");
  return MRE_OK;
}

static int target_ok(const std::string& wh, const int64_t* target) {
  return ((uintptr_t)target & 7) ? fail(MRE_ERR_ARG, wh + ": target must be 8-byte aligned") : MRE_OK;
}

// `required`: none of the three may be NULL (else the entry has its own rule for that)
static int loss_outputs_ok(const std::string& wh, const float* lse, const float* target_logit, const float* loss, bool required) {
  if (required && (!lse || !target_logit || !loss)) return fail(MRE_ERR_ARG, wh + ": null lse, target_logit or loss");
  if (((uintptr_t)lse & 3) || ((uintptr_t)target_logit & 3) || ((uintptr_t)loss & 3))
    return fail(MRE_ERR_ARG, wh + ": lse, target_logit and loss must be 4-byte aligned");
  return MRE_OK;
}

static int launched(void) {
  HIPCHK(hipGetLastError());
  return MRE_OK;
}

// ---- the Transporter place head on the device (csrc/mre_correlate.hip): correlate the crops with the scene, best cell
static bool correlate_shape_ok(int n, int rotations, int h, int w) {
  return n >= 0 && rotations >= 1 && rotations <= CR_MAX_ROT && h >= 1 && w >= 1 && h <= CR_MAX_DIM && w <= CR_MAX_DIM &&
         (long long)rotations * h * w < (1ll << 31);
}

static size_t correlate_workspace(int n, int h, int w) {
  const size_t slots = (size_t)n * cr_tiles((uint32_t)h, CR_TILE_H) * cr_tiles((uint32_t)w, CR_TILE_W);
  const size_t bytes = (slots * CR_SLOT_BYTES + 15) & ~(size_t)15;
  return bytes ? bytes : 16;   // never 0: a workspace can always be allocated and passed
}

extern "C" int mre_correlate_workspace(int n, int rotations, int h, int w, size_t* bytes) {
  const std::string wh("mre_correlate_workspace");
  if (!bytes) return fail(MRE_ERR_ARG, wh + ": null bytes");
  if (!correlate_shape_ok(n, rotations, h, w))
    return fail(MRE_ERR_ARG, wh + ": n >= 0, 1 <= rotations <= 64, 1 <= h, w <= 4096, rotations * h * w < 2^31");
  *bytes = correlate_workspace(n, h, w);
  return MRE_OK;
}

// the ranges mre_correlate shares with the five training entries below
static int correlate_ranges(const std::string& wh, int n, int rotations, int depth, int h, int w, int crop) {
  if (n < 0) return fail(MRE_ERR_ARG, wh + ": n >= 0");
  if (rotations < 1 || rotations > CR_MAX_ROT) return fail(MRE_ERR_ARG, wh + ": 1 <= rotations <= 64");
  if (depth < 1 || depth > CR_MAX_DEPTH) return fail(MRE_ERR_ARG, wh + ": 1 <= depth <= 16");
  if (crop < 2 || crop > CR_MAX_CROP || (crop & 1)) return fail(MRE_ERR_ARG, wh + ": crop must be even, 2 <= crop <= 64");
  if (h < 1 || w < 1 || h > CR_MAX_DIM || w > CR_MAX_DIM) return fail(MRE_ERR_ARG, wh + ": 1 <= h, w <= 4096");
  if (!correlate_shape_ok(n, rotations, h, w)) return fail(MRE_ERR_ARG, wh + ": rotations * h * w must be below 2^31");
  return MRE_OK;
}

// what every launch of the forward reads: the operands, the shape, the tiling
static void correlate_forward_args(CorrelateArgs& a, const uint16_t* scene, const uint16_t* kern, int n, int rotations,
                                   int depth, int h, int w, int crop, void* workspace) {
  memset(&a, 0, sizeof(a));
  a.scene = scene; a.kern = kern; a.workspace = workspace;
  a.n = (uint32_t)n; a.rot = (uint32_t)rotations; a.depth = (uint32_t)depth; a.h = (uint32_t)h; a.w = (uint32_t)w;
  a.crop = (uint32_t)crop; a.pivot = (uint32_t)crop / 2;
  a.tiles_x = cr_tiles(a.w, CR_TILE_W); a.tiles_y = cr_tiles(a.h, CR_TILE_H);
  // the wide access: a lane's 8 taps of a kernel row (every row then starts at a multiple of 8 elements)
  a.vec_kern = (crop % 8 == 0 && !((uintptr_t)kern & 15)) ? 1u : 0u;
}

extern "C" int mre_correlate(void* stream, const uint16_t* scene, const uint16_t* kern, int n, int rotations, int depth,
                             int h, int w, int crop, int dtype, void* logits, int64_t* best_index, float* best_value,
                             void* workspace, size_t workspace_bytes) {
  const std::string wh("mre_correlate");
  if (int rc = correlate_ranges(wh, n, rotations, depth, h, w, crop)) return rc;
  if (!scene || !kern) return fail(MRE_ERR_ARG, wh + ": null scene or kern");
  if (((uintptr_t)scene & 1) || ((uintptr_t)kern & 1)) return fail(MRE_ERR_ARG, wh + ": scene and kern must be 2-byte aligned");
  if (dtype != MRE_F32 && dtype != MRE_BF16) return fail(MRE_ERR_ARG, wh + ": dtype must be MRE_F32 or MRE_BF16");
  const size_t esize = element_size(dtype);
  if ((uintptr_t)logits & (esize - 1)) return fail(MRE_ERR_ARG, wh + ": logits must be aligned to its element size");
  if (int rc = best_pair_ok(wh, best_index, best_value)) return rc;
  if (!logits && !best_index) return fail(MRE_ERR_ARG, wh + ": nothing to write: logits and best_* are all NULL");
  const size_t need = correlate_workspace(n, h, w);
  if (int rc = workspace_ok(wh, workspace, workspace_bytes, need, "mre_correlate_workspace")) return rc;
  // no output or workspace byte range may overlap an input (n < 2^31, 64 x 16 x 64 x 64 x 2 B per env: below 2^54)
  const size_t cells = (size_t)h * w;
  const ByteRange ins[2] = {{scene, 2 * (size_t)n * depth * cells}, {kern, 2 * (size_t)n * rotations * depth * crop * crop}};
  const ByteRange outs[4] = {{logits, esize * (size_t)n * rotations * cells}, {best_index, 8 * (size_t)n},
                             {best_value, 4 * (size_t)n}, {workspace, need}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, wh + ": an output or the workspace overlaps an input");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(scene) || !is_device_ptr(kern) || !is_device_ptr(workspace) || (logits && !is_device_ptr(logits)) ||
      (best_index && (!is_device_ptr(best_index) || !is_device_ptr(best_value))))
    return fail(MRE_ERR_ARG, wh + ": scene, kern, the outputs and the workspace must be device pointers");
  CorrelateArgs a;
  correlate_forward_args(a, scene, kern, n, rotations, depth, h, w, crop, workspace);
  a.logits = logits; a.best_index = best_index; a.best_value = best_value;
  a.bf16 = dtype == MRE_BF16 ? 1u : 0u;
  a.vec_out = (logits && w % 8 == 0 && !((uintptr_t)logits & 15)) ? 1u : 0u;   // wide too: a lane's 8 logits of a pixel row
  mre_launch_correlate(&a, (hipStream_t)stream);
  return launched();
}

// ---- training the place head (csrc/mre_correlate_grad.hip): the loss, its gradient g, and the gradients of any g
extern "C" int mre_correlate_loss(void* stream, const uint16_t* scene, const uint16_t* kern, int n, int rotations, int depth,
                                  int h, int w, int crop, const int64_t* target, float* lse, float* target_logit,
                                  float* loss, void* workspace, size_t workspace_bytes) {
  const std::string wh("mre_correlate_loss");
  if (int rc = correlate_ranges(wh, n, rotations, depth, h, w, crop)) return rc;
  if (!scene || !kern || !target) return fail(MRE_ERR_ARG, wh + ": null scene, kern or target");
  if (((uintptr_t)scene & 1) || ((uintptr_t)kern & 1)) return fail(MRE_ERR_ARG, wh + ": scene and kern must be 2-byte aligned");
  if (int rc = target_ok(wh, target)) return rc;
  if (int rc = loss_outputs_ok(wh, lse, target_logit, loss, true)) return rc;
  const size_t need = correlate_workspace(n, h, w);
  if (int rc = workspace_ok(wh, workspace, workspace_bytes, need, "mre_correlate_workspace")) return rc;
  // (lengths below 2^54, as in mre_correlate)
  const size_t cells = (size_t)h * w;
  const ByteRange ins[3] = {{scene, 2 * (size_t)n * depth * cells}, {kern, 2 * (size_t)n * rotations * depth * crop * crop},
                            {target, 8 * (size_t)n}};
  const ByteRange outs[4] = {{lse, 4 * (size_t)n}, {target_logit, 4 * (size_t)n}, {loss, 4 * (size_t)n}, {workspace, need}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, wh + ": an output or the workspace overlaps an input");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(scene) || !is_device_ptr(kern) || !is_device_ptr(target) || !is_device_ptr(lse) ||
      !is_device_ptr(target_logit) || !is_device_ptr(loss) || !is_device_ptr(workspace))
    return fail(MRE_ERR_ARG, wh + ": scene, kern, target, the outputs and the workspace must be device pointers");
  CorrelateLossArgs a;
  memset(&a, 0, sizeof(a));
  correlate_forward_args(a.fwd, scene, kern, n, rotations, depth, h, w, crop, workspace);
  a.target = target; a.lse = lse; a.target_logit = target_logit; a.loss = loss;
  mre_launch_correlate_loss(&a, (hipStream_t)stream);
  return launched();
}

extern "C" int mre_correlate_dlogits(void* stream, const uint16_t* scene, const uint16_t* kern, int n, int rotations,
                                     int depth, int h, int w, int crop, const int64_t* target, const float* lse,
                                     const float* weight, uint16_t* g) {
  const std::string wh("mre_correlate_dlogits");
  if (int rc = correlate_ranges(wh, n, rotations, depth, h, w, crop)) return rc;
  if (!scene || !kern || !target || !lse) return fail(MRE_ERR_ARG, wh + ": null scene, kern, target or lse");
  if (((uintptr_t)scene & 1) || ((uintptr_t)kern & 1)) return fail(MRE_ERR_ARG, wh + ": scene and kern must be 2-byte aligned");
  if (int rc = target_ok(wh, target)) return rc;
  if (((uintptr_t)lse & 3) || ((uintptr_t)weight & 3)) return fail(MRE_ERR_ARG, wh + ": lse and weight must be 4-byte aligned");
  if (!g || ((uintptr_t)g & 1)) return fail(MRE_ERR_ARG, wh + ": g must be non-NULL and 2-byte aligned");
  const size_t cells = (size_t)h * w;
  const ByteRange ins[5] = {{scene, 2 * (size_t)n * depth * cells}, {kern, 2 * (size_t)n * rotations * depth * crop * crop},
                            {target, 8 * (size_t)n}, {lse, 4 * (size_t)n}, {weight, 4 * (size_t)n}};
  const ByteRange outs[1] = {{g, 2 * (size_t)n * rotations * cells}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, wh + ": g overlaps an input");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(scene) || !is_device_ptr(kern) || !is_device_ptr(target) || !is_device_ptr(lse) ||
      (weight && !is_device_ptr(weight)) || !is_device_ptr(g))
    return fail(MRE_ERR_ARG, wh + ": scene, kern, target, lse, weight and g must be device pointers");
  CorrelateLossArgs a;
  memset(&a, 0, sizeof(a));
  correlate_forward_args(a.fwd, scene, kern, n, rotations, depth, h, w, crop, nullptr);
  a.target = target; a.lse_in = lse; a.weight = weight; a.g = g;
  a.vec_g = (w % 8 == 0 && !((uintptr_t)g & 15)) ? 1u : 0u;
  mre_launch_correlate_dlogits(&a, (hipStream_t)stream);
  return launched();
}

// grad_scene keeps the flipped kernels (bfloat16) there, grad_kern the partial tiles of its cr_split(h) workgroups (float32)
static size_t correlate_grad_workspace(int n, int rotations, int depth, int h, int crop) {
  const size_t per = (size_t)n * rotations * depth * crop * crop, split = cr_split((uint32_t)h);
  const size_t bytes = (std::max(2 * per, split > 1 ? 4 * split * per : (size_t)0) + 15) & ~(size_t)15;
  return bytes ? bytes : 16;
}

extern "C" int mre_correlate_grad_workspace(int n, int rotations, int depth, int h, int w, int crop, size_t* bytes) {
  const std::string wh("mre_correlate_grad_workspace");
  if (!bytes) return fail(MRE_ERR_ARG, wh + ": null bytes");
  if (int rc = correlate_ranges(wh, n, rotations, depth, h, w, crop)) return rc;
  *bytes = correlate_grad_workspace(n, rotations, depth, h, crop);
  return MRE_OK;
}

// the checks the two gradient entries share: `other` is scene (grad_kern) or kern (grad_scene), of other_bytes
static int correlate_grad_check(const std::string& wh, const char* other_name, const uint16_t* g, const uint16_t* other,
                                size_t other_bytes, int n, int rotations, int depth, int h, int w, int crop, float* out,
                                size_t out_bytes, void* workspace, size_t workspace_bytes) {
  if (int rc = correlate_ranges(wh, n, rotations, depth, h, w, crop)) return rc;
  if (!g || !other) return fail(MRE_ERR_ARG, wh + ": null g or " + other_name);
  if (((uintptr_t)g & 1) || ((uintptr_t)other & 1)) return fail(MRE_ERR_ARG, wh + ": g and " + other_name + " must be 2-byte aligned");
  if (!out || ((uintptr_t)out & 3)) return fail(MRE_ERR_ARG, wh + ": the output must be non-NULL and 4-byte aligned");
  const size_t need = correlate_grad_workspace(n, rotations, depth, h, crop);
  if (int rc = workspace_ok(wh, workspace, workspace_bytes, need, "mre_correlate_grad_workspace")) return rc;
  // (n < 2^31 envs of at most 4 x 4 x 64 x 16 x 64 x 64 B of workspace: below 2^60)
  const ByteRange ins[2] = {{g, 2 * (size_t)n * rotations * h * w}, {other, other_bytes}};
  const ByteRange outs[2] = {{out, out_bytes}, {workspace, need}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, wh + ": the output or the workspace overlaps an input");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(g) || !is_device_ptr(other) || !is_device_ptr(out) || !is_device_ptr(workspace))
    return fail(MRE_ERR_ARG, wh + ": g, " + other_name + ", the output and the workspace must be device pointers");
  return MRE_OK;
}

static void correlate_grad_args(CorrelateGradArgs& a, const uint16_t* g, int n, int rotations, int depth, int h, int w, int crop,
                                float* out, void* workspace) {
  memset(&a, 0, sizeof(a));
  a.g = g; a.out = out; a.workspace = workspace;
  a.n = (uint32_t)n; a.rot = (uint32_t)rotations; a.depth = (uint32_t)depth; a.h = (uint32_t)h; a.w = (uint32_t)w;
  a.crop = (uint32_t)crop;
}

extern "C" int mre_correlate_grad_scene(void* stream, const uint16_t* g, const uint16_t* kern, int n, int rotations, int depth,
                                        int h, int w, int crop, float* grad_scene, void* workspace, size_t workspace_bytes) {
  const int rc = correlate_grad_check("mre_correlate_grad_scene", "kern", g, kern,
                                      2 * (size_t)std::max(n, 0) * rotations * depth * crop * crop, n, rotations, depth, h, w,
                                      crop, grad_scene, 4 * (size_t)std::max(n, 0) * depth * h * w, workspace, workspace_bytes);
  if (rc != MRE_OK || n == 0) return rc;
  CorrelateGradArgs a;
  correlate_grad_args(a, g, n, rotations, depth, h, w, crop, grad_scene, workspace);
  a.kern = kern;
  a.vec_out = (w % 8 == 0 && !((uintptr_t)grad_scene & 15)) ? 1u : 0u;
  mre_launch_correlate_grad_scene(&a, (hipStream_t)stream);
  return launched();
}

extern "C" int mre_correlate_grad_kern(void* stream, const uint16_t* g, const uint16_t* scene, int n, int rotations, int depth,
                                       int h, int w, int crop, float* grad_kern, void* workspace, size_t workspace_bytes) {
  const int rc = correlate_grad_check("mre_correlate_grad_kern", "scene", g, scene, 2 * (size_t)std::max(n, 0) * depth * h * w, n,
                                      rotations, depth, h, w, crop, grad_kern,
                                      4 * (size_t)std::max(n, 0) * rotations * depth * crop * crop, workspace, workspace_bytes);
  if (rc != MRE_OK || n == 0) return rc;
  CorrelateGradArgs a;
  correlate_grad_args(a, g, n, rotations, depth, h, w, crop, grad_kern, workspace);
  a.scene = scene;
  a.vec_g = (w % 8 == 0 && !((uintptr_t)g & 15)) ? 1u : 0u;
  mre_launch_correlate_grad_kern(&a, (hipStream_t)stream);
  return launched();
}

// ---- the Transporter pick head on the device (csrc/mre_attend.hip): best cell, loss and gradient from stored logits
static int attend_ranges(const std::string& wh, int n, int rotations, int h, int w, int dtype) {
  if (n < 0) return fail(MRE_ERR_ARG, wh + ": n >= 0");
  if (rotations < 1 || rotations > AT_MAX_ROT) return fail(MRE_ERR_ARG, wh + ": 1 <= rotations <= 64");
  if (h < 1 || w < 1 || h > AT_MAX_DIM || w > AT_MAX_DIM) return fail(MRE_ERR_ARG, wh + ": 1 <= h, w <= 4096");
  if ((long long)rotations * h * w >= (1ll << 31)) return fail(MRE_ERR_ARG, wh + ": rotations * h * w must be below 2^31");
  if (dtype != MRE_F32 && dtype != MRE_BF16) return fail(MRE_ERR_ARG, wh + ": dtype must be MRE_F32 or MRE_BF16");
  return MRE_OK;
}

static size_t attend_workspace(int n, int rotations, int h, int w) {
  const size_t bytes = (size_t)n * at_split((uint32_t)(rotations * h * w)) * AT_SLOT_BYTES;   // a multiple of 16
  return bytes ? bytes : 16;
}

extern "C" int mre_attend_workspace(int n, int rotations, int h, int w, size_t* bytes) {
  const std::string wh("mre_attend_workspace");
  if (!bytes) return fail(MRE_ERR_ARG, wh + ": null bytes");
  if (int rc = attend_ranges(wh, n, rotations, h, w, MRE_F32)) return rc;
  *bytes = attend_workspace(n, rotations, h, w);
  return MRE_OK;
}

extern "C" int mre_attend(void* stream, const void* logits, int n, int rotations, int h, int w, int dtype,
                          const int64_t* target, int64_t* best_index, float* best_value, float* lse, float* target_logit,
                          float* loss, void* workspace, size_t workspace_bytes) {
  const std::string wh("mre_attend");
  if (int rc = attend_ranges(wh, n, rotations, h, w, dtype)) return rc;
  const size_t esize = element_size(dtype);
  if (!logits || ((uintptr_t)logits & (esize - 1)))
    return fail(MRE_ERR_ARG, wh + ": logits must be non-NULL and aligned to its element size");
  if (int rc = best_pair_ok(wh, best_index, best_value)) return rc;
  if (!target != !lse || !target != !target_logit || !target != !loss)
    return fail(MRE_ERR_ARG, wh + ": target, lse, target_logit and loss are NULL together or not at all");
  if (int rc = target_ok(wh, target)) return rc;
  if (int rc = loss_outputs_ok(wh, lse, target_logit, loss, false)) return rc;
  if (!target && !best_index) return fail(MRE_ERR_ARG, wh + ": nothing to write: target and best_* are all NULL");
  const size_t need = attend_workspace(n, rotations, h, w);
  if (int rc = workspace_ok(wh, workspace, workspace_bytes, need, "mre_attend_workspace")) return rc;
  // no output or workspace byte range may overlap an input (n < 2^31 envs of fewer than 2^31 cells of 4 B: below 2^64)
  const size_t cells = (size_t)rotations * h * w;
  const ByteRange ins[2] = {{logits, esize * (size_t)n * cells}, {target, 8 * (size_t)n}};
  const ByteRange outs[6] = {{best_index, 8 * (size_t)n}, {best_value, 4 * (size_t)n}, {lse, 4 * (size_t)n},
                             {target_logit, 4 * (size_t)n}, {loss, 4 * (size_t)n}, {workspace, need}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, wh + ": an output or the workspace overlaps an input");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(logits) || !is_device_ptr(workspace) ||
      (best_index && (!is_device_ptr(best_index) || !is_device_ptr(best_value))) ||
      (target && (!is_device_ptr(target) || !is_device_ptr(lse) || !is_device_ptr(target_logit) || !is_device_ptr(loss))))
    return fail(MRE_ERR_ARG, wh + ": logits, target, the outputs and the workspace must be device pointers");
  AttendArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.target = target; a.best_index = best_index; a.best_value = best_value;
  a.lse = lse; a.target_logit = target_logit; a.loss = loss; a.workspace = workspace;
  a.n = (uint32_t)n; a.cells = (uint32_t)cells; a.bf16 = dtype == MRE_BF16 ? 1u : 0u;
  mre_launch_attend(&a, (hipStream_t)stream);
  return launched();
}

extern "C" int mre_attend_dlogits(void* stream, const void* logits, int n, int rotations, int h, int w, int dtype,
                                  const int64_t* target, const float* lse, const float* weight, void* g) {
  const std::string wh("mre_attend_dlogits");
  if (int rc = attend_ranges(wh, n, rotations, h, w, dtype)) return rc;
  const size_t esize = element_size(dtype);
  if (!logits || !target || !lse) return fail(MRE_ERR_ARG, wh + ": null logits, target or lse");
  if ((uintptr_t)logits & (esize - 1)) return fail(MRE_ERR_ARG, wh + ": logits must be aligned to its element size");
  if (int rc = target_ok(wh, target)) return rc;
  if (((uintptr_t)lse & 3) || ((uintptr_t)weight & 3)) return fail(MRE_ERR_ARG, wh + ": lse and weight must be 4-byte aligned");
  if (!g || ((uintptr_t)g & (esize - 1))) return fail(MRE_ERR_ARG, wh + ": g must be non-NULL and aligned to its element size");
  // (lengths below 2^64, as in mre_attend)
  const size_t cells = (size_t)rotations * h * w;
  const ByteRange ins[4] = {{logits, esize * (size_t)n * cells}, {target, 8 * (size_t)n}, {lse, 4 * (size_t)n},
                            {weight, 4 * (size_t)n}};
  const ByteRange outs[1] = {{g, esize * (size_t)n * cells}};
  if (ranges_overlap(ins, outs)) return fail(MRE_ERR_ARG, wh + ": g overlaps an input");
  if (n == 0) return MRE_OK;
  if (!is_device_ptr(logits) || !is_device_ptr(target) || !is_device_ptr(lse) || (weight && !is_device_ptr(weight)) ||
      !is_device_ptr(g))
    return fail(MRE_ERR_ARG, wh + ": logits, target, lse, weight and g must be device pointers");
  AttendGradArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.target = target; a.lse = lse; a.weight = weight; a.g = g;
  a.n = (uint32_t)n; a.cells = (uint32_t)cells; a.bf16 = dtype == MRE_BF16 ? 1u : 0u;
  mre_launch_attend_dlogits(&a, (hipStream_t)stream);
  return launched();
}

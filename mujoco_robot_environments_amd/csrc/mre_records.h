// Episode-record encoding and decoding on the device (csrc/mre_records.hip): packed varints of uint8 rows,
// their inverse, and CRC-32C of rows, for the TFRecord shards of dataset.py.  Shared between the kernels' translation
// unit and the C ABI (mre_stream_api.cpp); NOT part of lib.source_hash(): nothing here is launched by the
// step or the camera.
#ifndef MRE_RECORDS_H
#define MRE_RECORDS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr uint32_t REC_PACK_SEG = 4096;   // input bytes of a row one workgroup packs (<= 8192 packed bytes, staged in LDS)
constexpr uint32_t REC_CRC_SEG = 8192;    // bytes of a row one workgroup checksums (k_crc32c_rows)
constexpr size_t REC_MAX_ROW_BYTES = (size_t)1 << 30;   // a packed row's length stays below 2^32
constexpr uint32_t REC_UNPACK_SEG = 4096; // packed bytes of a row one workgroup unpacks (<= 4096 values, staged in LDS)
constexpr size_t REC_MAX_PACKED_BYTES = (size_t)1 << 31;   // of one row of mre_varint_unpack_rows: its counts fit 32 bits

struct RecArgs {
  const uint8_t* src;      // [src_rows][stride] bytes, row_bytes of each row are read
  size_t stride;
  uint32_t row_bytes;
  const int32_t* idx;      // [rows] source row of each output row (clamped to src_rows - 1) or null = identity
  uint32_t src_rows;
  uint32_t rows;
  uint32_t nseg;           // segments per row
  uint8_t* out;            // packed bytes of all rows, contiguous, row order
  long long* off;          // [rows] offset of each row in out
  uint32_t* len;           // [rows] packed length of each row
  uint32_t* crc;           // [rows] CRC-32C (standard form) of each row's output bytes
  uint32_t* segoff;        // [rows][nseg] workspace: count of values >= 128 per segment, then the segment's offset in its row
  uint32_t* segcrc;        // [rows][nseg] workspace: raw (zero initial value, no final xor) CRC of each segment
};

// mre_varint_unpack_rows: rows are described by four device arrays, not by a stride (mre.h)
struct UnpackArgs {
  const uint8_t* src;        // the file's bytes
  size_t src_bytes;
  const long long* src_off;  // [rows] packed bytes of row r: src[src_off[r] .. + src_len[r])
  const long long* src_len;
  const long long* nvalues;  // [rows] values expected
  const long long* out_off;  // [rows] values of row r: out[out_off[r] .. + nvalues[r])
  size_t max_src_len;        // the host's bound on src_len[]: the grid is sized by it, a longer row is a bad descriptor
  uint32_t rows;
  uint32_t nseg;             // segments of a row of max_src_len bytes
  uint8_t* out;
  size_t out_capacity;
  uint32_t* status;          // [rows] MRE_UNPACK_* bits
  uint32_t* segoff;          // [rows][nseg] workspace: values that start in each segment, then the segment's first value index
};

// status bits of mre_varint_unpack_rows; include/mre.h names them MRE_UNPACK_* for callers
constexpr uint32_t REC_UNPACK_LONG = 1, REC_UNPACK_OVERFLOW = 2, REC_UNPACK_TRUNCATED = 4, REC_UNPACK_COUNT = 8,
                   REC_UNPACK_DESC = 16;

extern "C" void mre_launch_varint_unpack(const UnpackArgs* a, hipStream_t stream);
// count + scan: len, off (and segoff) only
extern "C" void mre_launch_varint_size(const RecArgs* a, hipStream_t stream);
// pack + fold, after mre_launch_varint_size on the same stream: out, crc
extern "C" void mre_launch_varint_pack(const RecArgs* a, hipStream_t stream);
extern "C" void mre_launch_crc32c_rows(const RecArgs* a, hipStream_t stream);
extern "C" uint32_t mre_rec_crc32c_combine(uint32_t crc_a, uint32_t crc_b, size_t len_b);
#endif

// Episode-record encoding on the device: the two per-byte stages of dataset.py's shard writer.
//
//   * packed varints of uint8 rows (TFDS stores a uint8 tensor as an int64_list: one varint per pixel byte;
//     v < 128 -> v, v >= 128 -> v, 1).  A row is cut into segments of REC_PACK_SEG input bytes, one workgroup each:
//       k_varint_count    values >= 128 per segment
//       k_varint_scan     per row: exclusive scan of the counts -> each segment's offset in its row, the row's length
//       k_varint_offsets  exclusive scan of the row lengths -> 64-bit row offsets
//       k_varint_pack     the segment's output is put together in LDS (positions from ballots over the wave), its CRC
//                         is taken from LDS, and it leaves as aligned dwords
//       k_crc32c_fold     per row: the segments' CRCs folded into the row's
//   * CRC-32C of raw rows (a float32 frame's bytes are a packed float_list as they are): k_crc32c_rows + the fold.
//
// CRC arithmetic: the reflected Castagnoli polynomial, a register value read as a polynomial over GF(2) with bit 31 the
// coefficient of x^0.  raw(M) is the register after M from a zero start; raw(A || B) = raw(A) * x^(8 |B|) + raw(B), and
// leading zero bytes leave raw() unchanged.  So a segment is laid out right-aligned in its staging buffer, every thread
// takes the raw CRC of one fixed chunk of the buffer, multiplies it by the constant x^(8 * bytes behind the chunk) and the
// workgroup xors the products.  The standard CRC of a row of n bytes is raw(row) + 0xFFFFFFFF * x^(8 n) + 0xFFFFFFFF.
#include "mre_records.h"

namespace {

constexpr uint32_t POLY = 0x82F63B78u;
constexpr int NT = 256;                        // threads per workgroup, every kernel here
constexpr uint32_t STG = 2 * REC_PACK_SEG;     // staging bytes: the worst case of a packed segment
constexpr uint32_t CHUNK = STG / NT;           // staging bytes per thread in the CRC pass
static_assert(REC_CRC_SEG == STG, "k_crc32c_rows stages one segment in the same buffer");
static_assert(CHUNK == 32, "K[] below is built for 32-byte chunks");

// a * b mod P
__host__ __device__ constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
  }
  return p;
}

struct Tables {
  uint32_t T[4][256];   // slicing-by-4 tables
  uint32_t K[NT];       // x^(8 * CHUNK * (NT - 1 - t)): what thread t's chunk is multiplied by
  uint32_t X2N[68];     // x^(2^k), for every bit of 8 * (a 64-bit length)
};

constexpr Tables make_tables() {
  Tables t = {};
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? POLY : 0u);
    t.T[0][i] = c;
  }
  for (int k = 1; k < 4; k++)
    for (uint32_t i = 0; i < 256; i++) t.T[k][i] = (t.T[k - 1][i] >> 8) ^ t.T[0][t.T[k - 1][i] & 0xFFu];
  t.X2N[0] = 0x40000000u;   // x^1
  for (int k = 1; k < 68; k++) t.X2N[k] = mulmod(t.X2N[k - 1], t.X2N[k - 1]);
  t.K[NT - 1] = 0x80000000u;   // x^0
  for (int i = NT - 2; i >= 0; i--) t.K[i] = mulmod(t.K[i + 1], t.X2N[8]);   // * x^256 = x^(8 * CHUNK)
  return t;
}

constexpr Tables H_TAB = make_tables();
__device__ const Tables g_tab = make_tables();

// x^(8 n) mod P
__device__ inline uint32_t xpow8(uint64_t n) {
  uint32_t p = 0x80000000u;
  for (int k = 3; n; n >>= 1, k++)
    if (n & 1) p = mulmod(g_tab.X2N[k], p);
  return p;
}

__device__ inline uint32_t wave_xor(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d);
  return v;
}

__device__ inline size_t src_row(const RecArgs& a, uint32_t r) {
  if (!a.idx) return r;
  const uint32_t i = (uint32_t)a.idx[r];        // a negative index is a large one
  return i < a.src_rows ? i : a.src_rows - 1;
}

// the four dwords a thread owns of a pack segment: wave w holds bytes [1024 w, 1024 w + 1024) of the segment, lane l
// of it the dword 64 j + l of that quarter for j = 0..3; bytes past the segment's end read as 0
__device__ inline void load_quarter(const uint8_t* src, uint32_t nin, int wave, int lane, uint32_t w[4]) {
  const bool aligned = ((uintptr_t)src & 3) == 0;
  for (int j = 0; j < 4; j++) {
    const uint32_t b0 = 4u * (uint32_t)(wave * 256 + j * 64 + lane);
    uint32_t v = 0;
    if (b0 + 4 <= nin && aligned) {
      v = *(const uint32_t*)(src + b0);
    } else {
      for (uint32_t b = 0; b < 4; b++)
        if (b0 + b < nin) v |= (uint32_t)src[b0 + b] << (8 * b);
    }
    w[j] = v;
  }
}

__global__ __launch_bounds__(NT) void k_varint_count(RecArgs a) {
  __shared__ uint32_t s_sum[NT / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t r = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  const uint8_t* src = a.src + src_row(a, r) * a.stride + (size_t)s * REC_PACK_SEG;
  const uint32_t left = a.row_bytes - s * REC_PACK_SEG;
  const uint32_t nin = left < REC_PACK_SEG ? left : REC_PACK_SEG;
  uint32_t w[4];
  load_quarter(src, nin, wave, lane, w);
  uint32_t c = 0;
  for (int j = 0; j < 4; j++) c += __popc(w[j] & 0x80808080u);
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if (lane == 0) s_sum[wave] = c;
  __syncthreads();
  if (tid == 0) a.segoff[(size_t)r * a.nseg + s] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// exclusive scan of NT values through LDS; returns the value before this thread's, *total = the sum of all
template <typename T>
__device__ inline T block_exscan(T v, T* s_buf, T* total) {
  const int tid = threadIdx.x;
  __syncthreads();   // s_buf may still be read from the previous call
  s_buf[tid] = v;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const T add = tid >= d ? s_buf[tid - d] : (T)0;
    __syncthreads();
    s_buf[tid] += add;
    __syncthreads();
  }
  *total = s_buf[NT - 1];
  return s_buf[tid] - v;
}

// one workgroup per row: counts -> segment offsets in the row (in place), len[r]
__global__ __launch_bounds__(NT) void k_varint_scan(RecArgs a) {
  __shared__ uint32_t s_buf[NT];
  const int tid = threadIdx.x;
  const uint32_t r = blockIdx.x;
  uint32_t* seg = a.segoff + (size_t)r * a.nseg;
  uint32_t carry = 0;
  for (uint32_t s0 = 0; s0 < a.nseg; s0 += NT) {
    const uint32_t s = s0 + tid;
    const uint32_t c = s < a.nseg ? seg[s] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exscan(c, s_buf, &tot);
    if (s < a.nseg) seg[s] = s * REC_PACK_SEG + carry + ex;
    carry += tot;
  }
  if (tid == 0) a.len[r] = a.row_bytes + carry;
}

// one workgroup: row lengths -> 64-bit row offsets
__global__ __launch_bounds__(NT) void k_varint_offsets(RecArgs a) {
  __shared__ unsigned long long s_buf[NT];
  const int tid = threadIdx.x;
  unsigned long long carry = 0;
  for (uint32_t r0 = 0; r0 < a.rows; r0 += NT) {
    const uint32_t r = r0 + tid;
    const unsigned long long n = r < a.rows ? a.len[r] : 0ull;
    unsigned long long tot;
    const unsigned long long ex = block_exscan(n, s_buf, &tot);
    if (r < a.rows) a.off[r] = (long long)(carry + ex);
    carry += tot;
  }
}

__device__ inline void load_crc_tables(uint32_t* s_T, int tid) {
  for (int k = 0; k < 4; k++) s_T[k * 256 + tid] = g_tab.T[k][tid];
}

// raw CRC of the staging buffer's bytes [base, STG) (the bytes of base's chunk in front of base are zero); the result is
// valid in thread 0.  Ends with the workgroup's threads past a barrier.
__device__ inline uint32_t stage_crc(const uint32_t* s_stage, const uint32_t* s_T, uint32_t* s_red, uint32_t base, int tid) {
  uint32_t c = 0;
  if ((uint32_t)(tid + 1) * CHUNK > base) {
    const uint32_t* p = s_stage + tid * (CHUNK / 4);
    for (uint32_t k = 0; k < CHUNK / 4; k++) {
      c ^= p[k];
      c = s_T[3 * 256 + (c & 0xFFu)] ^ s_T[2 * 256 + ((c >> 8) & 0xFFu)] ^ s_T[256 + ((c >> 16) & 0xFFu)] ^ s_T[c >> 24];
    }
    c = mulmod(c, g_tab.K[tid]);
  }
  c = wave_xor(c);
  if ((tid & 63) == 0) s_red[tid >> 6] = c;
  __syncthreads();
  return s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3];
}

__global__ __launch_bounds__(NT) void k_varint_pack(RecArgs a) {
  __shared__ uint32_t s_stage[STG / 4 + 1];   // + 1: the unaligned read-out looks one dword ahead
  __shared__ uint32_t s_T[4 * 256];
  __shared__ uint32_t s_sum[NT / 64];
  __shared__ uint32_t s_red[NT / 64];
  uint8_t* sb = (uint8_t*)s_stage;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t r = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  const size_t seg_i = (size_t)r * a.nseg + s;
  const uint8_t* src = a.src + src_row(a, r) * a.stride + (size_t)s * REC_PACK_SEG;
  const uint32_t left = a.row_bytes - s * REC_PACK_SEG;
  const uint32_t nin = left < REC_PACK_SEG ? left : REC_PACK_SEG;
  const uint32_t segoff = a.segoff[seg_i];
  const uint32_t segend = s + 1 < a.nseg ? a.segoff[seg_i + 1] : a.len[r];
  const uint32_t nout = segend - segoff;
  if (nout > STG || nout < nin) return;   // cannot happen unless the source changed since the count pass
  const uint32_t base = STG - nout;

  load_crc_tables(s_T, tid);
  if ((uint32_t)tid < (base & (CHUNK - 1))) sb[(base & ~(CHUNK - 1)) + tid] = 0;
  if (tid == 0) s_stage[STG / 4] = 0;

  uint32_t w[4], pre[4];
  load_quarter(src, nin, wave, lane, w);
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t run = 0;   // values >= 128 in this wave's quarter, in front of dword j
  for (int j = 0; j < 4; j++) {
    const uint32_t c = __popc(w[j] & 0x80808080u);   // 0..4
    const unsigned long long b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
    pre[j] = run + __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below);
    run += __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  }
  if (lane == 0) s_sum[wave] = run;
  __syncthreads();
  uint32_t wbase = 0;
  for (int v = 0; v < wave; v++) wbase += s_sum[v];
  for (int j = 0; j < 4; j++) {
    const uint32_t b0 = 4u * (uint32_t)(wave * 256 + j * 64 + lane);
    uint32_t pos = base + b0 + wbase + pre[j];
    for (uint32_t b = 0; b < 4; b++) {
      if (b0 + b >= nin) break;
      const uint32_t v = (w[j] >> (8 * b)) & 0xFFu;
      if (pos < STG) sb[pos] = (uint8_t)v;     // (v & 0x7f) | 0x80 == v for v >= 128
      pos++;
      if (v >= 128u) {
        if (pos < STG) sb[pos] = 1;            // v >> 7
        pos++;
      }
    }
  }
  __syncthreads();

  const uint32_t crc = stage_crc(s_stage, s_T, s_red, base, tid);
  if (tid == 0) a.segcrc[seg_i] = crc;

  // out: head bytes up to a dword boundary of the destination, dwords, tail bytes
  uint8_t* dst = a.out + (size_t)a.off[r] + segoff;
  uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3)) & 3u;
  if (head > nout) head = nout;
  if ((uint32_t)tid < head) dst[tid] = sb[base + tid];
  const uint32_t nd = (nout - head) >> 2, q = base + head, m8 = 8u * (q & 3u);
  const uint32_t* lw = s_stage + (q >> 2);
  uint32_t* dw = (uint32_t*)(dst + head);
  for (uint32_t k = tid; k < nd; k += NT) {
    uint32_t v = lw[k];
    if (m8) v = (v >> m8) | (lw[k + 1] << (32u - m8));
    dw[k] = v;
  }
  const uint32_t tail = (nout - head) & 3u;
  if ((uint32_t)tid < tail) dst[head + 4 * nd + tid] = sb[q + 4 * nd + tid];
}

// raw CRC of segment s (REC_CRC_SEG bytes) of every row
__global__ __launch_bounds__(NT) void k_crc32c_rows(RecArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[STG / 4];
  __shared__ uint32_t s_T[4 * 256];
  __shared__ uint32_t s_red[NT / 64];
  uint8_t* sb = (uint8_t*)s_stage;
  const int tid = threadIdx.x;
  const uint32_t r = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  const uint8_t* src = a.src + src_row(a, r) * a.stride + (size_t)s * REC_CRC_SEG;
  const uint32_t left = a.row_bytes - s * REC_CRC_SEG;
  const uint32_t nin = left < REC_CRC_SEG ? left : REC_CRC_SEG;
  const uint32_t base = STG - nin;
  load_crc_tables(s_T, tid);
  if ((uint32_t)tid < (base & (CHUNK - 1))) sb[(base & ~(CHUNK - 1)) + tid] = 0;
  if ((((uintptr_t)src | nin) & 15) == 0) {
    const uint4* g = (const uint4*)src;
    uint4* l = (uint4*)(sb + base);
    for (uint32_t k = tid; k < nin / 16; k += NT) l[k] = g[k];
  } else if ((((uintptr_t)src | nin) & 3) == 0) {
    const uint32_t* g = (const uint32_t*)src;
    uint32_t* l = (uint32_t*)(sb + base);
    for (uint32_t k = tid; k < nin / 4; k += NT) l[k] = g[k];
  } else {
    for (uint32_t k = tid; k < nin; k += NT) sb[base + k] = src[k];
  }
  __syncthreads();
  const uint32_t crc = stage_crc(s_stage, s_T, s_red, base, tid);
  if (tid == 0) a.segcrc[(size_t)r * a.nseg + s] = crc;
}

// one workgroup per row: crc[r] from the segments' raw CRCs.  seg_bytes = 0: segment ends from segoff / len (varints);
// otherwise fixed segments of seg_bytes over row_bytes.
__global__ __launch_bounds__(NT) void k_crc32c_fold(RecArgs a, uint32_t seg_bytes) {
  __shared__ uint32_t s_red[NT / 64];
  const int tid = threadIdx.x;
  const uint32_t r = blockIdx.x;
  const size_t row0 = (size_t)r * a.nseg;
  const uint32_t n = seg_bytes ? a.row_bytes : a.len[r];
  uint32_t acc = 0;
  for (uint32_t s = tid; s < a.nseg; s += NT) {
    uint32_t end = n;
    if (s + 1 < a.nseg) end = seg_bytes ? (s + 1) * seg_bytes : a.segoff[row0 + s + 1];
    const uint32_t c = a.segcrc[row0 + s];
    if (c) acc ^= mulmod(c, xpow8(n - end));
  }
  acc = wave_xor(acc);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)
    a.crc[r] = s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3] ^ mulmod(0xFFFFFFFFu, xpow8(n)) ^ 0xFFFFFFFFu;
}

}  // namespace

extern "C" void mre_launch_varint_size(const RecArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(k_varint_count, dim3(a->rows * a->nseg), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_varint_scan, dim3(a->rows), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_varint_offsets, dim3(1), dim3(NT), 0, stream, *a);
}

extern "C" void mre_launch_varint_pack(const RecArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(k_varint_pack, dim3(a->rows * a->nseg), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_crc32c_fold, dim3(a->rows), dim3(NT), 0, stream, *a, 0u);
}

extern "C" void mre_launch_crc32c_rows(const RecArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(k_crc32c_rows, dim3(a->rows * a->nseg), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_crc32c_fold, dim3(a->rows), dim3(NT), 0, stream, *a, (uint32_t)REC_CRC_SEG);
}

// CRC of A || B from the standard CRCs of A and B: crc_a * x^(8 len_b) + crc_b
extern "C" uint32_t mre_rec_crc32c_combine(uint32_t crc_a, uint32_t crc_b, size_t len_b) {
  uint32_t p = 0x80000000u;
  unsigned long long n = len_b;
  for (int k = 3; n; n >>= 1, k++)
    if (n & 1) p = mulmod(H_TAB.X2N[k], p);
  return mulmod(p, crc_a) ^ crc_b;
}

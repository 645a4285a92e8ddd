// Episode-record encoding on the device: the two per-byte stages of dataset.py's shard writer, and (further down) the
// inverse of the first for its reader.
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

// ---------------------------------------------------------------- the inverse: packed varints -> uint8 rows
// A uint8 value is one byte v < 128, or two bytes v | 0x80, v >> 7.  So byte i of a row starts a value iff i == 0 or byte
// i - 1 has its high bit clear: a local test with one byte of look-behind, across dwords, waves and segments.  The value
// is (b[i] & 0x7f) | (b[i] & 0x80 ? b[i + 1] << 7 : 0), its index the number of start bytes in front of it:
//     k_unpack_desc     status[r] = 0, or MRE_UNPACK_DESC for a descriptor outside src / out (such a row is skipped by
//                       every kernel below: nothing of it is read or written)
//     k_varint_ucount   start bytes per segment of REC_UNPACK_SEG packed bytes; the malformed-input bits
//     k_varint_uscan    per row: exclusive scan of the counts -> each segment's first value index; the count bit
//     k_varint_unpack   the segment's values are put together in LDS (positions from ballots over the wave) at the byte
//                       phase of their destination, and leave as aligned dwords with head and tail bytes
// The bytes are outside input: every load is bounded by the row's own descriptor, which k_unpack_desc's rule holds inside
// src; every store by the row's nvalues (a row with too many start bytes is clipped and flagged).  Encodings this writer
// and TFDS never emit are flagged rather than decoded: a varint of three bytes or more (also a non-canonical zero such
// as 80 80 00), a second byte above 1.  80 00 decodes to 0 unflagged.
static_assert(REC_UNPACK_SEG == REC_PACK_SEG, "load_quarter spreads REC_PACK_SEG bytes over the workgroup");

struct UnpackRow {
  const uint8_t* src;
  uint8_t* out;
  uint32_t len;               // packed bytes (<= REC_MAX_PACKED_BYTES)
  unsigned long long nvalues;
};

__device__ inline bool unpack_row(const UnpackArgs& a, uint32_t r, UnpackRow* d) {
  const long long so = a.src_off[r], sl = a.src_len[r], nv = a.nvalues[r], oo = a.out_off[r];
  if (so < 0 || sl < 0 || nv < 0 || oo < 0) return false;
  if ((unsigned long long)sl > a.max_src_len) return false;
  if ((unsigned long long)so > a.src_bytes || (unsigned long long)sl > a.src_bytes - (unsigned long long)so) return false;
  if ((unsigned long long)oo > a.out_capacity || (unsigned long long)nv > a.out_capacity - (unsigned long long)oo) return false;
  d->src = a.src + so;
  d->out = a.out + oo;
  d->len = (uint32_t)sl;
  d->nvalues = (unsigned long long)nv;
  return true;
}

__global__ __launch_bounds__(NT) void k_unpack_desc(UnpackArgs a) {
  const uint32_t r = blockIdx.x * NT + threadIdx.x;
  if (r >= a.rows) return;
  UnpackRow d;
  a.status[r] = unpack_row(a, r, &d) ? 0u : REC_UNPACK_DESC;
}

// the segment's dwords as load_quarter lays them out, and for each the mask (bit 7 of every byte) of the bytes that start
// a value.  seg = the segment's first byte, pos = its index in the row, nin = its bytes.  err collects the malformed bits.
__device__ inline void load_starts(const uint8_t* seg, uint32_t pos, uint32_t nin, int wave, int lane, uint32_t w[4],
                                   uint32_t st[4], uint32_t* err) {
  load_quarter(seg, nin, wave, lane, w);
  uint32_t e = 0;
  for (int j = 0; j < 4; j++) {
    const uint32_t b0 = 4u * (uint32_t)(wave * 256 + j * 64 + lane);
    uint32_t prev = __shfl_up(w[j], 1) >> 24;            // the byte in front of this dword: the lane below holds it,
    if (lane == 0) prev = (b0 < nin && pos + b0 > 0) ? (seg + b0)[-1] : 0u;   // or memory does (inside the row: pos + b0 > 0;
                                                                              // b0 - 1 as an unsigned index would wrap at b0 = 0)
    const uint32_t nb = b0 >= nin ? 0u : (nin - b0 < 4u ? nin - b0 : 4u);
    const uint32_t vm = nb == 4u ? 0x80808080u : (0x80808080u & ((1u << (8u * nb)) - 1u));
    const uint32_t h = w[j] & 0x80808080u;               // bytes past nin are zero
    const uint32_t ph = (h << 8) | (prev & 0x80u);       // high bit of each byte's predecessor
    st[j] = ~ph & vm;
    if (h & ph) e |= REC_UNPACK_LONG;
    const uint32_t second = ((ph & ~h & vm) >> 7) * 0xFFu;   // the bytes that are a value's second byte
    if (w[j] & second & 0xFEFEFEFEu) e |= REC_UNPACK_OVERFLOW;
  }
  *err = e;
}

__global__ __launch_bounds__(NT) void k_varint_ucount(UnpackArgs a) {
  __shared__ uint32_t s_sum[NT / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t r = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  UnpackRow d;
  if (!unpack_row(a, r, &d)) return;
  const unsigned long long pos64 = (unsigned long long)s * REC_UNPACK_SEG;
  if (pos64 >= d.len) return;                 // a shorter row than the longest
  const uint32_t pos = (uint32_t)pos64, left = d.len - pos;
  const uint32_t nin = left < REC_UNPACK_SEG ? left : REC_UNPACK_SEG;
  uint32_t w[4], st[4], err;
  load_starts(d.src + pos, pos, nin, wave, lane, w, st, &err);
  if (left <= REC_UNPACK_SEG) {               // the row's last byte: a value may not be open behind it
    const uint32_t last = nin - 1;
    for (int j = 0; j < 4; j++)
      if ((last & ~3u) == 4u * (uint32_t)(wave * 256 + j * 64 + lane) && ((w[j] >> (8u * (last & 3u))) & 0x80u))
        err |= REC_UNPACK_TRUNCATED;
  }
  uint32_t c = 0;
  for (int j = 0; j < 4; j++) c += __popc(st[j]);
  for (int k = 32; k >= 1; k >>= 1) {
    c += __shfl_xor(c, k);
    err |= __shfl_xor(err, k);
  }
  if (lane == 0) {
    s_sum[wave] = c;
    if (err) atomicOr(&a.status[r], err);
  }
  __syncthreads();
  if (tid == 0) a.segoff[(size_t)r * a.nseg + s] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// one workgroup per row: counts -> each segment's first value index (in place); the total against nvalues
__global__ __launch_bounds__(NT) void k_varint_uscan(UnpackArgs a) {
  __shared__ uint32_t s_buf[NT];
  const int tid = threadIdx.x;
  const uint32_t r = blockIdx.x;
  UnpackRow d;
  if (!unpack_row(a, r, &d)) return;
  const uint32_t nseg = (uint32_t)(((unsigned long long)d.len + REC_UNPACK_SEG - 1) / REC_UNPACK_SEG);   // <= a.nseg
  uint32_t* seg = a.segoff + (size_t)r * a.nseg;
  uint32_t carry = 0;                          // <= len < 2^32
  for (uint32_t s0 = 0; s0 < nseg; s0 += NT) {
    const uint32_t s = s0 + tid;
    const uint32_t c = s < nseg ? seg[s] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exscan(c, s_buf, &tot);
    if (s < nseg) seg[s] = carry + ex;
    carry += tot;
  }
  if (tid == 0 && (unsigned long long)carry != d.nvalues) atomicOr(&a.status[r], REC_UNPACK_COUNT);
}

__global__ __launch_bounds__(NT) void k_varint_unpack(UnpackArgs a) {
  __shared__ uint32_t s_stage[REC_UNPACK_SEG / 4 + 1];   // + 1: the values sit at the byte phase of their destination
  __shared__ uint32_t s_sum[NT / 64];
  uint8_t* sb = (uint8_t*)s_stage;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t r = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  UnpackRow d;
  if (!unpack_row(a, r, &d)) return;
  const unsigned long long pos64 = (unsigned long long)s * REC_UNPACK_SEG;
  if (pos64 >= d.len) return;
  const uint32_t pos = (uint32_t)pos64, left = d.len - pos;
  const uint32_t nin = left < REC_UNPACK_SEG ? left : REC_UNPACK_SEG;
  const uint8_t* seg = d.src + pos;
  const uint32_t first = a.segoff[(size_t)r * a.nseg + s];   // index in the row of the segment's first value
  uint8_t* dst = d.out + first;
  const uint32_t shift = (uint32_t)((uintptr_t)dst & 3);

  uint32_t w[4], st[4], pre[4], err;
  load_starts(seg, pos, nin, wave, lane, w, st, &err);
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t run = 0;   // start bytes in this wave's quarter, in front of dword j
  for (int j = 0; j < 4; j++) {
    const uint32_t c = __popc(st[j]);   // 0..4
    const unsigned long long b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
    pre[j] = run + __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below);
    run += __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  }
  if (lane == 0) s_sum[wave] = run;
  __syncthreads();
  uint32_t wbase = 0;
  for (int v = 0; v < wave; v++) wbase += s_sum[v];
  const uint32_t count = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];   // <= nin
  for (int j = 0; j < 4; j++) {
    const uint32_t b0 = 4u * (uint32_t)(wave * 256 + j * 64 + lane);
    uint32_t next = __shfl_down(w[j], 1) & 0xFFu;          // the byte behind this dword: the lane above holds it,
    if (lane == 63) next = (b0 + 4u < left) ? seg[b0 + 4] : 0u;   // or memory does (inside the row: pos + b0 + 4 < len)
    const uint32_t ext = (w[j] >> 8) | (next << 24);       // byte b of ext = the byte behind byte b of w[j]
    uint32_t p = wbase + pre[j];
    for (uint32_t b = 0; b < 4; b++) {
      if (!((st[j] >> (8 * b)) & 0x80u)) continue;
      const uint32_t v = (w[j] >> (8 * b)) & 0xFFu;
      const uint32_t hi = (v & 0x80u) ? ((ext >> (8 * b)) & 1u) << 7 : 0u;
      if (p < REC_UNPACK_SEG) sb[shift + p] = (uint8_t)((v & 0x7Fu) | hi);
      p++;
    }
  }
  __syncthreads();

  // out: clipped to the row's nvalues; head bytes up to a dword boundary of the destination, dwords, tail bytes
  const unsigned long long room = d.nvalues > first ? d.nvalues - first : 0ull;
  const uint32_t nout = (unsigned long long)count < room ? count : (uint32_t)room;
  uint32_t head = (4u - shift) & 3u;
  if (head > nout) head = nout;
  if ((uint32_t)tid < head) dst[tid] = sb[shift + tid];
  const uint32_t nd = (nout - head) >> 2;
  const uint32_t* lw = s_stage + ((shift + head) >> 2);   // shift + head is 0 or 4 when nd > 0
  uint32_t* dw = (uint32_t*)(dst + head);
  for (uint32_t k = tid; k < nd; k += NT) dw[k] = lw[k];
  const uint32_t tail = (nout - head) & 3u;
  if ((uint32_t)tid < tail) dst[head + 4 * nd + tid] = sb[shift + head + 4 * nd + tid];
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

extern "C" void mre_launch_varint_unpack(const UnpackArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(k_unpack_desc, dim3((a->rows + NT - 1) / NT), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_varint_ucount, dim3(a->rows * a->nseg), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_varint_uscan, dim3(a->rows), dim3(NT), 0, stream, *a);
  hipLaunchKernelGGL(k_varint_unpack, dim3(a->rows * a->nseg), dim3(NT), 0, stream, *a);
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

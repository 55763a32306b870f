// The text lists of the kNN export (reference: faiss_knn.py:267-305, `write_knn` / `write_process`) formatted on the device;
// the contract and the digit routine: include/cdml_knn_writer.h, DESIGN.md section 9a.1.
//
// The reference formats every kept (id, distance) pair with Python's string operators, one worker per file; knn.write_knn
// does the same on the host with one numpy str() pass per file.  Here a line is sized and written by one wave:
//
//   k_line_sizes   lane t owns columns 1 + t and 65 + t of its row (k <= 128): the keep test, the guid's length from the
//                  offset table, the length of the distance's shortest repr (integer arithmetic, the header's routine); a
//                  wave sum gives the line's bytes.  A kept distance outside the routine's range raises the row's flag.
//   k_line_write   the same per-lane lengths, an exclusive wave scan in column order, and every lane stores its entries'
//                  bytes (guid, '#', digits, '<') at its scanned offset; the row's own guid goes lane-strided, ',' and
//                  '\n' from lane 0.  Every store is clipped to the row's extent [off[r], off[r + 1]) and to the buffer.
//
// Rows are independent, nothing is accumulated across waves: no atomics, the bytes are a function of the inputs only.
#include "common.h"
#include "../../include/cdml_knn_writer.h"

namespace cdml {
namespace {

constexpr int kWriterMaxCols = CDML_KNN_LIST;   // 128: two columns per lane
constexpr int kRowsPerBlock = 4;                // one wave per row, four waves per block

// guid i's bytes [b, e) of the table, or an empty range where the offsets are not a table's (never read outside it)
__device__ __forceinline__ void guid_range(const int64_t *__restrict__ goff, int64_t i, int64_t total, int64_t &b, int64_t &e) {
  b = goff[i];
  e = goff[i + 1];
  if (b < 0 || e < b || e > total) e = b = 0;
}

struct Entry {
  bool keep, digits;     // written at all; with a number (the distance is in the routine's range)
  int64_t gb, ge;        // its guid's bytes
  cdml_f32_dec dec;
  int64_t len;           // bytes: guid + '#' + number + '<', 0 when not kept
};

__device__ __forceinline__ Entry load_entry(const float *__restrict__ dr, const int64_t *__restrict__ ir, int c, int k,
                                            const int64_t *__restrict__ goff, int64_t n_guid, int64_t total) {
  Entry en;
  en.keep = en.digits = false;
  en.gb = en.ge = en.len = 0;
  en.dec.digits = 0;
  en.dec.p = 1;
  en.dec.k = 0;
  en.dec.sci = 0;
  if (c >= k) return en;
  const int64_t id = ir[c];
  const float d = dr[c];
  if (!(id > 0 && id < n_guid && d > 0.0f && d < 1.4f)) return en;   // (float32 compares; a NaN passes none)
  en.keep = true;
  guid_range(goff, id, total, en.gb, en.ge);
  en.len = (en.ge - en.gb) + 2;
  if (cdml_f32_shortest_in_range(d)) {
    en.digits = true;
    en.dec = cdml_f32_shortest_digits(d);
    en.len += cdml_f32_dec_length(en.dec);
  }
  return en;
}

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int delta) {
  const int lo = __shfl_up((int)(uint32_t)(uint64_t)v, delta, 64);
  const int hi = __shfl_up((int)(uint32_t)((uint64_t)v >> 32), delta, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const int lo = __shfl((int)(uint32_t)(uint64_t)v, src, 64);
  const int hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// inclusive scan over the wave's lanes
__device__ __forceinline__ int64_t wave_scan64(int64_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t u = shfl_up64(v, off);
    if (lane >= off) v += u;
  }
  return v;
}

__global__ void __launch_bounds__(64 * kRowsPerBlock)
k_line_sizes(const float *__restrict__ D, int64_t ldd, const int64_t *__restrict__ I, int64_t ldi, int64_t row0, int n_rows,
             int k, const int64_t *__restrict__ goff, int64_t n_guid, int64_t total, int64_t *__restrict__ sizes,
             int32_t *__restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= n_rows) return;                       // (wave-uniform)
  const float *dr = D + row * ldd;
  const int64_t *ir = I + row * ldi;
  const Entry a = load_entry(dr, ir, 1 + lane, k, goff, n_guid, total);
  const Entry b = load_entry(dr, ir, 65 + lane, k, goff, n_guid, total);
  const int64_t sum = shfl64(wave_scan64(a.len + b.len, lane), 63);
  const bool flag = (a.keep && !a.digits) || (b.keep && !b.digits);
  const unsigned long long any = __ballot(flag);
  if (lane == 0) {
    int64_t gb, ge;
    guid_range(goff, row0 + row, total, gb, ge);
    sizes[row] = (ge - gb) + 1 + sum + 1;
    flags[row] = any ? 1 : 0;
  }
}

struct Cursor {
  uint8_t *out;
  int64_t pos, lo, hi;   // the next byte; the row's extent, clipped to the buffer
  __device__ __forceinline__ void operator()(char c) {
    if (pos >= lo && pos < hi) out[pos] = (uint8_t)c;
    ++pos;
  }
};

__device__ __forceinline__ void write_entry(const Entry &en, const uint8_t *__restrict__ gbytes, Cursor &cur) {
  if (!en.keep) return;
  for (int64_t i = en.gb; i < en.ge; ++i) cur((char)gbytes[i]);
  cur('#');
  if (en.digits) cdml_f32_dec_emit(en.dec, [&](char c) { cur(c); });
  cur('<');
}

__global__ void __launch_bounds__(64 * kRowsPerBlock)
k_line_write(const float *__restrict__ D, int64_t ldd, const int64_t *__restrict__ I, int64_t ldi, int64_t row0, int n_rows,
             int k, const uint8_t *__restrict__ gbytes, const int64_t *__restrict__ goff, int64_t n_guid, int64_t total,
             const int64_t *__restrict__ off, uint8_t *__restrict__ out, int64_t out_bytes) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= n_rows) return;                       // (wave-uniform)
  const float *dr = D + row * ldd;
  const int64_t *ir = I + row * ldi;
  const Entry a = load_entry(dr, ir, 1 + lane, k, goff, n_guid, total);
  const Entry b = load_entry(dr, ir, 65 + lane, k, goff, n_guid, total);
  const int64_t sa = wave_scan64(a.len, lane), sb = wave_scan64(b.len, lane);
  const int64_t total_a = shfl64(sa, 63), total_b = shfl64(sb, 63);
  int64_t lo = off[row], hi = off[row + 1];
  if (lo < 0) lo = 0;
  if (hi > out_bytes) hi = out_bytes;
  int64_t gb, ge;
  guid_range(goff, row0 + row, total, gb, ge);
  const int64_t glen = ge - gb;
  Cursor cur{out, 0, lo, hi};
  for (int64_t i = lane; i < glen; i += 64) {      // the row's own guid, lane-strided
    cur.pos = off[row] + i;
    cur((char)gbytes[gb + i]);
  }
  const int64_t body = off[row] + glen + 1;
  if (lane == 0) {
    cur.pos = body - 1;
    cur(',');
    cur.pos = body + total_a + total_b;
    cur('\n');
  }
  cur.pos = body + (sa - a.len);                   // columns 1 .. 64 first, in lane order
  write_entry(a, gbytes, cur);
  cur.pos = body + total_a + (sb - b.len);         // then columns 65 .. 127
  write_entry(b, gbytes, cur);
}

int check_common(const char *what, const float *D, int64_t ldd, const int64_t *I, int64_t ldi, int64_t row0, int n_rows, int k,
                 const int64_t *guid_off, int64_t n_guid, int64_t guid_total) {
  CDML_REQUIRE(D && I && guid_off, CDML_E_BADARG, "%s: null pointer", what);
  CDML_REQUIRE(n_rows > 0 && row0 >= 0 && guid_total >= 0, CDML_E_BADARG, "%s: bad size (n_rows %d, row0 %lld, guid_total %lld)",
               what, n_rows, (long long)row0, (long long)guid_total);
  CDML_REQUIRE(k >= 1 && k <= kWriterMaxCols, CDML_E_UNSUPPORTED, "%s: k must be in [1, %d], got %d", what, kWriterMaxCols, k);
  CDML_REQUIRE(ldd >= k && ldi >= k, CDML_E_BADARG, "%s: row strides must be >= k", what);
  CDML_REQUIRE(row0 + n_rows <= n_guid, CDML_E_BADARG, "%s: rows [%lld, %lld) have no guid (n_guid %lld)", what, (long long)row0,
               (long long)(row0 + n_rows), (long long)n_guid);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_f32_shortest(float x, char *out) {
  if (!out || !cdml_f32_shortest_in_range(x)) return -1;
  const cdml_f32_dec d = cdml_f32_shortest_digits(x);
  int n = 0;
  cdml_f32_dec_emit(d, [&](char c) { out[n++] = c; });
  out[n] = 0;
  return n;
}

extern "C" int cdml_knn_line_sizes(const float *D, int64_t ldd, const int64_t *I, int64_t ldi, int64_t row0, int n_rows, int k,
                                   const int64_t *guid_off, int64_t n_guid, int64_t guid_total, int64_t *sizes,
                                   int32_t *flags, cdml_stream_t stream) {
  const int rc = check_common("knn_line_sizes", D, ldd, I, ldi, row0, n_rows, k, guid_off, n_guid, guid_total);
  if (rc != CDML_OK) return rc;
  CDML_REQUIRE(sizes && flags, CDML_E_BADARG, "knn_line_sizes: null pointer");
  const dim3 grid((unsigned)(((int64_t)n_rows + kRowsPerBlock - 1) / kRowsPerBlock));
  hipLaunchKernelGGL(k_line_sizes, grid, dim3(64 * kRowsPerBlock), 0, (hipStream_t)stream, D, ldd, I, ldi, row0, n_rows, k,
                     guid_off, n_guid, guid_total, sizes, flags);
  return check_launch("knn_line_sizes");
}

extern "C" int cdml_knn_line_write(const float *D, int64_t ldd, const int64_t *I, int64_t ldi, int64_t row0, int n_rows, int k,
                                   const uint8_t *guid_bytes, const int64_t *guid_off, int64_t n_guid, int64_t guid_total,
                                   const int64_t *off, uint8_t *out, int64_t out_bytes, cdml_stream_t stream) {
  const int rc = check_common("knn_line_write", D, ldd, I, ldi, row0, n_rows, k, guid_off, n_guid, guid_total);
  if (rc != CDML_OK) return rc;
  CDML_REQUIRE(off && out && (guid_bytes || guid_total == 0), CDML_E_BADARG, "knn_line_write: null pointer");
  CDML_REQUIRE(out_bytes >= 0, CDML_E_BADARG, "knn_line_write: out_bytes must be >= 0, got %lld", (long long)out_bytes);
  const dim3 grid((unsigned)(((int64_t)n_rows + kRowsPerBlock - 1) / kRowsPerBlock));
  hipLaunchKernelGGL(k_line_write, grid, dim3(64 * kRowsPerBlock), 0, (hipStream_t)stream, D, ldd, I, ldi, row0, n_rows, k,
                     guid_bytes, guid_off, n_guid, guid_total, off, out, out_bytes);
  return check_launch("knn_line_write");
}

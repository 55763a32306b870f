/* cdml_knn_writer.h -- the text lists of the kNN export formatted on the device: the C ABI of csrc/knn_writer.hip of
 * libcdml_hip.so and, for C++ translation units, the digit routine the kernels and the host entry point share (DESIGN.md
 * section 9a.1).  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on `stream`, status ints,
 * cdml_last_error()).
 *
 * A LINE of knn.write_knn (faiss_knn.py:267-305) for row r of D fp32 / I int64 [n_rows, k]:
 *     guid[row0 + r] + "," + sum over columns c = 1 .. k-1 that are KEPT of (guid[I[r][c]] + "#" + str(D[r][c]) + "<") + "\n"
 *   kept: I[r][c] > 0 and 0.0 < D[r][c] < 1.4f, as float32 compares (a NaN or an infinity is not kept); str = the shortest
 *   repr below.  guid i is the bytes guid_bytes[guid_off[i] .. guid_off[i + 1]) (utf-8 as the host encoded it: any length,
 *   0 included).  An id >= n_guid is not kept (the host path refuses such a table before anything is launched).
 *
 * cdml_knn_line_sizes   sizes[r] = the byte length of row r's line; flags[r] = 1 when a kept D[r][c] lies outside the digit
 *                       routine's range (below), else 0 (such an entry counts "#" and "<" and no digits: the caller formats
 *                       the rows of a flagged part on the host).
 * cdml_knn_line_write   the bytes of row r into out[off[r] .. off[r + 1]), off int64 [n_rows + 1] = the exclusive scan of
 *                       sizes.  Every store is bounded by [max(off[r], 0), min(off[r + 1], out_bytes)): a row never writes
 *                       outside its own extent, whatever off holds.
 * Both: one wave per row, two columns per lane (k <= 128 = cdml_knn_list_capacity()), no atomics; the output is a function
 * of the inputs.  Bad arguments (a null pointer, n_rows < 1, k outside [1, 128], a row stride < k, row0 < 0,
 * row0 + n_rows > n_guid, guid_total < 0, out_bytes < 0) return a negative status before any HIP call.
 *
 * THE SHORTEST REPR (cdml_f32_shortest): the text numpy's str(np.float32(x)) gives, for CDML_F32_SHORTEST_MIN <= x <
 * CDML_F32_SHORTEST_MAX, i.e. 2^-64 (5.42e-20) <= x < 2.  Outside that range the host entry point returns -1 and the
 * launches flag the row.
 *   x = m 2^-s exactly (m < 2^24 the significand, 23 <= s <= 87).  j = the smallest j >= 0 with m 10^j >= 2^s, so that
 *   x 10^j lies in [1, 10) and -j is x's decimal exponent.  Digits are peeled off N = m 10^j: d = N >> s, r = N mod 2^s,
 *   then r <- 10 r, with the half gap to the neighbouring floats carried in the same units, M = 10^(j + p - 1): after p
 *   digits the truncated decimal reads back as x iff 2 r < M (4 r < M where m = 2^23: the float below is half as far), the
 *   decimal one unit higher iff 2 r + M > 2^(s + 1) (strict compares: in this range no decimal of <= 9 digits lies ON a
 *   boundary between two floats, which have >= 24 binary places).  The first p at which either holds is the digit count
 *   (p <= 9 always for a float32); where both hold the nearer wins, 2 r against 2^s, a tie to the even digit; a carry into
 *   a run of nines shortens the digits (1.29999995 -> 1.3), one out of it moves the decade (9.99999975e-05 -> 1e-04).  This
 *   is the free-format Dragon4 walk (Steele & White; Burger & Dybvig) in fixed-width integers: N < 10 * 2^87, 10 r <
 *   10 * 2^87, M <= 10^28 < 2^94, 2 r + M < 2^96 -- everything fits an unsigned 128-bit integer, nothing is rounded, there
 *   is no floating-point operation and no "rare" error.
 *   Layout, numpy's: positional where x >= 1e-4 ("0.00012", "1.0", "1.25": digits, a point, at least one digit behind it),
 *   scientific below ("1e-05", "9.999e-05": no point for one digit, a sign and at least two exponent digits); the switch is
 *   on x itself (j <= 4), not on the rounded digits.  At most CDML_F32_SHORTEST_CHARS = 14 characters. */
#ifndef CDML_KNN_WRITER_H_
#define CDML_KNN_WRITER_H_

#include "cdml.h"

#define CDML_F32_SHORTEST_MIN 0x1p-64f
#define CDML_F32_SHORTEST_MAX 2.0f
#define CDML_F32_SHORTEST_CHARS 14

#ifdef __cplusplus
extern "C" {
#endif

/* out: at least CDML_F32_SHORTEST_CHARS + 1 bytes; the text and a terminating 0.  Returns the length, or -1 (nothing written)
 * for an x outside the range.  Host only; touches no device. */
int cdml_f32_shortest(float x, char *out);

int cdml_knn_line_sizes(const float *D, int64_t ldd, const int64_t *I, int64_t ldi, int64_t row0, int n_rows, int k,
                        const int64_t *guid_off, int64_t n_guid, int64_t guid_total, int64_t *sizes, int32_t *flags,
                        cdml_stream_t stream);
int cdml_knn_line_write(const float *D, int64_t ldd, const int64_t *I, int64_t ldi, int64_t row0, int n_rows, int k,
                        const uint8_t *guid_bytes, const int64_t *guid_off, int64_t n_guid, int64_t guid_total,
                        const int64_t *off, uint8_t *out, int64_t out_bytes, cdml_stream_t stream);

#ifdef __cplusplus
}

/* ---- the digit routine: __host__ __device__, integer arithmetic only ---------------------------------------------------- */
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CDML_HD __host__ __device__
#else
#define CDML_HD
#endif

struct cdml_f32_dec {
  uint32_t digits; /* the p significant digits as an integer, no trailing zero */
  int p;           /* 1 .. 9 */
  int k;           /* decimal exponent of the first digit: the value reads d.ddd x 10^k */
  int sci;         /* 1: scientific layout (x < 1e-4) */
};

CDML_HD inline bool cdml_f32_shortest_in_range(float x) { return x >= CDML_F32_SHORTEST_MIN && x < CDML_F32_SHORTEST_MAX; }

CDML_HD inline uint32_t cdml_pow10_u32(int e) { /* 10^e, 0 <= e <= 9 */
  uint32_t v = 1;
  for (int i = 0; i < e; ++i) v *= 10u;
  return v;
}

/* the shortest digits of an x in range (cdml_f32_shortest_in_range(x) must hold) */
CDML_HD inline cdml_f32_dec cdml_f32_shortest_digits(float x) {
  typedef unsigned __int128 u128;
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  const uint32_t frac = b & 0x7fffffu;
  const uint32_t m = frac | 0x800000u;               /* in range every x is a normal number */
  const int s = 150 - (int)((b >> 23) & 0xffu);      /* x = m 2^-s, 23 <= s <= 87 */
  const bool unequal = frac == 0;                    /* a power of two: the float below is half as far as the one above */
  const u128 one = (u128)1 << s, mask = one - 1;
  u128 N = m, M = 1;
  int j = 0;
  while ((N >> s) == 0 && j < 20) { /* (j < 20 holds in range: 2^-64 10^20 > 1) */
    N *= 10u;
    M *= 10u;
    ++j;
  }
  uint32_t digits = (uint32_t)(N >> s);
  u128 r = N & mask;
  int p = 1;
  bool low, high;
  for (;;) {
    low = (unequal ? 4u * r : 2u * r) < M;
    high = 2u * r + M > 2u * one;
    if (low || high || p == 9) break;
    r *= 10u;
    M *= 10u;
    digits = digits * 10u + (uint32_t)(r >> s);
    r &= mask;
    ++p;
  }
  bool down = low;
  if (low == high) {
    const u128 t = 2u * r;
    down = t < one || (t == one && !(digits & 1u));
  }
  cdml_f32_dec o;
  o.k = -j;
  o.sci = j > 4;
  if (!down) {
    ++digits;
    if (digits == cdml_pow10_u32(p)) { /* 9.99 -> 10.0: one digit, the next decade */
      digits = 1;
      p = 1;
      ++o.k;
    }
  }
  while (p > 1 && digits % 10u == 0) {
    digits /= 10u;
    --p;
  }
  o.digits = digits;
  o.p = p;
  return o;
}

CDML_HD inline int cdml_f32_dec_length(const cdml_f32_dec &d) {
  if (d.sci) return d.p + (d.p > 1 ? 1 : 0) + 4;   /* d[.ddd]e-XX */
  if (d.k >= 0) return 2 + (d.p > 1 ? d.p - 1 : 1); /* d.ddd | d.0 */
  return 1 - d.k + d.p;                             /* 0.<-k-1 zeros>ddd */
}

/* the characters, in order, through put(char); exactly cdml_f32_dec_length(d) calls */
template <typename Put>
CDML_HD inline void cdml_f32_dec_emit(const cdml_f32_dec &d, Put put) {
  uint32_t rest = d.digits, div = cdml_pow10_u32(d.p - 1);
  const bool lead = d.sci || d.k >= 0; /* one digit in front of the point */
  if (!lead) {
    put('0');
    put('.');
    for (int z = 0; z < -d.k - 1; ++z) put('0');
  }
  for (int i = 0; i < d.p; ++i) {
    const uint32_t c = rest / div;
    rest -= c * div;
    div /= 10u;
    put((char)('0' + c));
    if (lead && i == 0 && (d.p > 1 || !d.sci)) put('.');
  }
  if (!d.sci) {
    if (lead && d.p == 1) put('0');
    return;
  }
  const int e = -d.k; /* 4 <= e <= 20 */
  put('e');
  put('-');
  put((char)('0' + e / 10));
  put((char)('0' + e % 10));
}
#endif /* __cplusplus */

#endif /* CDML_KNN_WRITER_H_ */

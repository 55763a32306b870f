// The quantiser of the fp8 catalogue (include/cdml_f8.h) for gfx950: fp32 or fp16 rows -> OCP e4m3 codes + one power-of-two
// scale per row.  Not on the step path: it runs once, when a catalogue is loaded or converted (FeatureTableF8.from_table /
// synthetic quantise it chunk by chunk, so the wider table never has to exist whole).
//
// One wave per row, two passes over the row (the second one finds it in L2): the finite absmax by integer compares of the
// magnitude bits and a wave reduction, the scale from its exponent field (no log2f), then codes = v_cvt_pk_fp8_f32(x / scale)
// -- round to nearest even, exact division -- 8 codes = one 8-byte store per lane.  Lane l of step c holds columns
// 8 (l + 64 c) .. + 7, as the gather's lanes do.  Source pad columns are never trusted; destination columns F .. width - 1
// are written as code 0.
#include "common.h"
#include "gather_plan.h"
#include "../../include/cdml_f8.h"

namespace cdml {
namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / kWave;
constexpr int kF8MaxF = 4096;
using u32x2q = __attribute__((ext_vector_type(2))) uint32_t;
using f32x4q = __attribute__((ext_vector_type(4))) float;

// columns 8 q .. 8 q + 7 of a source row as fp32 (an fp16 source widens exactly)
__device__ __forceinline__ void load8(const float *row, int q, float (&x)[8]) {
  const f32x4q a = reinterpret_cast<const f32x4q *>(row)[2 * q], b = reinterpret_cast<const f32x4q *>(row)[2 * q + 1];
#pragma unroll
  for (int u = 0; u < 4; ++u) x[u] = a[u], x[4 + u] = b[u];
}
__device__ __forceinline__ void load8(const _Float16 *row, int q, float (&x)[8]) {
  const cdml_half8 a = reinterpret_cast<const cdml_half8 *>(row)[q];
#pragma unroll
  for (int u = 0; u < 8; ++u) x[u] = (float)a[u];
}

constexpr uint32_t kMagMask = 0x7FFFFFFFu, kInfBits = 0x7F800000u;

// four codes of y[0..3] = x / scale; xb: the bits of the unscaled values (an Inf / NaN element -> the NaN code of its sign)
__device__ __forceinline__ uint32_t pack4_e4m3(const float *y, const uint32_t *xb) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
  uint32_t o = (uint32_t)w;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((xb[k] & kMagMask) >= kInfBits) o = (o & ~(0xFFu << (8 * k))) | ((0x7Fu | ((xb[k] >> 24) & 0x80u)) << (8 * k));
  return o;
}

template <typename In>
__global__ void __launch_bounds__(kThreads)
k_quantize_rows_f8(const In *__restrict__ src, int64_t n_rows, int64_t src_stride, int F, uint8_t *__restrict__ codes,
                   int64_t code_stride, int width, float *__restrict__ scale) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nq = (F + 7) >> 3, wq = width >> 3;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave; r < n_rows; r += (int64_t)gridDim.x * kWavesPerBlock) {
    const In *row = src + r * src_stride;
    // the largest finite magnitude, as bits (the order of non-negative floats is the order of their bits)
    uint32_t m = 0;
    for (int q = lane; q < nq; q += kWave) {
      float x[8];
      load8(row, q, x);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t b = __float_as_uint(x[u]) & kMagMask;
        if (8 * q + u < F && b < kInfBits) m = max(m, b);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    // scale = 2^k, k = max(floor(log2 m), -119) - 7 in [-126, 120] (a denormal m has exponent field 0: the clamp's case);
    // m == 0 -> 1.  Both 2^k and 2^-k are normal numbers built from their exponent fields
    int k = 0;
    if (m) k = max((int)(m >> 23) - 127, -119) - 7;
    const float sc = __uint_as_float((uint32_t)(k + 127) << 23), inv = __uint_as_float((uint32_t)(127 - k) << 23);
    if (lane == 0) scale[r] = sc;
    uint8_t *dst = codes + r * code_stride;
    for (int q = lane; q < wq; q += kWave) {
      u32x2q o = {0u, 0u};
      if (q < nq) {
        float x[8], y[8];
        uint32_t xb[8];
        load8(row, q, x);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (8 * q + u >= F) x[u] = 0.f;
          xb[u] = __float_as_uint(x[u]);
          y[u] = x[u] * inv;
        }
        o[0] = pack4_e4m3(y, xb), o[1] = pack4_e4m3(y + 4, xb + 4);
      }
      *reinterpret_cast<u32x2q *>(dst + 8 * q) = o;
    }
  }
}

template <typename In>
int quantize_rows_f8(const char *who, const In *src, int64_t n_rows, int64_t src_stride, int F, uint8_t *codes,
                     int64_t code_stride, int64_t width, float *scale, cdml_stream_t stream) {
  CDML_REQUIRE(src && codes && scale && n_rows > 0, CDML_E_BADARG, "%s: bad argument", who);
  CDML_REQUIRE(F > 0 && F <= kF8MaxF, CDML_E_UNSUPPORTED, "%s: F = %d outside (0, %d]", who, F, kF8MaxF);
  CDML_REQUIRE(src_stride >= F && (src_stride & 7) == 0 && aligned16(src), CDML_E_ALIGN,
               "%s: src_stride must be >= F and a multiple of 8, src 16-B aligned", who);
  CDML_REQUIRE(width >= F && (width & 7) == 0 && width <= code_stride && width <= 2 * kF8MaxF && (code_stride & 7) == 0 &&
                   aligned_to(codes, 8) && aligned_to(scale, 4),
               CDML_E_ALIGN, "%s: width must be >= F, a multiple of 8 and <= code_stride (a multiple of 8), codes 8-B aligned", who);
  hipLaunchKernelGGL(k_quantize_rows_f8<In>, dim3(grid_for(n_rows, kWavesPerBlock)), dim3(kThreads), 0, (hipStream_t)stream,
                     src, n_rows, src_stride, F, codes, code_stride, (int)width, scale);
  return check_launch(who);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_quantize_rows_f8_f32(const float *src, int64_t n_rows, int64_t src_stride, int F, uint8_t *codes,
                                         int64_t code_stride, int64_t width, float *scale, cdml_stream_t stream) {
  return quantize_rows_f8("quantize_rows_f8_f32", src, n_rows, src_stride, F, codes, code_stride, width, scale, stream);
}

extern "C" int cdml_quantize_rows_f8_f16(const uint16_t *src, int64_t n_rows, int64_t src_stride, int F, uint8_t *codes,
                                         int64_t code_stride, int64_t width, float *scale, cdml_stream_t stream) {
  return quantize_rows_f8("quantize_rows_f8_f16", reinterpret_cast<const _Float16 *>(src), n_rows, src_stride, F, codes,
                          code_stride, width, scale, stream);
}

/* cdml_f8.h -- C ABI of the fp8 catalogue of the config-4 precision ("bf16"): OCP e4m3 codes in HBM, one byte per feature,
 * gathered into l2-normalised bf16 rows by the kernels of csrc/sampler_gather.hip (row policy RowF8) and written by the
 * quantiser of csrc/f8.hip.  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on `stream`,
 * status ints, cdml_last_error()).
 *
 * The format (cdml_amd/engine_bf16.FeatureTableF8 holds it; host model: tests/f8_ref.py).
 *   codes   OCP e4m3fn (torch.float8_e4m3fn: 1 sign, 4 exponent, 3 mantissa bits, bias 7, no infinity, NaN = 0x7F / 0xFF)
 *           [n_rows][row_stride] bytes, row_stride = round_up(F, 128) so that every row starts on a 128-B line; the pad
 *           columns hold code 0.
 *   scale   fp32 [n_rows], one power of two per row: value = code x scale.
 *
 * The quantiser rule -- integer / exponent arithmetic only, the same on the host and on the device.  m = the largest
 * finite |x| of the row (taken in fp32; an fp16 source is widened exactly):
 *   m > 0:   scale = 2^(max(floor(log2 m), -119) - 7)       (floor(log2 m) read from the exponent field; the clamp keeps the
 *                                                            scale a normal fp32 number, >= 2^-126, for rows below 2^-119)
 *   m == 0:  scale = 1
 *   code = RNE_e4m3(x / scale)                              (the division by a power of two is exact)
 * so |x / scale| < 256 and |code| <= 256 < 448: nothing saturates, and the largest code of a row with m >= 2^-119 is >= 128.
 * An Inf or NaN element becomes the NaN code of its sign (0x7F / 0xFF); the rest of its row is quantised as usual.
 *
 * What the training path computes from a row: x_hat = codes / max(|codes|_2, 1e-6) -- the 1e-12 clamp of the reference's
 * l2_normalize (models.py:58) applied to the CODES; the scale of a row cancels and is never read by the gather.  A zero row
 * stays zero.  A non-zero row has |codes|_2 >= 2^-9, far above the clamp, so a row whose TRUE norm is below 1e-6 is
 * normalised to unit length here, where the fp32 and fp16 catalogues damp such a row (x / 1e-6) instead.
 *
 * Error of the format.  Per element |code x scale - x| <= 2^-4 |x| (half an ulp of 3 mantissa bits), or <= 2^-10 x scale in
 * the code's subnormal range (|x / scale| < 2^-6), so per row |dequantised - x|_2 <= 2^-4 |x|_2 + sqrt(F) 2^-10 scale.
 *
 * Every e4m3 value is exactly an fp16 value.  The gather converts the eight codes a lane holds exactly to fp16 and then runs
 * the instructions of the fp16 gather (same lane -> column mapping: lane l of chunk c holds columns 8 (l + 64 c) .. + 7, an
 * 8-byte load; same sum-of-squares order), so its output is BIT FOR BIT that of cdml_gather_rows_f16 / cdml_sample_gather_f16
 * on the fp16 table holding the same values.  A NaN code comes out as NaN at its column (as there: fmaxf(ss, 1e-12f) drops the
 * NaN sum of squares, so the row's other columns are its codes x 1e6 -- the step's loss is NaN either way).
 *
 * cdml_sample_gather_f8 / _listed_f8 / _weighted_f8 / cdml_gather_rows_f8: the arguments, modes, ids, kind_out, oob_flag and
 *   per-step strides of their _f16 twins (cdml.h, cdml_hardneg.h, cdml_negweights.h); the table is the codes.  Layout rules
 *   of this format: F in (0, 4096]; row_stride (bytes = elements) >= F and a multiple of 16, table base 16-B aligned;
 *   out_stride (bf16 elements) >= F and a multiple of 8, x_out base 16-B aligned.
 * cdml_quantize_rows_f8_f32 / _f16: codes[r][0 .. width) and scale[r] of the rows src[r][0 .. F), r < n_rows; columns F ..
 *   width - 1 are written as code 0 and nothing else of a destination row is touched, so `codes` may be a slice (rows
 *   code_stride bytes apart) of a larger table, and the source stride is independent of it.  src_stride (elements) >= F and
 *   a multiple of 8, src base 16-B aligned; width >= F, a multiple of 8, <= code_stride; code_stride a multiple of 8, codes
 *   base 8-B aligned; F in (0, 4096].
 * Bad arguments return before any HIP call. */
#ifndef CDML_F8_H_
#define CDML_F8_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_sample_gather_f8(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                          const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global, const uint8_t *table,
                          int64_t n_rows, int64_t row_stride, int F, int32_t *idx_out, int32_t *shift_out,
                          uint16_t *x_out_bf16, int64_t out_stride, int n_steps, int64_t x_step_stride,
                          int64_t idx_step_stride, int32_t *oob_flag, cdml_stream_t stream);
int cdml_sample_gather_listed_f8(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                 const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                 const uint8_t *table, int64_t n_rows, int64_t row_stride, int F, const int32_t *lists,
                                 int64_t ldl, int L, uint64_t hard_thresh, int32_t *idx_out, int32_t *kind_out,
                                 uint16_t *x_out_bf16, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                 int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream);
int cdml_sample_gather_weighted_f8(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                   const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                   const uint8_t *table, int64_t n_rows, int64_t row_stride, int F, const int32_t *start,
                                   int64_t n_live, const int32_t *coarse, int bits, int32_t *idx_out, int32_t *kind_out,
                                   uint16_t *x_out_bf16, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                   int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream);
int cdml_gather_rows_f8(const uint8_t *table, int64_t row0, int64_t n_rows, int64_t row_stride, const int32_t *idx, int n_idx,
                        int F, uint16_t *x_out_bf16, int64_t out_stride, int32_t *oob_flag, cdml_stream_t stream);

int cdml_quantize_rows_f8_f32(const float *src, int64_t n_rows, int64_t src_stride, int F, uint8_t *codes,
                              int64_t code_stride, int64_t width, float *scale, cdml_stream_t stream);
int cdml_quantize_rows_f8_f16(const uint16_t *src, int64_t n_rows, int64_t src_stride, int F, uint8_t *codes,
                              int64_t code_stride, int64_t width, float *scale, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_F8_H_ */

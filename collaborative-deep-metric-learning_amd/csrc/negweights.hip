// The per-negative logQ bias of the weighted negatives (include/cdml_negweights.h): neg_bias[j] = lq[n_j] + offset for the
// negatives n_j = ids3[3 j + 2] the sampler drew (mode 3 of csrc/sampler_gather.hip), the vector the mixed N-pair chain's
// _nb launches subtract from the uniform block's logits.  B loads of 4 bytes: latency, not bandwidth -- one thread each.
#include "common.h"
#include "../../include/cdml_negweights.h"
#include <math.h>

namespace cdml {
namespace {

constexpr int kNwThreads = 256;

__global__ void __launch_bounds__(kNwThreads)
k_negw_bias(const float *__restrict__ lq, int64_t n_rows, const int32_t *__restrict__ ids3, int B, float offset,
            float *__restrict__ neg_bias) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= B) return;
  const int32_t n = ids3[3 * (int64_t)j + 2];
  neg_bias[j] = (n >= 0 && (int64_t)n < n_rows) ? lq[n] + offset : 0.f;     // an id outside the catalogue: no correction
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_negw_bias(const float *lq, int64_t n_rows, const int32_t *ids3, int B, float offset, float *neg_bias,
                              cdml_stream_t stream) {
  CDML_REQUIRE(lq && ids3 && neg_bias, CDML_E_BADARG, "negw_bias: null pointer");
  CDML_REQUIRE(n_rows >= 1 && B >= 1, CDML_E_BADARG, "negw_bias: n_rows and B must be positive (got %lld, %d)", (long long)n_rows, B);
  CDML_REQUIRE(isfinite(offset), CDML_E_BADARG, "negw_bias: offset must be finite (got %g)", (double)offset);
  hipLaunchKernelGGL(k_negw_bias, dim3((B + kNwThreads - 1) / kNwThreads), dim3(kNwThreads), 0, (hipStream_t)stream, lq, n_rows,
                     ids3, B, offset, neg_bias);
  return check_launch("negw_bias");
}

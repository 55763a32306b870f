// The sampling-bias correction of the N-pair loss (logQ; Yi et al., RecSys 2019) -- build-defined, the reference has no such
// loss.  lq(v) = log of the probability that video v is drawn into a batch; the corrected passes of csrc/npair.hip take it per
// slot: bias[2i] = lq(id(a_i)), bias[2i + 1] = lq(id(p_i)), mem_bias[k] = lq(mem_id[k]).
//
// Two sources of lq:
//   a fixed table     lq(v) = table[v], a per-video log-probability the caller supplies
//   the estimator     Yi et al.'s streaming frequency estimate, indexed by video id (no hash): last[v] (int32, -1 = unseen)
//                     is the step v was last drawn as a positive, gap[v] (fp32, initially g0 >= 1) the smoothed steps
//                     between two draws; lq(v) = -log(gap[v]).  At step t every positive video v of the batch takes
//                     gap[v] <- (1 - a) gap[v] + a (t - last[v]) when last[v] >= 0 (each product and sum rounded on its own:
//                     __fmul_rn / __fadd_rn, so a float32 host model matches bit for bit), and last[v] <- t.
//
// Three launches, enqueue-only, no atomics:
//   k_logq_gather<STREAM>  one lane per slot of [ids | mem_id]: bias / mem_bias (0 for an empty slot or an id outside
//                          [0, n_videos)); STREAM also snapshots (last, gap) of the B positives before the step changes them
//   k_logq_update          one lane per positive: the new (last, gap) from the snapshot.  Positives of the same video compute
//                          the same values from the same snapshot, so the order of their stores does not matter
//   k_logq_reset           last = -1, gap = g0
#include "common.h"
#include <math.h>

namespace cdml {
namespace {

constexpr int kLqThreads = 256;

__device__ __forceinline__ bool lq_in(int v, int64_t n) { return v >= 0 && (int64_t)v < n; }

// slot e < 2B: ids[e]; 2B <= e < 2B + M: mem_id[e - 2B]
template <bool STREAM>
__global__ void __launch_bounds__(kLqThreads)
k_logq_gather(const float *__restrict__ table, const int32_t *__restrict__ last, const float *__restrict__ gap, int64_t n,
              const int32_t *__restrict__ ids, int B, const int32_t *__restrict__ mem_id, int M, float *__restrict__ bias,
              float *__restrict__ mem_bias, int32_t *__restrict__ snap_last, float *__restrict__ snap_gap) {
  const int64_t e = (int64_t)blockIdx.x * kLqThreads + threadIdx.x;
  const int64_t nb = 2 * (int64_t)B;
  if (e >= nb + M) return;
  const int v = e < nb ? ids[e] : mem_id[e - nb];
  const bool in = lq_in(v, n);
  float lq = 0.f;
  if (in) lq = STREAM ? -logf(gap[v]) : table[v];
  if (e < nb)
    bias[e] = lq;
  else
    mem_bias[e - nb] = lq;
  if constexpr (STREAM) {
    if (e < nb && (e & 1)) {
      snap_last[e >> 1] = in ? last[v] : -1;
      snap_gap[e >> 1] = in ? gap[v] : 1.f;
    }
  }
}

__global__ void __launch_bounds__(kLqThreads)
k_logq_update(int32_t *__restrict__ last, float *__restrict__ gap, int64_t n, const int32_t *__restrict__ ids, int B,
              const int32_t *__restrict__ snap_last, const float *__restrict__ snap_gap, float alpha, uint64_t step_imm,
              const uint64_t *__restrict__ step_dev) {
  const int r = blockIdx.x * kLqThreads + threadIdx.x;
  if (r >= B) return;
  const int v = ids[2 * r + 1];
  if (!lq_in(v, n)) return;
  const int64_t t = (int64_t)(step_imm + (step_dev ? *step_dev : 0));
  const int l = snap_last[r];
  float g = snap_gap[r];
  if (l >= 0) g = __fadd_rn(__fmul_rn(__fadd_rn(1.f, -alpha), g), __fmul_rn(alpha, (float)(t - (int64_t)l)));
  gap[v] = g;
  last[v] = (int32_t)t;
}

__global__ void __launch_bounds__(kLqThreads)
k_logq_reset(int32_t *__restrict__ last, float *__restrict__ gap, int64_t n, float g0) {
  const int64_t v = (int64_t)blockIdx.x * kLqThreads + threadIdx.x;
  if (v >= n) return;
  last[v] = -1;
  gap[v] = g0;
}

unsigned lq_blocks(int64_t n) { return (unsigned)((n + kLqThreads - 1) / kLqThreads); }

int lq_check(const char *who, int64_t n, const int32_t *ids, int B, const int32_t *mem_id, int M, const float *bias,
             const float *mem_bias) {
  CDML_REQUIRE(ids && bias, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(n >= 1 && n <= 2147483647LL, CDML_E_BADARG, "%s: n_videos must be in [1, 2^31 - 1], got %lld", who,
               (long long)n);
  CDML_REQUIRE(B >= 1 && M >= 0, CDML_E_BADARG, "%s: needs B >= 1 and M >= 0 (got B %d, M %d)", who, B, M);
  CDML_REQUIRE(!M || (mem_id && mem_bias), CDML_E_BADARG, "%s: null pointer (M > 0 needs mem_id and mem_bias)", who);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_logq_table_gather(const float *table, int64_t n_videos, const int32_t *ids, int B, const int32_t *mem_id,
                                      int M, float *bias, float *mem_bias, cdml_stream_t stream) {
  if (int rc = lq_check("logq_table_gather", n_videos, ids, B, mem_id, M, bias, mem_bias)) return rc;
  CDML_REQUIRE(table, CDML_E_BADARG, "logq_table_gather: null pointer (table)");
  hipLaunchKernelGGL(k_logq_gather<false>, dim3(lq_blocks(2 * (int64_t)B + M)), dim3(kLqThreads), 0, (hipStream_t)stream,
                     table, (const int32_t *)nullptr, (const float *)nullptr, n_videos, ids, B, mem_id, M, bias, mem_bias,
                     (int32_t *)nullptr, (float *)nullptr);
  return check_launch("logq_table_gather");
}

extern "C" int cdml_logq_stream_gather(const int32_t *last, const float *gap, int64_t n_videos, const int32_t *ids, int B,
                                       const int32_t *mem_id, int M, float *bias, float *mem_bias, int32_t *snap_last,
                                       float *snap_gap, cdml_stream_t stream) {
  if (int rc = lq_check("logq_stream_gather", n_videos, ids, B, mem_id, M, bias, mem_bias)) return rc;
  CDML_REQUIRE(last && gap && snap_last && snap_gap, CDML_E_BADARG, "logq_stream_gather: null pointer (estimator state)");
  hipLaunchKernelGGL(k_logq_gather<true>, dim3(lq_blocks(2 * (int64_t)B + M)), dim3(kLqThreads), 0, (hipStream_t)stream,
                     (const float *)nullptr, last, gap, n_videos, ids, B, mem_id, M, bias, mem_bias, snap_last, snap_gap);
  return check_launch("logq_stream_gather");
}

extern "C" int cdml_logq_stream_update(int32_t *last, float *gap, int64_t n_videos, const int32_t *ids, int B,
                                       const int32_t *snap_last, const float *snap_gap, float alpha, uint64_t step,
                                       const uint64_t *step_dev, cdml_stream_t stream) {
  CDML_REQUIRE(last && gap && ids && snap_last && snap_gap, CDML_E_BADARG, "logq_stream_update: null pointer");
  CDML_REQUIRE(n_videos >= 1 && n_videos <= 2147483647LL, CDML_E_BADARG,
               "logq_stream_update: n_videos must be in [1, 2^31 - 1], got %lld", (long long)n_videos);
  CDML_REQUIRE(B >= 1, CDML_E_BADARG, "logq_stream_update: B must be >= 1, got %d", B);
  CDML_REQUIRE(alpha > 0.f && alpha <= 1.f, CDML_E_BADARG, "logq_stream_update: alpha must be in (0, 1], got %g",
               (double)alpha);
  hipLaunchKernelGGL(k_logq_update, dim3(lq_blocks(B)), dim3(kLqThreads), 0, (hipStream_t)stream, last, gap, n_videos, ids, B,
                     snap_last, snap_gap, alpha, step, step_dev);
  return check_launch("logq_stream_update");
}

extern "C" int cdml_logq_stream_reset(int32_t *last, float *gap, int64_t n_videos, float g0, cdml_stream_t stream) {
  CDML_REQUIRE(last && gap, CDML_E_BADARG, "logq_stream_reset: null pointer");
  CDML_REQUIRE(n_videos >= 1 && n_videos <= 2147483647LL, CDML_E_BADARG,
               "logq_stream_reset: n_videos must be in [1, 2^31 - 1], got %lld", (long long)n_videos);
  CDML_REQUIRE(isfinite(g0) && g0 >= 1.f, CDML_E_BADARG, "logq_stream_reset: the initial gap g0 must be finite and >= 1, got %g",
               (double)g0);
  hipLaunchKernelGGL(k_logq_reset, dim3(lq_blocks(n_videos)), dim3(kLqThreads), 0, (hipStream_t)stream, last, gap, n_videos,
                     g0);
  return check_launch("logq_stream_reset");
}

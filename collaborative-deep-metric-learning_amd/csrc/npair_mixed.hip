// The N-pair loss with mixed negative sampling (Yang et al., WWW 2020 companion; build-defined -- the reference's only
// negative rule is the uniform draw itself, parse_data.py:292-298): the softmax of every anchor runs over the in-batch
// positives AND the batch's uniformly drawn catalogue negatives (and the cross-batch memory), and the uniform negatives
// receive a gradient.  include/cdml_npair_mixed.h states the definition; csrc/npair.hip the in-batch / memory rules.
//
// The chain reads the uniform sampler's own layout -- ids[3i], [3i+1], [3i+2] = a_i, p_i, n_i and the embedded rows
// e[3i], e[3i+1], e[3i+2] -- so nothing is repacked: a lane takes FOUR triplets' twelve ids as three 16-B loads.
//   k_mixed_split     the three bf16 planes of A, P, N from e's stride-3 rows into the operand images of the plane
//                     GEMMs: A3, the row image [P; N; ..] and (through a 64 x 64 LDS tile) the transposed image
//   k_mixed_rows      one block per anchor: one pass over S[i][:] -- the in-batch and the uniform block four columns per
//                     lane from the same id loads, then the memory block -- with an online (max, sum-exp) per lane,
//                     combined by a fixed butterfly and then wave by wave (row_fold of csrc/npair_common.h)
//   k_npair_cols<BIAS, 3> / k_npair_col_fold   (npair_common.h; symmetric) the column term over the in-batch block: the
//                     in-batch chain's column pass reading the ids three apart
//   k_mixed_stats     one block: the step scalars from the per-row partials in a fixed order (step_scalars)
//   k_mixed_w<FMT>    W of all blocks in ONE launch, four columns per lane, as three bf16 planes or fp32 (store_w4)
// BIAS (template switch): the logQ correction -- in-batch logits less bias[2j + 1] (the [2B] layout of the logQ gather),
// the uniform block's less the scalar lq_u, a slot's less mem_bias[k].  NB (a further template switch, include/
// cdml_negweights.h): the uniform block's correction is one value per column, neg_bias[j], read as one float4 beside u4 --
// the argument slot of lq_u then holds the vector's pointer (LqArg), so the scalar instantiations are what they were.
// No atomics; every sum in a fixed order.
#include "npair_common.h"
#include "../../include/cdml_npair_mixed.h"
#include "../../include/cdml_negweights.h"
#include <math.h>
#include <type_traits>

namespace cdml {
namespace {

constexpr int kMxThreads = 256;
constexpr int kMxTile = 64;            // the split's tile

// the ids of triplets j0 .. j0 + 3 (j0 a multiple of 4): twelve consecutive int32, three 16-B loads
__device__ __forceinline__ void mx_ids4(const int32_t *ids, int j0, int (&a)[4], int (&p)[4], int (&n)[4]) {
  const int4 *src = reinterpret_cast<const int4 *>(ids + 3 * (int64_t)j0);
  const int4 x = src[0], y = src[1], z = src[2];
  a[0] = x.x; p[0] = x.y; n[0] = x.z;
  a[1] = x.w; p[1] = y.x; n[1] = y.y;
  a[2] = y.z; p[2] = y.w; n[2] = z.x;
  a[3] = z.y; p[3] = z.z; n[3] = z.w;
}

__device__ __forceinline__ bool mx_other(int q, int ida, int idp) { return q != ida && q != idp; }

// the uniform block's correction as a kernel argument: the scalar lq_u, or (NB) the per-column vector neg_bias
template <bool NB>
using LqArg = typename std::conditional<NB, const float *, float>::type;

// part[4 i .. 4 i + 3] = {lse_i - (S_ii / t - lq(p_i)), 2 - 2 S_ii, sum over the counted negatives of 2 - 2 S, their count}
template <bool MEM, bool BIAS, bool NB = false>
__global__ void __launch_bounds__(kMxThreads)
k_mixed_rows(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t,
             float *__restrict__ lse, float *__restrict__ part, int64_t neg_col, int64_t mem_col,
             const int32_t *__restrict__ mem_id, int n_mem, const float *__restrict__ bias, LqArg<NB> lq_u,
             const float *__restrict__ mem_bias) {
  const int i = blockIdx.x;
  const float *row = S + (int64_t)i * lds;
  const int ida = ids ? ids[3 * (int64_t)i] : 0, idp = ids ? ids[3 * (int64_t)i + 1] : 0;
  float m = -INFINITY, s = 0.f, nsum = 0.f, ncnt = 0.f;
  for (int j0 = 4 * threadIdx.x; j0 < B; j0 += 4 * kMxThreads) {
    const float4 v4 = *reinterpret_cast<const float4 *>(row + j0);
    const float4 u4 = *reinterpret_cast<const float4 *>(row + neg_col + j0);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w}, u[4] = {u4.x, u4.y, u4.z, u4.w};
    int a[4] = {0, 0, 0, 0}, p[4] = {0, 0, 0, 0}, n[4] = {0, 0, 0, 0};
    if (ids) mx_ids4(ids, j0, a, p, n);
    float bp[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS) {                                // slots 2 j0 .. 2 j0 + 7 of the [2B] layout: the positives' are odd
      const float4 b0 = *reinterpret_cast<const float4 *>(bias + 2 * (int64_t)j0);
      const float4 b1 = *reinterpret_cast<const float4 *>(bias + 2 * (int64_t)j0 + 4);
      bp[0] = b0.y; bp[1] = b0.w; bp[2] = b1.y; bp[3] = b1.w;
    }
    float nb[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS && NB) {                          // the uniform block's per-column correction
      const float4 n4 = *reinterpret_cast<const float4 *>(lq_u + j0);
      nb[0] = n4.x; nb[1] = n4.y; nb[2] = n4.z; nb[3] = n4.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {                        // the in-batch block
      const int j = j0 + q;
      if (j != i && ids && !mx_other(p[q], ida, idp)) continue;
      if constexpr (BIAS)
        lse_add(m, s, v[q] * inv_t - bp[q]);
      else
        lse_add(m, s, v[q] * inv_t);
      if (j != i) {
        nsum += 2.f - 2.f * v[q];
        ncnt += 1.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {                        // the uniform block: no special diagonal
      if (ids && !mx_other(n[q], ida, idp)) continue;
      if constexpr (BIAS && NB)
        lse_add(m, s, u[q] * inv_t - nb[q]);
      else if constexpr (BIAS)
        lse_add(m, s, u[q] * inv_t - lq_u);
      else
        lse_add(m, s, u[q] * inv_t);
      nsum += 2.f - 2.f * u[q];
      ncnt += 1.f;
    }
  }
  if constexpr (MEM) {
    const float *mrow = row + mem_col;
    for (int k = 4 * threadIdx.x; k < n_mem; k += 4 * kMxThreads) {
      const float4 v4 = *reinterpret_cast<const float4 *>(mrow + k);
      const int4 q4 = *reinterpret_cast<const int4 *>(mem_id + k);
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
      const int q[4] = {q4.x, q4.y, q4.z, q4.w};
      float b[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (BIAS) {
        const float4 b4 = *reinterpret_cast<const float4 *>(mem_bias + k);
        b[0] = b4.x; b[1] = b4.y; b[2] = b4.z; b[3] = b4.w;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (q[c] < 0 || (ids && !mx_other(q[c], ida, idp))) continue;
        if constexpr (BIAS)
          lse_add(m, s, v[c] * inv_t - b[c]);
        else
          lse_add(m, s, v[c] * inv_t);
        nsum += 2.f - 2.f * v[c];
        ncnt += 1.f;
      }
    }
  }
  float M, Sx, ns, nc;
  if (!row_fold<kMxThreads>(m, s, nsum, ncnt, M, Sx, ns, nc)) return;
  const float sii = row[i];
  float d;
  if constexpr (BIAS)
    d = sii * inv_t - bias[2 * (int64_t)i + 1];
  else
    d = sii * inv_t;
  row_store(M, Sx, ns, nc, sii, d, i, lse, part);
}

// stats[0] = loss, [1] = mean |a_i - p_i|^2, [2] = mean squared distance over the counted negatives of the three blocks,
// [3] = their fraction of B (B - 1) + B B + B M
__global__ void __launch_bounds__(1024)
k_mixed_stats(const float *__restrict__ part, const float *__restrict__ closs, int B, int symmetric, int M,
              float *__restrict__ stats) {
  const float fb = (float)B;
  step_scalars<false>(part, B, symmetric, [&](int i) { return closs[i]; }, fb * (float)(B - 1) + fb * fb + fb * (float)M, stats);
}

// Row i = blockIdx.x, columns c0 = 4 (blockIdx.y * kMxThreads + threadIdx.x) .. c0 + 3 of the span [0, mem_col + M) (without
// a memory: [0, neg_col + B)).  Every block starts and ends on a multiple of 4, so the four columns lie in one block or in a
// gap between two, which is not written.  scale = 1 / (B t); the uniform and the memory block halve it with `symmetric`.
template <int FMT, bool MEM, bool BIAS, bool NB = false>
__global__ void __launch_bounds__(kMxThreads)
k_mixed_w(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, int64_t neg_col, int64_t mem_col,
          const int32_t *__restrict__ mem_id, int M, float inv_t, int symmetric, const float *__restrict__ lse, float scale,
          void *__restrict__ Wout, int64_t ldw, int64_t plane, const float *__restrict__ bias, LqArg<NB> lq_u,
          const float *__restrict__ mem_bias) {
  const int i = blockIdx.x;
  const int64_t c0 = ((int64_t)blockIdx.y * kMxThreads + threadIdx.x) * 4;
  const int64_t span = MEM ? mem_col + M : neg_col + B;
  if (c0 >= span) return;
  const int ida = ids ? ids[3 * (int64_t)i] : 0, idp = ids ? ids[3 * (int64_t)i + 1] : 0;
  const float lr = lse[i];
  const float4 v4 = *reinterpret_cast<const float4 *>(S + (int64_t)i * lds + c0);
  const float v[4] = {v4.x, v4.y, v4.z, v4.w};
  const float side = symmetric ? 0.5f * scale : scale;
  float w[4];
  if (c0 < B) {                                          // the in-batch block (k_npair_w's arithmetic)
    const int j0 = (int)c0;
    int a[4] = {0, 0, 0, 0}, p[4] = {0, 0, 0, 0}, n[4];
    if (ids) mx_ids4(ids, j0, a, p, n);
    float bp[4] = {0.f, 0.f, 0.f, 0.f}, ba = 0.f;
    if constexpr (BIAS) {
      const float4 b0 = *reinterpret_cast<const float4 *>(bias + 2 * (int64_t)j0);
      const float4 b1 = *reinterpret_cast<const float4 *>(bias + 2 * (int64_t)j0 + 4);
      bp[0] = b0.y; bp[1] = b0.w; bp[2] = b1.y; bp[3] = b1.w;
      ba = bias[2 * (int64_t)i];
    }
    float lc[4] = {0.f, 0.f, 0.f, 0.f};
    if (symmetric) {
      const float4 l4 = *reinterpret_cast<const float4 *>(lse + B + j0);
      lc[0] = l4.x; lc[1] = l4.y; lc[2] = l4.z; lc[3] = l4.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + q;
      const bool rc = j == i || !ids || mx_other(p[q], ida, idp);
      float r;
      if constexpr (BIAS)
        r = rc ? expf(v[q] * inv_t - bp[q] - lr) : 0.f;
      else
        r = rc ? expf(v[q] * inv_t - lr) : 0.f;
      if (j == i) r -= 1.f;
      if (symmetric) {
        const bool cc = j == i || !ids || mx_other(ida, a[q], p[q]);
        float c;
        if constexpr (BIAS)
          c = cc ? expf(v[q] * inv_t - ba - lc[q]) : 0.f;
        else
          c = cc ? expf(v[q] * inv_t - lc[q]) : 0.f;
        if (j == i) c -= 1.f;
        r = 0.5f * (r + c);
      }
      w[q] = r * scale;
    }
  } else if (c0 >= neg_col && c0 < neg_col + B) {        // the uniform block
    const int j0 = (int)(c0 - neg_col);
    int a[4], p[4], n[4] = {0, 0, 0, 0};
    if (ids) mx_ids4(ids, j0, a, p, n);
    float nb[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS && NB) {
      const float4 n4 = *reinterpret_cast<const float4 *>(lq_u + j0);
      nb[0] = n4.x; nb[1] = n4.y; nb[2] = n4.z; nb[3] = n4.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool cn = !ids || mx_other(n[q], ida, idp);
      if constexpr (BIAS && NB)
        w[q] = cn ? expf(v[q] * inv_t - nb[q] - lr) * side : 0.f;
      else if constexpr (BIAS)
        w[q] = cn ? expf(v[q] * inv_t - lq_u - lr) * side : 0.f;
      else
        w[q] = cn ? expf(v[q] * inv_t - lr) * side : 0.f;
    }
  } else if (MEM && c0 >= mem_col) {                     // the memory block (k_npair_mem_w's arithmetic)
    const int64_t k0 = c0 - mem_col;
    const int4 q4 = *reinterpret_cast<const int4 *>(mem_id + k0);
    const int qk[4] = {q4.x, q4.y, q4.z, q4.w};
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS) {
      const float4 b4 = *reinterpret_cast<const float4 *>(mem_bias + k0);
      b[0] = b4.x; b[1] = b4.y; b[2] = b4.z; b[3] = b4.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool cm = qk[q] >= 0 && (!ids || mx_other(qk[q], ida, idp));
      if constexpr (BIAS)
        w[q] = cm ? expf(v[q] * inv_t - b[q] - lr) * side : 0.f;
      else
        w[q] = cm ? expf(v[q] * inv_t - lr) * side : 0.f;
    }
  } else {
    return;                                              // a gap between two blocks
  }
  store_w4<FMT>(Wout, i, ldw, plane, c0, w, 4);
}

// blockIdx.z = the role of the rows this block splits: 0 anchors (e[3r] -> A3[r]), 1 positives (e[3r + 1] -> R3[r] and
// T3[.][r]), 2 uniform negatives (e[3r + 2] -> R3[neg_row + r] and T3[.][neg_row + r]).  A 64 x 64 tile per block: a lane
// loads 16 B of a row and stores 8 B per plane; the transposed image goes through LDS so that its stores run along r too.
__global__ void __launch_bounds__(kMxThreads)
k_mixed_split(const float *__restrict__ e, int64_t lde, int B, int D, __bf16 *__restrict__ A3, int64_t lda, int64_t plane_a,
              __bf16 *__restrict__ R3, int64_t ldr, int64_t plane_r, __bf16 *__restrict__ T3, int64_t ldt, int64_t plane_t,
              int64_t neg_row) {
  __shared__ float tile[kMxTile][kMxTile + 1];
  const int role = blockIdx.z;
  const int c0 = blockIdx.x * kMxTile, r0 = blockIdx.y * kMxTile;
  const int64_t base = role == 2 ? neg_row : 0;
  const int g = threadIdx.x & 15, sub = threadIdx.x >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = sub + 16 * k;
    const int gr = r0 + r, gc = c0 + 4 * g;
    if (gr >= B || gc >= D) continue;
    const float4 v4 = *reinterpret_cast<const float4 *>(e + (3 * (int64_t)gr + role) * lde + gc);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    bf4 h, m, l;
    split4(v, h, m, l);
    __bf16 *dst = role == 0 ? A3 + (int64_t)gr * lda + gc : R3 + (base + gr) * ldr + gc;
    const int64_t pl = role == 0 ? plane_a : plane_r;
    *reinterpret_cast<bf4 *>(dst) = h;
    *reinterpret_cast<bf4 *>(dst + pl) = m;
    *reinterpret_cast<bf4 *>(dst + 2 * pl) = l;
    if (role != 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) tile[r][4 * g + q] = v[q];
    }
  }
  if (role == 0) return;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = sub + 16 * k;
    const int gc = c0 + c, gr = r0 + 4 * g;
    if (gc >= D || gr >= B) continue;
    const float v[4] = {tile[4 * g][c], tile[4 * g + 1][c], tile[4 * g + 2][c], tile[4 * g + 3][c]};
    bf4 h, m, l;
    split4(v, h, m, l);
    __bf16 *dst = T3 + (int64_t)gc * ldt + base + gr;
    *reinterpret_cast<bf4 *>(dst) = h;
    *reinterpret_cast<bf4 *>(dst + plane_t) = m;
    *reinterpret_cast<bf4 *>(dst + 2 * plane_t) = l;
  }
}

// the arguments the statistics and the W launches share
int mx_check(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
             const int32_t *mem_id, int M, const float *bias, float lq_u, const float *mem_bias, float temperature,
             const float *lse) {
  CDML_REQUIRE(S && lse, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(B >= 4 && mult4(B), CDML_E_BADARG, "%s: B must be a positive multiple of 4, got %d", who, B);
  CDML_REQUIRE(M >= 0 && mult4(M), CDML_E_BADARG, "%s: the memory size M must be 0 or a positive multiple of 4, got %d", who, M);
  CDML_REQUIRE(!M || mem_id, CDML_E_BADARG, "%s: null pointer (M > 0 needs mem_id)", who);
  if (int rc = np_temperature_check(who, temperature)) return rc;
  CDML_REQUIRE(neg_col >= B && mult4(neg_col), CDML_E_BADARG, "%s: neg_col must be >= B (%d) and a multiple of 4, got %lld", who,
               B, (long long)neg_col);
  CDML_REQUIRE(!M || (mem_col >= neg_col + B && mult4(mem_col)), CDML_E_BADARG,
               "%s: mem_col must be >= neg_col + B (%lld) and a multiple of 4, got %lld", who, (long long)(neg_col + B),
               (long long)mem_col);
  const int64_t span = M ? mem_col + M : neg_col + B;
  CDML_REQUIRE(lds >= span && mult4(lds) && aligned16(S) && aligned16(lse) && aligned16(ids) && aligned16(mem_id), CDML_E_BADARG,
               "%s: S, lse, ids and mem_id need 16-B aligned bases and lds >= %lld, a multiple of 4 (got %lld)", who,
               (long long)span, (long long)lds);
  if (bias) {
    CDML_REQUIRE(aligned16(bias) && isfinite(lq_u), CDML_E_BADARG, "%s: bias needs a 16-B aligned base and lq_u must be finite (got %g)",
                 who, (double)lq_u);
    CDML_REQUIRE(!M || (mem_bias && aligned16(mem_bias)), CDML_E_BADARG,
                 "%s: the corrected loss with a memory needs mem_bias (16-B aligned)", who);
  }
  return CDML_OK;
}

// the vector form's own argument (the scalar launches' check of lq_u, mx_check, is given 0)
int mx_check_nb(const char *who, const float *bias, const float *neg_bias) {
  CDML_REQUIRE(!bias || (neg_bias && aligned16(neg_bias)), CDML_E_BADARG,
               "%s: the corrected loss needs neg_bias (fp32 [B], 16-B aligned)", who);
  return CDML_OK;
}

// LQ: float (the scalar lq_u) or const float * (neg_bias, the NB kernels)
template <bool MEM, bool BIAS, typename LQ>
int mx_stats_launch(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                    const int32_t *mem_id, int M, const float *bias, LQ lq_u, const float *mem_bias, float temperature,
                    int symmetric, float *lse, float *stats, void *workspace, cdml_stream_t stream) {
  const float inv_t = 1.0f / temperature;
  float *part = static_cast<float *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  constexpr bool NB = std::is_pointer<LQ>::value;
  hipLaunchKernelGGL((k_mixed_rows<MEM, BIAS, NB>), dim3(B), dim3(kMxThreads), 0, st, S, lds, ids, B, inv_t, lse, part, neg_col,
                     mem_col, mem_id, M, bias, lq_u, mem_bias);
  if (int rc = check_launch("npair_mixed_stats rows")) return rc;
  if (symmetric)
    if (int rc = np_cols_launch<BIAS, 3>("npair_mixed_stats columns", "npair_mixed_stats column fold", S, lds, ids, B, inv_t,
                                         bias, lse, part, st))
      return rc;
  hipLaunchKernelGGL(k_mixed_stats, dim3(1), dim3(1024), 0, st, part, part + 4 * (size_t)B, B, symmetric ? 1 : 0, M, stats);
  return check_launch("npair_mixed_stats");
}

template <int FMT, typename LQ>
int mx_w_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                const int32_t *mem_id, int M, const float *bias, LQ lq_u, const float *mem_bias, float temperature,
                int symmetric, const float *lse, void *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  constexpr bool NB = std::is_pointer<LQ>::value;
  if constexpr (NB) {
    if (int rc = mx_check(who, S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, 0.f, mem_bias, temperature, lse)) return rc;
    if (int rc = mx_check_nb(who, bias, lq_u)) return rc;
  } else {
    if (int rc = mx_check(who, S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias, temperature, lse)) return rc;
  }
  const int64_t span = M ? mem_col + M : neg_col + B;
  if (int rc = np_w_check(who, FMT, span, W, ldw, plane)) return rc;
  const dim3 grid((unsigned)B, (unsigned)((span + 4 * kMxThreads - 1) / (4 * kMxThreads)));
  const float inv_t = 1.0f / temperature, scale = 1.0f / ((float)B * temperature);
  const int sym = symmetric ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  // (without a correction the block's bias is not read: the uncorrected kernels are the scalar form's, whichever entry asks)
#define CDML_MX_W(MEM, BIAS, NBK, LQ_ARG)                                                                                       \
  hipLaunchKernelGGL((k_mixed_w<FMT, MEM, BIAS, NBK>), grid, dim3(kMxThreads), 0, st, S, lds, ids, B, neg_col, mem_col, mem_id, M, \
                     inv_t, sym, lse, scale, W, ldw, plane, bias, LQ_ARG, mem_bias)
  if (M && bias) {
    CDML_MX_W(true, true, NB, lq_u);
  } else if (M) {
    CDML_MX_W(true, false, false, 0.f);
  } else if (bias) {
    CDML_MX_W(false, true, NB, lq_u);
  } else {
    CDML_MX_W(false, false, false, 0.f);
  }
#undef CDML_MX_W
  return check_launch(who);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" size_t cdml_npair_mixed_workspace(int B, int M) { return M >= 0 ? np_ws_bytes(B) : 0; }

template <typename LQ>
static int mx_stats(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                    const int32_t *mem_id, int M, const float *bias, LQ lq_u, const float *mem_bias, float temperature,
                    int symmetric, float *lse, float *stats, void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  if constexpr (std::is_pointer<LQ>::value) {
    if (int rc = mx_check(who, S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, 0.f, mem_bias, temperature, lse)) return rc;
    if (int rc = mx_check_nb(who, bias, lq_u)) return rc;
  } else {
    if (int rc = mx_check(who, S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias, temperature, lse)) return rc;
  }
  CDML_REQUIRE(stats, CDML_E_BADARG, "%s: null pointer (stats)", who);
  if (int rc = np_ws_check(who, workspace, workspace_bytes, np_ws_bytes(B), "cdml_npair_mixed_workspace(B, M)")) return rc;
  if (M) {
    if (bias)
      return mx_stats_launch<true, true>(S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias, temperature,
                                         symmetric, lse, stats, workspace, stream);
    return mx_stats_launch<true, false>(S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, 0.f, mem_bias, temperature, symmetric,
                                        lse, stats, workspace, stream);       // (uncorrected: the block's bias is not read)
  }
  if (bias)
    return mx_stats_launch<false, true>(S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias, temperature, symmetric,
                                        lse, stats, workspace, stream);
  return mx_stats_launch<false, false>(S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, 0.f, mem_bias, temperature, symmetric,
                                       lse, stats, workspace, stream);
}

extern "C" int cdml_npair_mixed_stats(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                                      const int32_t *mem_id, int M, const float *bias, float lq_u, const float *mem_bias,
                                      float temperature, int symmetric, float *lse, float *stats, void *workspace,
                                      size_t workspace_bytes, cdml_stream_t stream) {
  return mx_stats("npair_mixed_stats", S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias, temperature, symmetric,
                  lse, stats, workspace, workspace_bytes, stream);
}

// ---- the per-negative bias (include/cdml_negweights.h): the same launches on the NB instantiations ----
extern "C" int cdml_npair_mixed_stats_nb(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col,
                                         int64_t mem_col, const int32_t *mem_id, int M, const float *bias, const float *neg_bias,
                                         const float *mem_bias, float temperature, int symmetric, float *lse, float *stats,
                                         void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  return mx_stats("npair_mixed_stats_nb", S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, neg_bias, mem_bias, temperature,
                  symmetric, lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_mixed_grad_x3_nb(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col,
                                           int64_t mem_col, const int32_t *mem_id, int M, const float *bias,
                                           const float *neg_bias, const float *mem_bias, float temperature, int symmetric,
                                           const float *lse, uint16_t *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  return mx_w_launch<kWX3>("npair_mixed_grad_x3_nb", S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, neg_bias, mem_bias,
                           temperature, symmetric, lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_mixed_grad_f32_nb(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col,
                                            int64_t mem_col, const int32_t *mem_id, int M, const float *bias,
                                            const float *neg_bias, const float *mem_bias, float temperature, int symmetric,
                                            const float *lse, float *W, int64_t ldw, cdml_stream_t stream) {
  return mx_w_launch<kWF32>("npair_mixed_grad_f32_nb", S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, neg_bias, mem_bias,
                            temperature, symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_mixed_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col,
                                        int64_t mem_col, const int32_t *mem_id, int M, const float *bias, float lq_u,
                                        const float *mem_bias, float temperature, int symmetric, const float *lse, uint16_t *W,
                                        int64_t ldw, int64_t plane, cdml_stream_t stream) {
  return mx_w_launch<kWX3>("npair_mixed_grad_x3", S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias, temperature,
                           symmetric, lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_mixed_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col,
                                         int64_t mem_col, const int32_t *mem_id, int M, const float *bias, float lq_u,
                                         const float *mem_bias, float temperature, int symmetric, const float *lse, float *W,
                                         int64_t ldw, cdml_stream_t stream) {
  return mx_w_launch<kWF32>("npair_mixed_grad_f32", S, lds, ids, B, neg_col, mem_col, mem_id, M, bias, lq_u, mem_bias,
                            temperature, symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_mixed_split_x3(const float *e, int64_t lde, int B, int D, uint16_t *A3, int64_t lda, int64_t plane_a,
                                         uint16_t *R3, int64_t ldr, int64_t plane_r, uint16_t *T3, int64_t ldt,
                                         int64_t plane_t, int64_t neg_row, cdml_stream_t stream) {
  const char *who = "npair_mixed_split_x3";
  CDML_REQUIRE(e && A3 && R3 && T3, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(B >= 4 && mult4(B) && D >= 4 && mult4(D), CDML_E_BADARG, "%s: B and D must be positive multiples of 4 (got %d, %d)",
               who, B, D);
  CDML_REQUIRE(lde >= D && mult4(lde) && aligned16(e), CDML_E_BADARG,
               "%s: e needs a 16-B aligned base and lde >= D (%d), a multiple of 4 (got %lld)", who, D, (long long)lde);
  CDML_REQUIRE(neg_row >= B && mult4(neg_row), CDML_E_BADARG, "%s: neg_row must be >= B (%d) and a multiple of 4, got %lld", who, B,
               (long long)neg_row);
  const auto al8 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
  CDML_REQUIRE(al8(A3) && al8(R3) && al8(T3) && mult4(lda) && mult4(plane_a) && mult4(ldr) && mult4(plane_r) && mult4(ldt) &&
                   mult4(plane_t),
               CDML_E_BADARG, "%s: the plane images need 8-B aligned bases, leading dimensions and plane strides multiples of 4", who);
  CDML_REQUIRE(plane_a >= D && lda >= 2 * plane_a + D && plane_r >= D && ldr >= 2 * plane_r + D, CDML_E_BADARG,
               "%s: row images need plane >= D (%d) and ld >= 2 plane + D (got A3 %lld / %lld, R3 %lld / %lld)", who, D,
               (long long)plane_a, (long long)lda, (long long)plane_r, (long long)ldr);
  CDML_REQUIRE(plane_t >= neg_row + B && ldt >= 2 * plane_t + neg_row + B, CDML_E_BADARG,
               "%s: the transposed image needs plane_t >= neg_row + B (%lld) and ldt >= 2 plane_t + neg_row + B (got %lld / %lld)",
               who, (long long)(neg_row + B), (long long)plane_t, (long long)ldt);
  const dim3 grid((unsigned)((D + kMxTile - 1) / kMxTile), (unsigned)((B + kMxTile - 1) / kMxTile), 3);
  hipLaunchKernelGGL(k_mixed_split, grid, dim3(kMxThreads), 0, (hipStream_t)stream, e, lde, B, D,
                     reinterpret_cast<__bf16 *>(A3), lda, plane_a, reinterpret_cast<__bf16 *>(R3), ldr, plane_r,
                     reinterpret_cast<__bf16 *>(T3), ldt, plane_t, neg_row);
  return check_launch(who);
}

// Multi-class N-pair loss (Sohn 2016; an InfoNCE / sampled softmax with in-batch negatives) over the score matrix
// S[i][j] = <a_i, p_j> of a batch of B pairs -- build-defined, the reference has only the triplet hinge (losses.py:20-49).
//
//   row term     m_ij = 1 if j == i or id(p_j) is neither id(a_i) nor id(p_i)   (the in-batch sampler's validity rule)
//                lse_i = log sum_j m_ij exp(S_ij / t),   L_row = mean_i (lse_i - S_ii / t)
//   column term  m'_ij = 1 if i == j or id(a_i) is neither id(a_j) nor id(p_j)
//                lse'_j = log sum_i m'_ij exp(S_ij / t), L_col = mean_j (lse'_j - S_jj / t)
//   loss         L_row, or (L_row + L_col) / 2 with `symmetric`
//   gradient     W_ij = (m_ij exp(S_ij / t - lse_i) - d_ij) / (B t)  [+ the column term's, halved]:  dA = W P, dP = W^T A
//
// Four launches, all enqueue-only, no atomics, every sum in a fixed order (the results are bit-reproducible):
//   k_npair_rows      one block per anchor row: one coalesced pass over S[i][:] with an online (max, sum-exp) per lane,
//                     combined by a fixed butterfly and then wave by wave -> lse_i and the row's loss / stat partials
//   k_npair_cols      (symmetric) a 256-row chunk x 256 columns per block, one column per lane: coalesced rows of S,
//                     online (max, sum-exp) per column and chunk
//   k_npair_col_fold  one lane per column folds the chunks in order -> lse'_j and the column's loss term
//   k_npair_stats     one block: the step scalars from the per-row partials in a fixed order (as k_loss_stats does)
//   k_npair_w<X3>     W, four columns per lane, as three exact bf16 planes [B][hi | mid | lo] (the operand layout of the
//                     plane GEMMs, split as cdml_split_f32_bf16x3 splits) or as fp32 (precision "f32")
#include "common.h"
#include <math.h>

namespace cdml {
namespace {

constexpr int kNpThreads = 256;
constexpr int kNpChunk = 256;          // rows per block of the column pass

__device__ __forceinline__ void np_split3(float v, __bf16 &h, __bf16 &m, __bf16 &l) {
  h = (__bf16)v;
  const float r = v - (float)h;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

// (m, s) <- the pair for the values summarised by (m, s) and by (m2, s2); an empty pair is (-inf, 0)
__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  if (mx == -INFINITY) return;
  s = s * expf(m - mx) + s2 * expf(m2 - mx);
  m = mx;
}

__device__ __forceinline__ void lse_add(float &m, float &s, float x) {
  if (x > m) {
    s = s * expf(m - x) + 1.f;
    m = x;
  } else {
    s += expf(x - m);
  }
}

// ids: int32[2B], 2i = id(a_i), 2i+1 = id(p_i); NULL = every row a video of its own
__device__ __forceinline__ bool row_counts(const int32_t *ids, int i, int j, int ida, int idp) {
  if (j == i || !ids) return true;
  const int q = ids[2 * j + 1];
  return q != ida && q != idp;
}

__device__ __forceinline__ bool col_counts(const int32_t *ids, int i, int j, int idaj, int idpj) {
  if (i == j || !ids) return true;
  const int q = ids[2 * i];
  return q != idaj && q != idpj;
}

// part[4 i .. 4 i + 3] = {lse_i - S_ii / t, 2 - 2 S_ii, sum over the counted j != i of 2 - 2 S_ij, their count}
__global__ void __launch_bounds__(kNpThreads)
k_npair_rows(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t,
             float *__restrict__ lse, float *__restrict__ part) {
  __shared__ float sm[kNpThreads / kWave][4];
  const int i = blockIdx.x;
  const float *row = S + (int64_t)i * lds;
  const int ida = ids ? ids[2 * i] : 0, idp = ids ? ids[2 * i + 1] : 0;
  float m = -INFINITY, s = 0.f, nsum = 0.f, ncnt = 0.f;
  for (int j = threadIdx.x; j < B; j += kNpThreads) {
    if (!row_counts(ids, i, j, ida, idp)) continue;
    const float v = row[j];
    lse_add(m, s, v * inv_t);
    if (j != i) {
      nsum += 2.f - 2.f * v;
      ncnt += 1.f;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
    lse_merge(m, s, m2, s2);
  }
  nsum = wave_sum(nsum);
  ncnt = wave_sum(ncnt);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    sm[wave][0] = m;
    sm[wave][1] = s;
    sm[wave][2] = nsum;
    sm[wave][3] = ncnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0][0], Sx = sm[0][1], ns = sm[0][2], nc = sm[0][3];
    for (int w = 1; w < kNpThreads / kWave; ++w) {
      lse_merge(M, Sx, sm[w][0], sm[w][1]);
      ns += sm[w][2];
      nc += sm[w][3];
    }
    const float sii = row[i];
    const float l = M + logf(Sx);
    lse[i] = l;
    *reinterpret_cast<float4 *>(part + 4 * (int64_t)i) = make_float4(l - sii * inv_t, 2.f - 2.f * sii, ns, nc);
  }
}

// cm / cs [chunk][B]: the (max, sum-exp) of column j over rows chunk * kNpChunk .. + kNpChunk - 1
__global__ void __launch_bounds__(kNpThreads)
k_npair_cols(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t,
             float *__restrict__ cm, float *__restrict__ cs) {
  const int j = blockIdx.x * kNpThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (j >= B) return;
  const int idaj = ids ? ids[2 * j] : 0, idpj = ids ? ids[2 * j + 1] : 0;
  const int i0 = c * kNpChunk, i1 = min(B, i0 + kNpChunk);
  float m = -INFINITY, s = 0.f;
  for (int i = i0; i < i1; ++i) {
    if (!col_counts(ids, i, j, idaj, idpj)) continue;
    lse_add(m, s, S[(int64_t)i * lds + j] * inv_t);
  }
  cm[(int64_t)c * B + j] = m;
  cs[(int64_t)c * B + j] = s;
}

// lse[B + j] = lse'_j, closs[j] = lse'_j - S_jj / t: the chunks folded in order
__global__ void __launch_bounds__(kNpThreads)
k_npair_col_fold(const float *__restrict__ S, int64_t lds, int B, int chunks, float inv_t, const float *__restrict__ cm,
                 const float *__restrict__ cs, float *__restrict__ lse, float *__restrict__ closs) {
  const int j = blockIdx.x * kNpThreads + threadIdx.x;
  if (j >= B) return;
  float m = -INFINITY, s = 0.f;
  for (int c = 0; c < chunks; ++c) lse_merge(m, s, cm[(int64_t)c * B + j], cs[(int64_t)c * B + j]);
  const float l = m + logf(s);
  lse[B + j] = l;
  closs[j] = l - S[(int64_t)j * lds + j] * inv_t;
}

// stats[0] = loss, [1] = mean |a_i - p_i|^2, [2] = mean |a_i - p_j|^2 over the counted row-term negatives, [3] = the fraction
// of off-diagonal row-term entries that count (squared distances of unit rows: 2 - 2 S)
__global__ void __launch_bounds__(1024)
k_npair_stats(const float *__restrict__ part, const float *__restrict__ closs, int B, int symmetric,
              float *__restrict__ stats) {
  __shared__ float sm[5][1024 / kWave];
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < B; i += 1024) {
    const float4 p = *reinterpret_cast<const float4 *>(part + 4 * (int64_t)i);
    acc[0] += p.x;
    acc[1] += p.y;
    acc[2] += p.z;
    acc[3] += p.w;
    if (symmetric) acc[4] += closs[i];
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const float v = wave_sum(acc[c]);
    if (lane == 0) sm[c][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < 1024 / kWave; ++w)
      for (int c = 0; c < 5; ++c) t[c] += sm[c][w];
    const float fb = (float)B;
    stats[0] = symmetric ? 0.5f * (t[0] / fb + t[4] / fb) : t[0] / fb;
    stats[1] = t[1] / fb;
    stats[2] = t[3] > 0.f ? t[2] / t[3] : 0.f;
    stats[3] = B > 1 ? t[3] / (fb * (float)(B - 1)) : 0.f;
  }
}

__device__ __forceinline__ float npair_w(const int32_t *ids, int i, int j, int ida, int idp, float v, float inv_t, float lse_r,
                                         const float *lse_c, int symmetric, float scale) {
  float r = row_counts(ids, i, j, ida, idp) ? expf(v * inv_t - lse_r) : 0.f;
  if (j == i) r -= 1.f;
  if (symmetric) {
    const int idaj = ids ? ids[2 * j] : 0, idpj = ids ? ids[2 * j + 1] : 0;
    float c = col_counts(ids, i, j, idaj, idpj) ? expf(v * inv_t - lse_c[j]) : 0.f;
    if (j == i) c -= 1.f;
    r = 0.5f * (r + c);
  }
  return r * scale;
}

// row i = blockIdx.x, columns 4 (blockIdx.y * kNpThreads + threadIdx.x) .. + 3; columns >= B are not written
template <bool X3>
__global__ void __launch_bounds__(kNpThreads)
k_npair_w(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t, int symmetric,
          const float *__restrict__ lse, float scale, void *__restrict__ Wout, int64_t ldw, int64_t plane) {
  const int i = blockIdx.x;
  const int j0 = (blockIdx.y * kNpThreads + threadIdx.x) * 4;
  if (j0 >= B) return;
  const int ida = ids ? ids[2 * i] : 0, idp = ids ? ids[2 * i + 1] : 0;
  const float lr = lse[i];
  const float *lc = lse + B;
  const float *row = S + (int64_t)i * lds;
  float w[4];
  if (j0 + 3 < B) {
    const float4 v = *reinterpret_cast<const float4 *>(row + j0);
    w[0] = npair_w(ids, i, j0, ida, idp, v.x, inv_t, lr, lc, symmetric, scale);
    w[1] = npair_w(ids, i, j0 + 1, ida, idp, v.y, inv_t, lr, lc, symmetric, scale);
    w[2] = npair_w(ids, i, j0 + 2, ida, idp, v.z, inv_t, lr, lc, symmetric, scale);
    w[3] = npair_w(ids, i, j0 + 3, ida, idp, v.w, inv_t, lr, lc, symmetric, scale);
  } else {
    for (int q = 0; q < 4; ++q)
      w[q] = (j0 + q < B) ? npair_w(ids, i, j0 + q, ida, idp, row[j0 + q], inv_t, lr, lc, symmetric, scale) : 0.f;
  }
  const int n = min(4, B - j0);
  if (X3) {
    using bf4 = __attribute__((ext_vector_type(4))) __bf16;
    bf4 h, m, l;
    for (int q = 0; q < 4; ++q) {
      __bf16 a, b, c;
      np_split3(w[q], a, b, c);
      h[q] = a;
      m[q] = b;
      l[q] = c;
    }
    __bf16 *dst = static_cast<__bf16 *>(Wout) + (int64_t)i * ldw + j0;
    if (n == 4) {
      *reinterpret_cast<bf4 *>(dst) = h;
      *reinterpret_cast<bf4 *>(dst + plane) = m;
      *reinterpret_cast<bf4 *>(dst + 2 * plane) = l;
    } else {
      for (int q = 0; q < n; ++q) {
        dst[q] = h[q];
        dst[plane + q] = m[q];
        dst[2 * plane + q] = l[q];
      }
    }
  } else {
    float *dst = static_cast<float *>(Wout) + (int64_t)i * ldw + j0;
    if (n == 4)
      *reinterpret_cast<float4 *>(dst) = make_float4(w[0], w[1], w[2], w[3]);
    else
      for (int q = 0; q < n; ++q) dst[q] = w[q];
  }
}

int np_chunks(int B) { return (B + kNpChunk - 1) / kNpChunk; }

// workspace floats: part [4B] | closs [B] | cm [chunks B] | cs [chunks B]
size_t np_ws_bytes(int B) {
  if (B < 1) return 0;
  const size_t f = (size_t)B * (5 + 2 * (size_t)np_chunks(B));
  return (f * sizeof(float) + 255) / 256 * 256;
}

int np_check(const char *who, const float *S, int64_t lds, int B, float temperature, const float *lse) {
  CDML_REQUIRE(S && lse, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(B >= 1, CDML_E_BADARG, "%s: B must be >= 1, got %d", who, B);
  CDML_REQUIRE(isfinite(temperature) && temperature > 0.f, CDML_E_BADARG, "%s: temperature must be finite and > 0, got %g",
               who, (double)temperature);
  CDML_REQUIRE(lds >= B && (lds & 3) == 0 && aligned16(S), CDML_E_BADARG,
               "%s: S needs a 16-B aligned base and lds >= B (%d), a multiple of 4 (got %lld)", who, B, (long long)lds);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" size_t cdml_npair_workspace(int B) { return np_ws_bytes(B); }

extern "C" int cdml_npair_stats(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                float *lse, float *stats, void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = np_check("npair_stats", S, lds, B, temperature, lse)) return rc;
  CDML_REQUIRE(stats && workspace, CDML_E_BADARG, "npair_stats: null pointer");
  CDML_REQUIRE(aligned16(workspace) && workspace_bytes >= np_ws_bytes(B), CDML_E_BADARG,
               "npair_stats: the workspace must be 16-B aligned and hold cdml_npair_workspace(%d) = %zu bytes (got %zu)", B,
               np_ws_bytes(B), workspace_bytes);
  const float inv_t = 1.0f / temperature;
  const int chunks = np_chunks(B);
  float *part = static_cast<float *>(workspace), *closs = part + 4 * (size_t)B;
  float *cm = closs + B, *cs = cm + (size_t)chunks * B;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_npair_rows, dim3(B), dim3(kNpThreads), 0, st, S, lds, ids, B, inv_t, lse, part);
  if (int rc = check_launch("npair_stats rows")) return rc;
  if (symmetric) {
    const unsigned gx = (unsigned)((B + kNpThreads - 1) / kNpThreads);
    hipLaunchKernelGGL(k_npair_cols, dim3(gx, chunks), dim3(kNpThreads), 0, st, S, lds, ids, B, inv_t, cm, cs);
    if (int rc = check_launch("npair_stats columns")) return rc;
    hipLaunchKernelGGL(k_npair_col_fold, dim3(gx), dim3(kNpThreads), 0, st, S, lds, B, chunks, inv_t, cm, cs, lse, closs);
    if (int rc = check_launch("npair_stats column fold")) return rc;
  }
  hipLaunchKernelGGL(k_npair_stats, dim3(1), dim3(1024), 0, st, part, closs, B, symmetric ? 1 : 0, stats);
  return check_launch("npair_stats");
}

extern "C" int cdml_npair_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                  const float *lse, uint16_t *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  if (int rc = np_check("npair_grad_x3", S, lds, B, temperature, lse)) return rc;
  CDML_REQUIRE(W, CDML_E_BADARG, "npair_grad_x3: null pointer");
  CDML_REQUIRE(plane >= B && ldw >= 2 * plane + B && (plane & 3) == 0 && (ldw & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(W) & 7) == 0,
               CDML_E_BADARG,
               "npair_grad_x3: W needs an 8-B aligned base, plane >= B (%d) and ldw >= 2 plane + B, both multiples of 4 "
               "(got plane %lld, ldw %lld)", B, (long long)plane, (long long)ldw);
  const dim3 grid((unsigned)B, (unsigned)((B + 4 * kNpThreads - 1) / (4 * kNpThreads)));
  hipLaunchKernelGGL(k_npair_w<true>, grid, dim3(kNpThreads), 0, (hipStream_t)stream, S, lds, ids, B, 1.0f / temperature,
                     symmetric ? 1 : 0, lse, 1.0f / ((float)B * temperature), (void *)W, ldw, plane);
  return check_launch("npair_grad_x3");
}

extern "C" int cdml_npair_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                   const float *lse, float *W, int64_t ldw, cdml_stream_t stream) {
  if (int rc = np_check("npair_grad_f32", S, lds, B, temperature, lse)) return rc;
  CDML_REQUIRE(W, CDML_E_BADARG, "npair_grad_f32: null pointer");
  CDML_REQUIRE(ldw >= B && (ldw & 3) == 0 && aligned16(W), CDML_E_BADARG,
               "npair_grad_f32: W needs a 16-B aligned base and ldw >= B (%d), a multiple of 4 (got %lld)", B, (long long)ldw);
  const dim3 grid((unsigned)B, (unsigned)((B + 4 * kNpThreads - 1) / (4 * kNpThreads)));
  hipLaunchKernelGGL(k_npair_w<false>, grid, dim3(kNpThreads), 0, (hipStream_t)stream, S, lds, ids, B, 1.0f / temperature,
                     symmetric ? 1 : 0, lse, 1.0f / ((float)B * temperature), (void *)W, ldw, (int64_t)0);
  return check_launch("npair_grad_f32");
}

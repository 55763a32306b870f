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
//   k_npair_w<FMT>    W, four columns per lane, as three exact bf16 planes [B][hi | mid | lo] (the operand layout of the
//                     plane GEMMs, split as cdml_split_f32_bf16x3 splits), as fp32 (precision "f32") or as ONE bf16 plane,
//                     the round-to-nearest-even of that fp32 value (precision "bf16": include/cdml_npair_bf16.h)
//
// Cross-batch memory (cdml_npair_memory_*): S = A [P; Mem]^T is [B][B + M], the memory's M columns at mem_col.  The row term
// also counts slot k when mem_id[k] >= 0 is neither id(a_i) nor id(p_i); the column term stays over the in-batch block.
//   k_npair_rows<true>   the row pass going on over the memory columns (float4 / int4 per lane)
//   k_npair_mem_w<FMT>   W's memory block, c_ik exp(S_ik / t - lse_i) / (B t) (halved with `symmetric`)
//   k_npair_mem_push<X3> the ring push of the step's positives (after the products that read the memory), fp32 rows + ids,
//                        and for X3 the slots' row-plane and transposed-plane operand images
//
// Sampling-bias correction (logQ, Yi et al. 2019; cdml_npair_logq_* / cdml_npair_memory_logq_*): every logit that enters a
// log-sum-exp or the diagonal loses the log sampling probability of its candidate -- row term column j: S_ij / t - lq(p_j),
// memory slot k: S_ik / t - lq(mem_id[k]), column term row i: S_ij / t - lq(a_i).  The passes read it per slot, bias[2i] =
// lq(a_i), bias[2i + 1] = lq(p_i) (laid out like ids) and mem_bias[k]: the BIAS instantiations of the kernels below; the
// BIAS = false ones are the arithmetic of the uncorrected loss.  csrc/npair_logq.hip fills the vectors.
#include "common.h"
#include "../../include/cdml_npair_bf16.h"
#include <math.h>

namespace cdml {
namespace {

constexpr int kNpThreads = 256;
constexpr int kNpChunk = 256;          // rows per block of the column pass
// what k_npair_w / k_npair_mem_w store: fp32, three exact bf16 planes, or one bf16 plane (the rounded fp32 value)
enum : int { kWF32 = 0, kWX3 = 1, kWBf16 = 2 };

__device__ __forceinline__ void np_split3(float v, __bf16 &h, __bf16 &m, __bf16 &l) { split3_bf16(v, h, m, l); }

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

// memory slot k counts for anchor i when it holds a row (mem_id >= 0) of neither the anchor's nor its positive's video
__device__ __forceinline__ bool mem_counts(const int32_t *ids, int q, int ida, int idp) {
  return q >= 0 && (!ids || (q != ida && q != idp));
}

template <bool BIAS>
__device__ __forceinline__ void mem_add(const int32_t *ids, float v, int q, float b, int ida, int idp, float inv_t, float &m,
                                        float &s, float &nsum, float &ncnt) {
  if (!mem_counts(ids, q, ida, idp)) return;
  if constexpr (BIAS)
    lse_add(m, s, v * inv_t - b);
  else
    lse_add(m, s, v * inv_t);
  nsum += 2.f - 2.f * v;
  ncnt += 1.f;
}

// part[4 i .. 4 i + 3] = {lse_i - S_ii / t, 2 - 2 S_ii, sum over the counted j != i of 2 - 2 S_ij, their count}
// MEM: the row goes on over the n_mem memory columns at mem_col .. mem_col + n_mem - 1 of S (cross-batch memory, slot ids mem_id;
// four columns per lane per pass, after the in-batch columns: the same fixed order on every run)
// BIAS: column j's logit less bias[2j + 1], slot k's less mem_bias[k] (part[4 i] too: lse_i - (S_ii / t - bias[2i + 1]))
template <bool MEM, bool BIAS>
__global__ void __launch_bounds__(kNpThreads)
k_npair_rows(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t,
             float *__restrict__ lse, float *__restrict__ part, int64_t mem_col, const int32_t *__restrict__ mem_id, int n_mem,
             const float *__restrict__ bias, const float *__restrict__ mem_bias) {
  __shared__ float sm[kNpThreads / kWave][4];
  const int i = blockIdx.x;
  const float *row = S + (int64_t)i * lds;
  const int ida = ids ? ids[2 * i] : 0, idp = ids ? ids[2 * i + 1] : 0;
  float m = -INFINITY, s = 0.f, nsum = 0.f, ncnt = 0.f;
  for (int j = threadIdx.x; j < B; j += kNpThreads) {
    if (!row_counts(ids, i, j, ida, idp)) continue;
    const float v = row[j];
    if constexpr (BIAS)
      lse_add(m, s, v * inv_t - bias[2 * j + 1]);
    else
      lse_add(m, s, v * inv_t);
    if (j != i) {
      nsum += 2.f - 2.f * v;
      ncnt += 1.f;
    }
  }
  if constexpr (MEM) {
    const float *mrow = row + mem_col;
    for (int k = 4 * threadIdx.x; k < n_mem; k += 4 * kNpThreads) {
      const float4 v = *reinterpret_cast<const float4 *>(mrow + k);
      const int4 q = *reinterpret_cast<const int4 *>(mem_id + k);
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (BIAS) b = *reinterpret_cast<const float4 *>(mem_bias + k);
      mem_add<BIAS>(ids, v.x, q.x, b.x, ida, idp, inv_t, m, s, nsum, ncnt);
      mem_add<BIAS>(ids, v.y, q.y, b.y, ida, idp, inv_t, m, s, nsum, ncnt);
      mem_add<BIAS>(ids, v.z, q.z, b.z, ida, idp, inv_t, m, s, nsum, ncnt);
      mem_add<BIAS>(ids, v.w, q.w, b.w, ida, idp, inv_t, m, s, nsum, ncnt);
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
    float d;
    if constexpr (BIAS)
      d = sii * inv_t - bias[2 * i + 1];
    else
      d = sii * inv_t;
    *reinterpret_cast<float4 *>(part + 4 * (int64_t)i) = make_float4(l - d, 2.f - 2.f * sii, ns, nc);
  }
}

// cm / cs [chunk][B]: the (max, sum-exp) of column j over rows chunk * kNpChunk .. + kNpChunk - 1
// BIAS: row i's logit less bias[2i] (the anchor's: one value per row, the same for every lane of the wave)
template <bool BIAS>
__global__ void __launch_bounds__(kNpThreads)
k_npair_cols(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t,
             float *__restrict__ cm, float *__restrict__ cs, const float *__restrict__ bias) {
  const int j = blockIdx.x * kNpThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (j >= B) return;
  const int idaj = ids ? ids[2 * j] : 0, idpj = ids ? ids[2 * j + 1] : 0;
  const int i0 = c * kNpChunk, i1 = min(B, i0 + kNpChunk);
  float m = -INFINITY, s = 0.f;
  for (int i = i0; i < i1; ++i) {
    if (!col_counts(ids, i, j, idaj, idpj)) continue;
    if constexpr (BIAS)
      lse_add(m, s, S[(int64_t)i * lds + j] * inv_t - bias[2 * i]);
    else
      lse_add(m, s, S[(int64_t)i * lds + j] * inv_t);
  }
  cm[(int64_t)c * B + j] = m;
  cs[(int64_t)c * B + j] = s;
}

// lse[B + j] = lse'_j, closs[j] = lse'_j - S_jj / t (BIAS: - (S_jj / t - bias[2j])): the chunks folded in order
template <bool BIAS>
__global__ void __launch_bounds__(kNpThreads)
k_npair_col_fold(const float *__restrict__ S, int64_t lds, int B, int chunks, float inv_t, const float *__restrict__ cm,
                 const float *__restrict__ cs, float *__restrict__ lse, float *__restrict__ closs, const float *__restrict__ bias) {
  const int j = blockIdx.x * kNpThreads + threadIdx.x;
  if (j >= B) return;
  float m = -INFINITY, s = 0.f;
  for (int c = 0; c < chunks; ++c) lse_merge(m, s, cm[(int64_t)c * B + j], cs[(int64_t)c * B + j]);
  const float l = m + logf(s);
  lse[B + j] = l;
  if constexpr (BIAS)
    closs[j] = l - (S[(int64_t)j * lds + j] * inv_t - bias[2 * j]);
  else
    closs[j] = l - S[(int64_t)j * lds + j] * inv_t;
}

// stats[0] = loss, [1] = mean |a_i - p_i|^2, [2] = mean |a_i - p_j|^2 over the counted row-term negatives, [3] = the fraction
// of off-diagonal row-term entries that count (squared distances of unit rows: 2 - 2 S); M > 0: the memory's B M entries
// are row-term negatives too
__global__ void __launch_bounds__(1024)
k_npair_stats(const float *__restrict__ part, const float *__restrict__ closs, int B, int symmetric, int M,
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
    const float den = M ? fb * (float)(B - 1) + fb * (float)M : fb * (float)(B - 1);
    stats[3] = den > 0.f ? t[3] / den : 0.f;
  }
}

// BIAS: the row term's logit less bp = bias[2j + 1] (positive j's), the column term's less ba = bias[2i] (anchor i's)
template <bool BIAS>
__device__ __forceinline__ float npair_w(const int32_t *ids, int i, int j, int ida, int idp, float v, float inv_t, float lse_r,
                                         const float *lse_c, int symmetric, float scale, float bp, float ba) {
  float r;
  if constexpr (BIAS)
    r = row_counts(ids, i, j, ida, idp) ? expf(v * inv_t - bp - lse_r) : 0.f;
  else
    r = row_counts(ids, i, j, ida, idp) ? expf(v * inv_t - lse_r) : 0.f;
  if (j == i) r -= 1.f;
  if (symmetric) {
    const int idaj = ids ? ids[2 * j] : 0, idpj = ids ? ids[2 * j + 1] : 0;
    float c;
    if constexpr (BIAS)
      c = col_counts(ids, i, j, idaj, idpj) ? expf(v * inv_t - ba - lse_c[j]) : 0.f;
    else
      c = col_counts(ids, i, j, idaj, idpj) ? expf(v * inv_t - lse_c[j]) : 0.f;
    if (j == i) c -= 1.f;
    r = 0.5f * (r + c);
  }
  return r * scale;
}

// row i = blockIdx.x, columns 4 (blockIdx.y * kNpThreads + threadIdx.x) .. + 3; columns >= B are not written
template <int FMT, bool BIAS>
__global__ void __launch_bounds__(kNpThreads)
k_npair_w(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t, int symmetric,
          const float *__restrict__ lse, float scale, void *__restrict__ Wout, int64_t ldw, int64_t plane,
          const float *__restrict__ bias) {
  const int i = blockIdx.x;
  const int j0 = (blockIdx.y * kNpThreads + threadIdx.x) * 4;
  if (j0 >= B) return;
  const int ida = ids ? ids[2 * i] : 0, idp = ids ? ids[2 * i + 1] : 0;
  const float lr = lse[i];
  const float *lc = lse + B;
  const float *row = S + (int64_t)i * lds;
  const float ba = BIAS ? bias[2 * i] : 0.f;
  float w[4];
  if (j0 + 3 < B) {
    const float4 v = *reinterpret_cast<const float4 *>(row + j0);
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
    if constexpr (BIAS) {                            // the four columns' slots 2j .. 2j + 7: two 16-B loads, positives odd
      b0 = *reinterpret_cast<const float4 *>(bias + 2 * j0);
      b1 = *reinterpret_cast<const float4 *>(bias + 2 * j0 + 4);
    }
    w[0] = npair_w<BIAS>(ids, i, j0, ida, idp, v.x, inv_t, lr, lc, symmetric, scale, b0.y, ba);
    w[1] = npair_w<BIAS>(ids, i, j0 + 1, ida, idp, v.y, inv_t, lr, lc, symmetric, scale, b0.w, ba);
    w[2] = npair_w<BIAS>(ids, i, j0 + 2, ida, idp, v.z, inv_t, lr, lc, symmetric, scale, b1.y, ba);
    w[3] = npair_w<BIAS>(ids, i, j0 + 3, ida, idp, v.w, inv_t, lr, lc, symmetric, scale, b1.w, ba);
  } else {
    for (int q = 0; q < 4; ++q)
      w[q] = (j0 + q < B) ? npair_w<BIAS>(ids, i, j0 + q, ida, idp, row[j0 + q], inv_t, lr, lc, symmetric, scale,
                                          BIAS ? bias[2 * (j0 + q) + 1] : 0.f, ba)
                          : 0.f;
  }
  const int n = min(4, B - j0);
  if constexpr (FMT == kWX3) {
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
  } else if constexpr (FMT == kWBf16) {
    using bf4 = __attribute__((ext_vector_type(4))) __bf16;
    bf4 r;
    for (int q = 0; q < 4; ++q) r[q] = (__bf16)w[q];
    __bf16 *dst = static_cast<__bf16 *>(Wout) + (int64_t)i * ldw + j0;
    if (n == 4)
      *reinterpret_cast<bf4 *>(dst) = r;
    else
      for (int q = 0; q < n; ++q) dst[q] = r[q];
  } else {
    float *dst = static_cast<float *>(Wout) + (int64_t)i * ldw + j0;
    if (n == 4)
      *reinterpret_cast<float4 *>(dst) = make_float4(w[0], w[1], w[2], w[3]);
    else
      for (int q = 0; q < n; ++q) dst[q] = w[q];
  }
}

// The memory block of W: W[i][mem_col + k] = c_ik exp(S[i][mem_col + k] / t - lse_i) * scale (scale = 1 / (B t), halved
// with `symmetric`: the column term has no memory part).  Row i = blockIdx.x, slots 4 (blockIdx.y * kNpThreads +
// threadIdx.x) .. + 3 (M a multiple of 4).  BIAS: slot k's logit less mem_bias[k]
template <int FMT, bool BIAS>
__global__ void __launch_bounds__(kNpThreads)
k_npair_mem_w(const float *__restrict__ S, int64_t lds, int64_t mem_col, const int32_t *__restrict__ ids,
              const int32_t *__restrict__ mem_id, int M, float inv_t, const float *__restrict__ lse, float scale,
              void *__restrict__ Wout, int64_t ldw, int64_t plane, const float *__restrict__ mem_bias) {
  const int i = blockIdx.x;
  const int k0 = (blockIdx.y * kNpThreads + threadIdx.x) * 4;
  if (k0 >= M) return;
  const int ida = ids ? ids[2 * i] : 0, idp = ids ? ids[2 * i + 1] : 0;
  const float lr = lse[i];
  const float4 v = *reinterpret_cast<const float4 *>(S + (int64_t)i * lds + mem_col + k0);
  const int4 q = *reinterpret_cast<const int4 *>(mem_id + k0);
  float w[4];
  if constexpr (BIAS) {
    const float4 b = *reinterpret_cast<const float4 *>(mem_bias + k0);
    w[0] = mem_counts(ids, q.x, ida, idp) ? expf(v.x * inv_t - b.x - lr) * scale : 0.f;
    w[1] = mem_counts(ids, q.y, ida, idp) ? expf(v.y * inv_t - b.y - lr) * scale : 0.f;
    w[2] = mem_counts(ids, q.z, ida, idp) ? expf(v.z * inv_t - b.z - lr) * scale : 0.f;
    w[3] = mem_counts(ids, q.w, ida, idp) ? expf(v.w * inv_t - b.w - lr) * scale : 0.f;
  } else {
    w[0] = mem_counts(ids, q.x, ida, idp) ? expf(v.x * inv_t - lr) * scale : 0.f;
    w[1] = mem_counts(ids, q.y, ida, idp) ? expf(v.y * inv_t - lr) * scale : 0.f;
    w[2] = mem_counts(ids, q.z, ida, idp) ? expf(v.z * inv_t - lr) * scale : 0.f;
    w[3] = mem_counts(ids, q.w, ida, idp) ? expf(v.w * inv_t - lr) * scale : 0.f;
  }
  if constexpr (FMT == kWX3) {
    using bf4 = __attribute__((ext_vector_type(4))) __bf16;
    bf4 h, m, l;
    for (int c = 0; c < 4; ++c) {
      __bf16 a, b, d;
      np_split3(w[c], a, b, d);
      h[c] = a;
      m[c] = b;
      l[c] = d;
    }
    __bf16 *dst = static_cast<__bf16 *>(Wout) + (int64_t)i * ldw + mem_col + k0;
    *reinterpret_cast<bf4 *>(dst) = h;
    *reinterpret_cast<bf4 *>(dst + plane) = m;
    *reinterpret_cast<bf4 *>(dst + 2 * plane) = l;
  } else if constexpr (FMT == kWBf16) {
    using bf4 = __attribute__((ext_vector_type(4))) __bf16;
    bf4 r;
    for (int c = 0; c < 4; ++c) r[c] = (__bf16)w[c];
    *reinterpret_cast<bf4 *>(static_cast<__bf16 *>(Wout) + (int64_t)i * ldw + mem_col + k0) = r;
  } else {
    *reinterpret_cast<float4 *>(static_cast<float *>(Wout) + (int64_t)i * ldw + mem_col + k0) =
        make_float4(w[0], w[1], w[2], w[3]);
  }
}

constexpr int kPushTile = 64;

// The ring push of step t = step_imm + *step_dev (when t >= start): slots s .. s + B - 1, s = ((t - start) mod (M / B)) B,
// take the B positives P[r] (fp32 rows, D columns) and their ids ids[2 r + 1].  X3: also the slots' operand images --
// R3[s + r][p * plane_r + c] and T3[c][p * plane_t + s + r] = bf16 plane p of P[r][c] (cdml_split_f32_bf16x3's split),
// the transposed one through a 64 x 64 LDS tile so that both stores run along contiguous addresses
template <bool X3>
__global__ void __launch_bounds__(kNpThreads)
k_npair_mem_push(const float *__restrict__ P, int64_t ldp, const int32_t *__restrict__ ids, int B, int D, uint64_t step_imm,
                 const uint64_t *__restrict__ step_dev, int64_t start, int M, float *__restrict__ mem, int64_t ldm,
                 int32_t *__restrict__ mem_id, __bf16 *__restrict__ R3, int64_t ldr, int64_t plane_r,
                 __bf16 *__restrict__ T3, int64_t ldt, int64_t plane_t) {
  __shared__ float tile[kPushTile][kPushTile + 1];
  const uint64_t t = step_imm + (step_dev ? *step_dev : 0);
  if (t < (uint64_t)start) return;
  const int64_t s = (int64_t)((t - (uint64_t)start) % (uint64_t)(M / B)) * B;
  const int c0 = blockIdx.x * kPushTile, r0 = blockIdx.y * kPushTile;
  const int lane = threadIdx.x % kPushTile, sub = threadIdx.x / kPushTile;
  constexpr int kStep = kNpThreads / kPushTile;
  if (blockIdx.x == 0 && threadIdx.x < kPushTile && r0 + (int)threadIdx.x < B)
    mem_id[s + r0 + threadIdx.x] = ids[2 * (r0 + threadIdx.x) + 1];
  for (int r = sub; r < kPushTile; r += kStep) {
    const int gr = r0 + r, gc = c0 + lane;
    if (gr >= B || gc >= D) continue;
    const float v = P[(int64_t)gr * ldp + gc];
    mem[(s + gr) * ldm + gc] = v;
    if (X3) {
      __bf16 h, m, l;
      np_split3(v, h, m, l);
      __bf16 *d = R3 + (s + gr) * ldr + gc;
      d[0] = h;
      d[plane_r] = m;
      d[2 * plane_r] = l;
      tile[r][lane] = v;
    }
  }
  if (!X3) return;
  __syncthreads();
  for (int c = sub; c < kPushTile; c += kStep) {
    const int gr = r0 + lane, gc = c0 + c;
    if (gr >= B || gc >= D) continue;
    __bf16 h, m, l;
    np_split3(tile[lane][c], h, m, l);
    __bf16 *d = T3 + (int64_t)gc * ldt + s + gr;
    d[0] = h;
    d[plane_t] = m;
    d[2 * plane_t] = l;
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

int np_bias_check(const char *who, const float *bias) {
  CDML_REQUIRE(bias, CDML_E_BADARG, "%s: null pointer (bias)", who);
  CDML_REQUIRE(aligned16(bias), CDML_E_BADARG, "%s: bias needs a 16-B aligned base", who);
  return CDML_OK;
}

// the statistics launches (rows, columns + fold with `symmetric`, step scalars); MEM: S's memory block at mem_col
template <bool MEM, bool BIAS>
int np_stats_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                    int64_t mem_col, const int32_t *mem_id, const float *mem_bias, int M, float temperature, int symmetric,
                    float *lse, float *stats, void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  CDML_REQUIRE(stats && workspace, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(aligned16(workspace) && workspace_bytes >= np_ws_bytes(B), CDML_E_BADARG,
               "%s: the workspace must be 16-B aligned and hold cdml_npair%s_workspace(%d) = %zu bytes (got %zu)", who,
               MEM ? "_memory" : "", B, np_ws_bytes(B), workspace_bytes);
  const float inv_t = 1.0f / temperature;
  const int chunks = np_chunks(B);
  float *part = static_cast<float *>(workspace), *closs = part + 4 * (size_t)B;
  float *cm = closs + B, *cs = cm + (size_t)chunks * B;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_npair_rows<MEM, BIAS>), dim3(B), dim3(kNpThreads), 0, st, S, lds, ids, B, inv_t, lse, part, mem_col,
                     mem_id, M, bias, mem_bias);
  if (int rc = check_launch(MEM ? "npair_memory_stats rows" : "npair_stats rows")) return rc;
  if (symmetric) {                                   // (with a memory: the in-batch block as it stands, through lds)
    const unsigned gx = (unsigned)((B + kNpThreads - 1) / kNpThreads);
    hipLaunchKernelGGL(k_npair_cols<BIAS>, dim3(gx, chunks), dim3(kNpThreads), 0, st, S, lds, ids, B, inv_t, cm, cs, bias);
    if (int rc = check_launch(MEM ? "npair_memory_stats columns" : "npair_stats columns")) return rc;
    hipLaunchKernelGGL(k_npair_col_fold<BIAS>, dim3(gx), dim3(kNpThreads), 0, st, S, lds, B, chunks, inv_t, cm, cs, lse, closs,
                       bias);
    if (int rc = check_launch(MEM ? "npair_memory_stats column fold" : "npair_stats column fold")) return rc;
  }
  hipLaunchKernelGGL(k_npair_stats, dim3(1), dim3(1024), 0, st, part, closs, B, symmetric ? 1 : 0, MEM ? M : 0, stats);
  return check_launch(who);
}

int np_w_x3_check(const char *who, int B, const uint16_t *W, int64_t ldw, int64_t plane) {
  CDML_REQUIRE(W, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(plane >= B && ldw >= 2 * plane + B && (plane & 3) == 0 && (ldw & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(W) & 7) == 0,
               CDML_E_BADARG,
               "%s: W needs an 8-B aligned base, plane >= B (%d) and ldw >= 2 plane + B, both multiples of 4 "
               "(got plane %lld, ldw %lld)", who, B, (long long)plane, (long long)ldw);
  return CDML_OK;
}

int np_w_f32_check(const char *who, int B, const float *W, int64_t ldw) {
  CDML_REQUIRE(W, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(ldw >= B && (ldw & 3) == 0 && aligned16(W), CDML_E_BADARG,
               "%s: W needs a 16-B aligned base and ldw >= B (%d), a multiple of 4 (got %lld)", who, B, (long long)ldw);
  return CDML_OK;
}

template <int FMT, bool BIAS>
int np_w_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, const float *bias, float temperature,
                int symmetric, const float *lse, void *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  const dim3 grid((unsigned)B, (unsigned)((B + 4 * kNpThreads - 1) / (4 * kNpThreads)));
  hipLaunchKernelGGL((k_npair_w<FMT, BIAS>), grid, dim3(kNpThreads), 0, (hipStream_t)stream, S, lds, ids, B, 1.0f / temperature,
                     symmetric ? 1 : 0, lse, 1.0f / ((float)B * temperature), W, ldw, plane, bias);
  return check_launch(who);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" size_t cdml_npair_workspace(int B) { return np_ws_bytes(B); }

extern "C" int cdml_npair_stats(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                float *lse, float *stats, void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = np_check("npair_stats", S, lds, B, temperature, lse)) return rc;
  return np_stats_launch<false, false>("npair_stats", S, lds, ids, B, nullptr, 0, nullptr, nullptr, 0, temperature, symmetric,
                                       lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                  const float *lse, uint16_t *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  if (int rc = np_check("npair_grad_x3", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_w_x3_check("npair_grad_x3", B, W, ldw, plane)) return rc;
  return np_w_launch<kWX3, false>("npair_grad_x3", S, lds, ids, B, nullptr, temperature, symmetric, lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                   const float *lse, float *W, int64_t ldw, cdml_stream_t stream) {
  if (int rc = np_check("npair_grad_f32", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_w_f32_check("npair_grad_f32", B, W, ldw)) return rc;
  return np_w_launch<kWF32, false>("npair_grad_f32", S, lds, ids, B, nullptr, temperature, symmetric, lse, W, ldw, 0, stream);
}

// ---- the sampling-bias (logQ) corrected loss: bias[2B] per row as ids, laid out by csrc/npair_logq.hip ------------------

extern "C" int cdml_npair_logq_stats(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                     float temperature, int symmetric, float *lse, float *stats, void *workspace,
                                     size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = np_check("npair_logq_stats", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_logq_stats", bias)) return rc;
  return np_stats_launch<false, true>("npair_logq_stats", S, lds, ids, B, bias, 0, nullptr, nullptr, 0, temperature, symmetric,
                                      lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_logq_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                       float temperature, int symmetric, const float *lse, uint16_t *W, int64_t ldw,
                                       int64_t plane, cdml_stream_t stream) {
  if (int rc = np_check("npair_logq_grad_x3", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_logq_grad_x3", bias)) return rc;
  if (int rc = np_w_x3_check("npair_logq_grad_x3", B, W, ldw, plane)) return rc;
  return np_w_launch<kWX3, true>("npair_logq_grad_x3", S, lds, ids, B, bias, temperature, symmetric, lse, W, ldw, plane,
                                 stream);
}

extern "C" int cdml_npair_logq_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                        float temperature, int symmetric, const float *lse, float *W, int64_t ldw,
                                        cdml_stream_t stream) {
  if (int rc = np_check("npair_logq_grad_f32", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_logq_grad_f32", bias)) return rc;
  if (int rc = np_w_f32_check("npair_logq_grad_f32", B, W, ldw)) return rc;
  return np_w_launch<kWF32, true>("npair_logq_grad_f32", S, lds, ids, B, bias, temperature, symmetric, lse, W, ldw, 0, stream);
}

// ---- cross-batch memory (XBM, Wang et al. 2020): a ring of M earlier positives as extra row-term columns of S ----------

namespace cdml {
namespace {

int npm_check(const char *who, const float *S, int64_t lds, int B, int64_t mem_col, const int32_t *mem_id, int M,
              float temperature, const float *lse) {
  CDML_REQUIRE(S && lse && mem_id, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(B >= 1, CDML_E_BADARG, "%s: B must be >= 1, got %d", who, B);
  CDML_REQUIRE(M >= 4 && (M & 3) == 0, CDML_E_BADARG, "%s: the memory size M must be a positive multiple of 4, got %d", who, M);
  CDML_REQUIRE(isfinite(temperature) && temperature > 0.f, CDML_E_BADARG, "%s: temperature must be finite and > 0, got %g",
               who, (double)temperature);
  CDML_REQUIRE(mem_col >= B && (mem_col & 3) == 0 && lds >= mem_col + M && (lds & 3) == 0 && aligned16(S) && aligned16(mem_id),
               CDML_E_BADARG,
               "%s: S and mem_id need 16-B aligned bases, mem_col >= B (%d) and lds >= mem_col + M (%d), multiples of 4 "
               "(got mem_col %lld, lds %lld)", who, B, M, (long long)mem_col, (long long)lds);
  return CDML_OK;
}

int npm_mem_bias_check(const char *who, const float *mem_bias) {
  CDML_REQUIRE(mem_bias, CDML_E_BADARG, "%s: null pointer (mem_bias)", who);
  CDML_REQUIRE(aligned16(mem_bias), CDML_E_BADARG, "%s: mem_bias needs a 16-B aligned base", who);
  return CDML_OK;
}

int npm_w_x3_check(const char *who, int64_t mem_col, int M, const uint16_t *W, int64_t ldw, int64_t plane) {
  CDML_REQUIRE(W, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(plane >= mem_col + M && ldw >= 2 * plane + mem_col + M && (plane & 3) == 0 && (ldw & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(W) & 7) == 0,
               CDML_E_BADARG,
               "%s: W needs an 8-B aligned base, plane >= mem_col + M (%lld) and ldw >= 2 plane + mem_col + M, "
               "both multiples of 4 (got plane %lld, ldw %lld)", who, (long long)(mem_col + M), (long long)plane, (long long)ldw);
  return CDML_OK;
}

int npm_w_f32_check(const char *who, int64_t mem_col, int M, const float *W, int64_t ldw) {
  CDML_REQUIRE(W, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(ldw >= mem_col + M && (ldw & 3) == 0 && aligned16(W), CDML_E_BADARG,
               "%s: W needs a 16-B aligned base and ldw >= mem_col + M (%lld), a multiple of 4 (got %lld)", who,
               (long long)(mem_col + M), (long long)ldw);
  return CDML_OK;
}

template <int FMT, bool BIAS>
int npm_w_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                 const int32_t *mem_id, const float *mem_bias, int M, float temperature, int symmetric, const float *lse,
                 void *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  const dim3 grid((unsigned)B, (unsigned)((M + 4 * kNpThreads - 1) / (4 * kNpThreads)));
  const float scale = (symmetric ? 0.5f : 1.0f) / ((float)B * temperature);
  hipLaunchKernelGGL((k_npair_mem_w<FMT, BIAS>), grid, dim3(kNpThreads), 0, (hipStream_t)stream, S, lds, mem_col, ids, mem_id, M,
                     1.0f / temperature, lse, scale, W, ldw, plane, mem_bias);
  return check_launch(who);
}

}  // namespace
}  // namespace cdml

extern "C" size_t cdml_npair_memory_workspace(int B, int M) { return M >= 0 ? np_ws_bytes(B) : 0; }

extern "C" int cdml_npair_memory_stats(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                       const int32_t *mem_id, int M, float temperature, int symmetric, float *lse,
                                       float *stats, void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_stats", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  return np_stats_launch<true, false>("npair_memory_stats", S, lds, ids, B, nullptr, mem_col, mem_id, nullptr, M, temperature,
                                      symmetric, lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_memory_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                         const int32_t *mem_id, int M, float temperature, int symmetric, const float *lse,
                                         uint16_t *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_grad_x3", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = npm_w_x3_check("npair_memory_grad_x3", mem_col, M, W, ldw, plane)) return rc;
  return npm_w_launch<kWX3, false>("npair_memory_grad_x3", S, lds, ids, B, mem_col, mem_id, nullptr, M, temperature, symmetric,
                                   lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_memory_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                          const int32_t *mem_id, int M, float temperature, int symmetric, const float *lse,
                                          float *W, int64_t ldw, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_grad_f32", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = npm_w_f32_check("npair_memory_grad_f32", mem_col, M, W, ldw)) return rc;
  return npm_w_launch<kWF32, false>("npair_memory_grad_f32", S, lds, ids, B, mem_col, mem_id, nullptr, M, temperature,
                                    symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_logq_stats(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                            int64_t mem_col, const int32_t *mem_id, const float *mem_bias, int M,
                                            float temperature, int symmetric, float *lse, float *stats, void *workspace,
                                            size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_logq_stats", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_memory_logq_stats", bias)) return rc;
  if (int rc = npm_mem_bias_check("npair_memory_logq_stats", mem_bias)) return rc;
  return np_stats_launch<true, true>("npair_memory_logq_stats", S, lds, ids, B, bias, mem_col, mem_id, mem_bias, M, temperature,
                                     symmetric, lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_memory_logq_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                              const int32_t *mem_id, const float *mem_bias, int M, float temperature,
                                              int symmetric, const float *lse, uint16_t *W, int64_t ldw, int64_t plane,
                                              cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_logq_grad_x3", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = npm_mem_bias_check("npair_memory_logq_grad_x3", mem_bias)) return rc;
  if (int rc = npm_w_x3_check("npair_memory_logq_grad_x3", mem_col, M, W, ldw, plane)) return rc;
  return npm_w_launch<kWX3, true>("npair_memory_logq_grad_x3", S, lds, ids, B, mem_col, mem_id, mem_bias, M, temperature,
                                  symmetric, lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_memory_logq_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                               const int32_t *mem_id, const float *mem_bias, int M, float temperature,
                                               int symmetric, const float *lse, float *W, int64_t ldw, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_logq_grad_f32", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = npm_mem_bias_check("npair_memory_logq_grad_f32", mem_bias)) return rc;
  if (int rc = npm_w_f32_check("npair_memory_logq_grad_f32", mem_col, M, W, ldw)) return rc;
  return npm_w_launch<kWF32, true>("npair_memory_logq_grad_f32", S, lds, ids, B, mem_col, mem_id, mem_bias, M, temperature,
                                   symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_push(const float *P, int64_t ldp, const int32_t *ids, int B, int D, uint64_t step,
                                      const uint64_t *step_dev, int64_t start, int M, float *mem, int64_t ldm,
                                      int32_t *mem_id, uint16_t *R3, int64_t ldr, int64_t plane_r, uint16_t *T3,
                                      int64_t ldt, int64_t plane_t, cdml_stream_t stream) {
  CDML_REQUIRE(P && ids && mem && mem_id, CDML_E_BADARG, "npair_memory_push: null pointer");
  CDML_REQUIRE(B >= 1 && D >= 1 && M >= B && M % B == 0, CDML_E_BADARG,
               "npair_memory_push: needs B >= 1, D >= 1 and M a multiple of B (got B %d, D %d, M %d)", B, D, M);
  CDML_REQUIRE(ldp >= D && ldm >= D && start >= 0, CDML_E_BADARG,
               "npair_memory_push: ldp and ldm must be >= D (%d) and start >= 0 (got ldp %lld, ldm %lld, start %lld)", D,
               (long long)ldp, (long long)ldm, (long long)start);
  CDML_REQUIRE(!R3 == !T3, CDML_E_BADARG, "npair_memory_push: the plane images R3 and T3 go together");
  CDML_REQUIRE(!R3 || (plane_r >= D && ldr >= 2 * plane_r + D && plane_t >= M && ldt >= 2 * plane_t + M), CDML_E_BADARG,
               "npair_memory_push: plane images need plane_r >= D, ldr >= 2 plane_r + D, plane_t >= M and ldt >= 2 plane_t + M "
               "(got %lld, %lld, %lld, %lld)", (long long)plane_r, (long long)ldr, (long long)plane_t, (long long)ldt);
  const dim3 grid((unsigned)((D + kPushTile - 1) / kPushTile), (unsigned)((B + kPushTile - 1) / kPushTile));
  hipStream_t st = (hipStream_t)stream;
  if (R3)
    hipLaunchKernelGGL(k_npair_mem_push<true>, grid, dim3(kNpThreads), 0, st, P, ldp, ids, B, D, step, step_dev, start, M, mem,
                       ldm, mem_id, reinterpret_cast<__bf16 *>(R3), ldr, plane_r, reinterpret_cast<__bf16 *>(T3), ldt, plane_t);
  else
    hipLaunchKernelGGL(k_npair_mem_push<false>, grid, dim3(kNpThreads), 0, st, P, ldp, ids, B, D, step, step_dev, start, M, mem,
                       ldm, mem_id, (__bf16 *)nullptr, (int64_t)0, (int64_t)0, (__bf16 *)nullptr, (int64_t)0, (int64_t)0);
  return check_launch("npair_memory_push");
}

// ---- precision "bf16" (include/cdml_npair_bf16.h): W as ONE bf16 plane, the round-to-nearest-even of the fp32 value the
// _f32 entry points write -- the kWBf16 format of k_npair_w / k_npair_mem_w.  (The operand images and the ring push of that
// precision are csrc/npair_bf16.hip.) ----------------------------------------------------------------------------------

namespace cdml {
namespace {

int np_w_bf16_check(const char *who, int64_t span, const uint16_t *W, int64_t ldw) {
  CDML_REQUIRE(W, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(ldw >= span && (ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 7) == 0, CDML_E_BADARG,
               "%s: W needs an 8-B aligned base and ldw >= %lld, a multiple of 4 (got %lld)", who, (long long)span,
               (long long)ldw);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

extern "C" int cdml_npair_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                    const float *lse, uint16_t *W, int64_t ldw, cdml_stream_t stream) {
  if (int rc = np_check("npair_grad_bf16", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_w_bf16_check("npair_grad_bf16", B, W, ldw)) return rc;
  return np_w_launch<kWBf16, false>("npair_grad_bf16", S, lds, ids, B, nullptr, temperature, symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_logq_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                         float temperature, int symmetric, const float *lse, uint16_t *W, int64_t ldw,
                                         cdml_stream_t stream) {
  if (int rc = np_check("npair_logq_grad_bf16", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_logq_grad_bf16", bias)) return rc;
  if (int rc = np_w_bf16_check("npair_logq_grad_bf16", B, W, ldw)) return rc;
  return np_w_launch<kWBf16, true>("npair_logq_grad_bf16", S, lds, ids, B, bias, temperature, symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                           const int32_t *mem_id, int M, float temperature, int symmetric, const float *lse,
                                           uint16_t *W, int64_t ldw, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_grad_bf16", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = np_w_bf16_check("npair_memory_grad_bf16", mem_col + M, W, ldw)) return rc;
  return npm_w_launch<kWBf16, false>("npair_memory_grad_bf16", S, lds, ids, B, mem_col, mem_id, nullptr, M, temperature,
                                     symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_logq_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                                const int32_t *mem_id, const float *mem_bias, int M, float temperature,
                                                int symmetric, const float *lse, uint16_t *W, int64_t ldw,
                                                cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_logq_grad_bf16", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = npm_mem_bias_check("npair_memory_logq_grad_bf16", mem_bias)) return rc;
  if (int rc = np_w_bf16_check("npair_memory_logq_grad_bf16", mem_col + M, W, ldw)) return rc;
  return npm_w_launch<kWBf16, true>("npair_memory_logq_grad_bf16", S, lds, ids, B, mem_col, mem_id, mem_bias, M, temperature,
                                    symmetric, lse, W, ldw, 0, stream);
}

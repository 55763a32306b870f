// The one copy of what the N-pair chains share (csrc/npair.hip, npair_mixed.hip, npair_dp.hip, npair_bf16.hip): the online
// log-sum-exp pair, the plane split of four values, the block-level tail of the row passes, the step-scalar reduction, the
// store of four W values, the in-batch column pass and the host checks of temperature, bias vectors, workspace and W layout.
// "No atomics, every sum in a fixed order, bit-reproducible" is kept HERE: the order in which lanes, waves and chunks are
// combined is the result's bits.  Everything has internal linkage, like the kernels of the files that include it.
#pragma once
#include "common.h"
#include <math.h>

namespace cdml {
namespace {

constexpr int kNpThreads = 256;
constexpr int kNpChunk = 256;          // rows per block of the column pass
// what a W kernel stores: fp32, three exact bf16 planes, or one bf16 plane (the rounded fp32 value); the ring push: no
// images, three-plane images or one-plane images
enum : int { kWF32 = 0, kWX3 = 1, kWBf16 = 2 };

using bf4 = __attribute__((ext_vector_type(4))) __bf16;

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

// split3_bf16 (common.h) of four values
__device__ __forceinline__ void split4(const float (&w)[4], bf4 &h, bf4 &m, bf4 &l) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    __bf16 a, b, c;
    split3_bf16(w[q], a, b, c);
    h[q] = a;
    m[q] = b;
    l[q] = c;
  }
}

// The tail of a row pass of THREADS lanes: each lane's online pair (m, s) and its sums (nsum, ncnt) -> the block's (M, Sx,
// ns, nc), by a fixed butterfly within the wave and then wave by wave in wave order.  True on thread 0, which alone holds
// the result.
template <int THREADS>
__device__ __forceinline__ bool row_fold(float m, float s, float nsum, float ncnt, float &M, float &Sx, float &ns, float &nc) {
  __shared__ float sm[THREADS / kWave][4];
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
  if (threadIdx.x != 0) return false;
  M = sm[0][0], Sx = sm[0][1], ns = sm[0][2], nc = sm[0][3];
  for (int w = 1; w < THREADS / kWave; ++w) {
    lse_merge(M, Sx, sm[w][0], sm[w][1]);
    ns += sm[w][2];
    nc += sm[w][3];
  }
  return true;
}

// lse[i] and part[4 i .. 4 i + 3] = {lse_i - d, 2 - 2 S_ii, ns, nc} from thread 0's row_fold result; d = the diagonal's logit
__device__ __forceinline__ void row_store(float M, float Sx, float ns, float nc, float sii, float d, int i,
                                          float *__restrict__ lse, float *__restrict__ part) {
  const float l = M + logf(Sx);
  lse[i] = l;
  *reinterpret_cast<float4 *>(part + 4 * (int64_t)i) = make_float4(l - d, 2.f - 2.f * sii, ns, nc);
}

// The step scalars of one block of 1024 lanes from the per-row partials, in a fixed order: stats[0] = loss (with
// `symmetric` the mean of the row term and of col(i) over the rows), [1] = mean |a_i - p_i|^2, [2] = mean squared distance
// over the counted negatives, [3] = their count / den (GUARD: 0 when den is not positive)
template <bool GUARD, class ColTerm>
__device__ __forceinline__ void step_scalars(const float *__restrict__ part, int B, int symmetric, ColTerm col, float den,
                                             float *__restrict__ stats) {
  __shared__ float sm[5][1024 / kWave];
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < B; i += 1024) {
    const float4 p = *reinterpret_cast<const float4 *>(part + 4 * (int64_t)i);
    acc[0] += p.x;
    acc[1] += p.y;
    acc[2] += p.z;
    acc[3] += p.w;
    if (symmetric) acc[4] += col(i);
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
    stats[3] = (!GUARD || den > 0.f) ? t[3] / den : 0.f;
  }
}

// W[row][col .. col + n - 1] <- w[0 .. n - 1] (n = 4: vector stores; n < 4: the tail of a row) as fp32, as three exact bf16
// planes [hi | mid | lo] `plane` apart (the split of cdml_split_f32_bf16x3) or as one bf16 plane (round to nearest even)
template <int FMT>
__device__ __forceinline__ void store_w4(void *__restrict__ Wout, int64_t row, int64_t ldw, int64_t plane, int64_t col,
                                         const float (&w)[4], int n) {
  if constexpr (FMT == kWX3) {
    bf4 h, m, l;
    split4(w, h, m, l);
    __bf16 *dst = static_cast<__bf16 *>(Wout) + row * ldw + col;
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
    bf4 r;
    for (int q = 0; q < 4; ++q) r[q] = (__bf16)w[q];
    __bf16 *dst = static_cast<__bf16 *>(Wout) + row * ldw + col;
    if (n == 4)
      *reinterpret_cast<bf4 *>(dst) = r;
    else
      for (int q = 0; q < n; ++q) dst[q] = r[q];
  } else {
    float *dst = static_cast<float *>(Wout) + row * ldw + col;
    if (n == 4)
      *reinterpret_cast<float4 *>(dst) = make_float4(w[0], w[1], w[2], w[3]);
    else
      for (int q = 0; q < n; ++q) dst[q] = w[q];
  }
}

// ---- the column term over the in-batch block (symmetric): ids are IDS apart per pair, [IDS i] = id(a_i), [IDS i + 1] =
// id(p_i) (2: the pair layout; 3: the uniform sampler's triplets); NULL = every row a video of its own ----

template <int IDS>
__device__ __forceinline__ bool col_counts(const int32_t *ids, int i, int j, int idaj, int idpj) {
  if (i == j || !ids) return true;
  const int q = ids[IDS * i];
  return q != idaj && q != idpj;
}

// cm / cs [chunk][B]: the (max, sum-exp) of column j over rows chunk * kNpChunk .. + kNpChunk - 1
// BIAS: row i's logit less bias[2i] (the anchor's: one value per row, the same for every lane of the wave)
template <bool BIAS, int IDS>
__global__ void __launch_bounds__(kNpThreads)
k_npair_cols(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, float inv_t,
             float *__restrict__ cm, float *__restrict__ cs, const float *__restrict__ bias) {
  const int j = blockIdx.x * kNpThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (j >= B) return;
  const int idaj = ids ? ids[IDS * j] : 0, idpj = ids ? ids[IDS * j + 1] : 0;
  const int i0 = c * kNpChunk, i1 = min(B, i0 + kNpChunk);
  float m = -INFINITY, s = 0.f;
  for (int i = i0; i < i1; ++i) {
    if (!col_counts<IDS>(ids, i, j, idaj, idpj)) continue;
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

inline int np_chunks(int B) { return (B + kNpChunk - 1) / kNpChunk; }

// workspace floats: part [4B] | closs [B] | cm [chunks B] | cs [chunks B]
inline size_t np_ws_bytes(int B) {
  if (B < 1) return 0;
  const size_t f = (size_t)B * (5 + 2 * (size_t)np_chunks(B));
  return (f * sizeof(float) + 255) / 256 * 256;
}

// the two column launches into that workspace (closs = part + 4B): lse[B ..] and closs
template <bool BIAS, int IDS>
int np_cols_launch(const char *what_cols, const char *what_fold, const float *S, int64_t lds, const int32_t *ids, int B,
                   float inv_t, const float *bias, float *lse, float *part, hipStream_t st) {
  const int chunks = np_chunks(B);
  float *closs = part + 4 * (size_t)B, *cm = closs + B, *cs = cm + (size_t)chunks * B;
  const unsigned gx = (unsigned)((B + kNpThreads - 1) / kNpThreads);
  hipLaunchKernelGGL((k_npair_cols<BIAS, IDS>), dim3(gx, chunks), dim3(kNpThreads), 0, st, S, lds, ids, B, inv_t, cm, cs, bias);
  if (int rc = check_launch(what_cols)) return rc;
  hipLaunchKernelGGL(k_npair_col_fold<BIAS>, dim3(gx), dim3(kNpThreads), 0, st, S, lds, B, chunks, inv_t, cm, cs, lse, closs,
                     bias);
  return check_launch(what_fold);
}

// ---- host checks ----

inline bool mult4(int64_t v) { return (v & 3) == 0; }

inline int np_temperature_check(const char *who, float temperature) {
  CDML_REQUIRE(isfinite(temperature) && temperature > 0.f, CDML_E_BADARG, "%s: temperature must be finite and > 0, got %g",
               who, (double)temperature);
  return CDML_OK;
}

// a logQ bias vector (`name`: bias / mem_bias)
inline int np_bias_check(const char *who, const char *name, const float *bias) {
  CDML_REQUIRE(bias, CDML_E_BADARG, "%s: null pointer (%s)", who, name);
  CDML_REQUIRE(aligned16(bias), CDML_E_BADARG, "%s: %s needs a 16-B aligned base", who, name);
  return CDML_OK;
}

// `need` = what `fn` (the entry that sizes the workspace, with its arguments) returns
inline int np_ws_check(const char *who, const void *workspace, size_t workspace_bytes, size_t need, const char *fn) {
  CDML_REQUIRE(workspace, CDML_E_BADARG, "%s: null pointer (workspace)", who);
  CDML_REQUIRE(aligned16(workspace) && workspace_bytes >= need, CDML_E_BADARG,
               "%s: the workspace must be 16-B aligned and hold %s = %zu bytes (got %zu)", who, fn, need, workspace_bytes);
  return CDML_OK;
}

// W's layout for `span` written columns per row: fp32 (16-B base, ldw >= span), three planes (8-B base, plane >= span,
// ldw >= 2 plane + span) or one bf16 plane (8-B base, ldw >= span); leading dimension and plane multiples of 4
inline int np_w_check(const char *who, int fmt, int64_t span, const void *W, int64_t ldw, int64_t plane) {
  CDML_REQUIRE(W, CDML_E_BADARG, "%s: null pointer (W)", who);
  const bool al8 = (reinterpret_cast<uintptr_t>(W) & 7) == 0;
  if (fmt == kWX3)
    CDML_REQUIRE(plane >= span && ldw >= 2 * plane + span && mult4(plane) && mult4(ldw) && al8, CDML_E_BADARG,
                 "%s: W needs an 8-B aligned base, plane >= the column span (%lld) and ldw >= 2 plane + span, both multiples "
                 "of 4 (got plane %lld, ldw %lld)", who, (long long)span, (long long)plane, (long long)ldw);
  else
    CDML_REQUIRE(ldw >= span && mult4(ldw) && (fmt == kWF32 ? aligned16(W) : al8), CDML_E_BADARG,
                 "%s: W needs %s aligned base and ldw >= the column span (%lld), a multiple of 4 (got %lld)", who,
                 fmt == kWF32 ? "a 16-B" : "an 8-B", (long long)span, (long long)ldw);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

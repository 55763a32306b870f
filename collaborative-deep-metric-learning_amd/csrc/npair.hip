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
// Four launches, all enqueue-only, no atomics, every sum in a fixed order (the results are bit-reproducible); the building
// blocks shared with the mixed-negatives and the data-parallel chain are csrc/npair_common.h:
//   k_npair_rows      one block per anchor row: one coalesced pass over S[i][:] with an online (max, sum-exp) per lane,
//                     combined by a fixed butterfly and then wave by wave (row_fold) -> lse_i and the row's loss / stat
//                     partials
//   k_npair_cols      (npair_common.h; symmetric) a 256-row chunk x 256 columns per block, one column per lane: coalesced
//                     rows of S, online (max, sum-exp) per column and chunk
//   k_npair_col_fold  (npair_common.h) one lane per column folds the chunks in order -> lse'_j and the column's loss term
//   k_npair_stats     one block: the step scalars from the per-row partials in a fixed order (step_scalars)
//   k_npair_w<FMT>    W, four columns per lane, as three exact bf16 planes [B][hi | mid | lo] (the operand layout of the
//                     plane GEMMs, split as cdml_split_f32_bf16x3 splits), as fp32 (precision "f32") or as ONE bf16 plane,
//                     the round-to-nearest-even of that fp32 value (precision "bf16": include/cdml_npair_bf16.h)
//
// Cross-batch memory (cdml_npair_memory_*): S = A [P; Mem]^T is [B][B + M], the memory's M columns at mem_col.  The row term
// also counts slot k when mem_id[k] >= 0 is neither id(a_i) nor id(p_i); the column term stays over the in-batch block.
//   k_npair_rows<true>   the row pass going on over the memory columns (float4 / int4 per lane)
//   k_npair_mem_w<FMT>   W's memory block, c_ik exp(S_ik / t - lse_i) / (B t) (halved with `symmetric`)
//   k_npair_mem_push<FMT> the ring push of the step's positives (after the products that read the memory), fp32 rows + ids,
//                        and the slots' row and transposed operand images: none (kWF32), three planes (kWX3) or one bf16
//                        plane (kWBf16: cdml_npair_memory_push_bf16)
//
// Sampling-bias correction (logQ, Yi et al. 2019; cdml_npair_logq_* / cdml_npair_memory_logq_*): every logit that enters a
// log-sum-exp or the diagonal loses the log sampling probability of its candidate -- row term column j: S_ij / t - lq(p_j),
// memory slot k: S_ik / t - lq(mem_id[k]), column term row i: S_ij / t - lq(a_i).  The passes read it per slot, bias[2i] =
// lq(a_i), bias[2i + 1] = lq(p_i) (laid out like ids) and mem_bias[k]: the BIAS instantiations of the kernels below; the
// BIAS = false ones are the arithmetic of the uncorrected loss.  csrc/npair_logq.hip fills the vectors.
#include "npair_common.h"
#include "../../include/cdml_npair_bf16.h"
#include <math.h>

namespace cdml {
namespace {

// ids: int32[2B], 2i = id(a_i), 2i+1 = id(p_i); NULL = every row a video of its own
__device__ __forceinline__ bool row_counts(const int32_t *ids, int i, int j, int ida, int idp) {
  if (j == i || !ids) return true;
  const int q = ids[2 * j + 1];
  return q != ida && q != idp;
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
  float M, Sx, ns, nc;
  if (!row_fold<kNpThreads>(m, s, nsum, ncnt, M, Sx, ns, nc)) return;
  const float sii = row[i];
  float d;
  if constexpr (BIAS)
    d = sii * inv_t - bias[2 * i + 1];
  else
    d = sii * inv_t;
  row_store(M, Sx, ns, nc, sii, d, i, lse, part);
}

// stats[0] = loss, [1] = mean |a_i - p_i|^2, [2] = mean |a_i - p_j|^2 over the counted row-term negatives, [3] = the fraction
// of off-diagonal row-term entries that count (squared distances of unit rows: 2 - 2 S); M > 0: the memory's B M entries
// are row-term negatives too
__global__ void __launch_bounds__(1024)
k_npair_stats(const float *__restrict__ part, const float *__restrict__ closs, int B, int symmetric, int M,
              float *__restrict__ stats) {
  const float fb = (float)B;
  const float den = M ? fb * (float)(B - 1) + fb * (float)M : fb * (float)(B - 1);
  step_scalars<true>(part, B, symmetric, [&](int i) { return closs[i]; }, den, stats);
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
      c = col_counts<2>(ids, i, j, idaj, idpj) ? expf(v * inv_t - ba - lse_c[j]) : 0.f;
    else
      c = col_counts<2>(ids, i, j, idaj, idpj) ? expf(v * inv_t - lse_c[j]) : 0.f;
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
  store_w4<FMT>(Wout, i, ldw, plane, j0, w, min(4, B - j0));
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
  store_w4<FMT>(Wout, i, ldw, plane, mem_col + k0, w, 4);
}

constexpr int kPushTile = 64;

// plane p of v at d[p * plane]: the three planes of cdml_split_f32_bf16x3's split, or the one rounded plane
template <int FMT>
__device__ __forceinline__ void push_image(float v, __bf16 *d, int64_t plane) {
  if constexpr (FMT == kWX3) {
    __bf16 h, m, l;
    split3_bf16(v, h, m, l);
    d[0] = h;
    d[plane] = m;
    d[2 * plane] = l;
  } else {
    d[0] = (__bf16)v;
  }
}

// The ring push of step t = step_imm + *step_dev (when t >= start): slots s .. s + B - 1, s = ((t - start) mod (M / B)) B,
// take the B positives P[r] (fp32 rows, D columns) and their ids ids[2 r + 1].  FMT kWX3 / kWBf16: also the slots' operand
// images -- R[s + r][p * plane_r + c] and T[c][p * plane_t + s + r] = bf16 plane p of P[r][c] (three planes) or bf16(P[r][c])
// (one plane, p = 0), the transposed one through a 64 x 64 LDS tile so that both stores run along contiguous addresses.
// kWF32: rows and ids only
template <int FMT>
__global__ void __launch_bounds__(kNpThreads)
k_npair_mem_push(const float *__restrict__ P, int64_t ldp, const int32_t *__restrict__ ids, int B, int D, uint64_t step_imm,
                 const uint64_t *__restrict__ step_dev, int64_t start, int M, float *__restrict__ mem, int64_t ldm,
                 int32_t *__restrict__ mem_id, __bf16 *__restrict__ R, int64_t ldr, int64_t plane_r, __bf16 *__restrict__ T,
                 int64_t ldt, int64_t plane_t) {
  __shared__ float tile[kPushTile][kPushTile + 1];
  const uint64_t t = step_imm + (step_dev ? *step_dev : 0);
  if (t < (uint64_t)start) return;                 // (the whole grid takes the same branch: no barrier is skipped by some)
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
    if constexpr (FMT != kWF32) {
      push_image<FMT>(v, R + (s + gr) * ldr + gc, plane_r);
      tile[r][lane] = v;
    }
  }
  if constexpr (FMT != kWF32) {
    __syncthreads();
    for (int c = sub; c < kPushTile; c += kStep) {
      const int gr = r0 + lane, gc = c0 + c;
      if (gr >= B || gc >= D) continue;            // (the same rows and columns as above: every entry read was written)
      push_image<FMT>(tile[lane][c], T + (int64_t)gc * ldt + s + gr, plane_t);
    }
  }
}

int np_check(const char *who, const float *S, int64_t lds, int B, float temperature, const float *lse) {
  CDML_REQUIRE(S && lse, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(B >= 1, CDML_E_BADARG, "%s: B must be >= 1, got %d", who, B);
  if (int rc = np_temperature_check(who, temperature)) return rc;
  CDML_REQUIRE(lds >= B && mult4(lds) && aligned16(S), CDML_E_BADARG,
               "%s: S needs a 16-B aligned base and lds >= B (%d), a multiple of 4 (got %lld)", who, B, (long long)lds);
  return CDML_OK;
}

int npm_check(const char *who, const float *S, int64_t lds, int B, int64_t mem_col, const int32_t *mem_id, int M,
              float temperature, const float *lse) {
  CDML_REQUIRE(S && lse && mem_id, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(B >= 1, CDML_E_BADARG, "%s: B must be >= 1, got %d", who, B);
  CDML_REQUIRE(M >= 4 && mult4(M), CDML_E_BADARG, "%s: the memory size M must be a positive multiple of 4, got %d", who, M);
  if (int rc = np_temperature_check(who, temperature)) return rc;
  CDML_REQUIRE(mem_col >= B && mult4(mem_col) && lds >= mem_col + M && mult4(lds) && aligned16(S) && aligned16(mem_id),
               CDML_E_BADARG,
               "%s: S and mem_id need 16-B aligned bases, mem_col >= B (%d) and lds >= mem_col + M (%d), multiples of 4 "
               "(got mem_col %lld, lds %lld)", who, B, M, (long long)mem_col, (long long)lds);
  return CDML_OK;
}

// the statistics launches (rows, columns + fold with `symmetric`, step scalars); MEM: S's memory block at mem_col
template <bool MEM, bool BIAS>
int np_stats_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                    int64_t mem_col, const int32_t *mem_id, const float *mem_bias, int M, float temperature, int symmetric,
                    float *lse, float *stats, void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  CDML_REQUIRE(stats, CDML_E_BADARG, "%s: null pointer (stats)", who);
  if (int rc = np_ws_check(who, workspace, workspace_bytes, np_ws_bytes(B),
                           MEM ? "cdml_npair_memory_workspace(B, M)" : "cdml_npair_workspace(B)"))
    return rc;
  const float inv_t = 1.0f / temperature;
  float *part = static_cast<float *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_npair_rows<MEM, BIAS>), dim3(B), dim3(kNpThreads), 0, st, S, lds, ids, B, inv_t, lse, part, mem_col,
                     mem_id, M, bias, mem_bias);
  if (int rc = check_launch(MEM ? "npair_memory_stats rows" : "npair_stats rows")) return rc;
  if (symmetric)                                     // (with a memory: the in-batch block as it stands, through lds)
    if (int rc = np_cols_launch<BIAS, 2>(MEM ? "npair_memory_stats columns" : "npair_stats columns",
                                         MEM ? "npair_memory_stats column fold" : "npair_stats column fold", S, lds, ids, B,
                                         inv_t, bias, lse, part, st))
      return rc;
  hipLaunchKernelGGL(k_npair_stats, dim3(1), dim3(1024), 0, st, part, part + 4 * (size_t)B, B, symmetric ? 1 : 0, MEM ? M : 0,
                     stats);
  return check_launch(who);
}

// W's in-batch block: B columns from column 0
template <int FMT, bool BIAS>
int np_w_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, const float *bias, float temperature,
                int symmetric, const float *lse, void *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  if (int rc = np_check(who, S, lds, B, temperature, lse)) return rc;
  if (BIAS)
    if (int rc = np_bias_check(who, "bias", bias)) return rc;
  if (int rc = np_w_check(who, FMT, B, W, ldw, plane)) return rc;
  const dim3 grid((unsigned)B, (unsigned)((B + 4 * kNpThreads - 1) / (4 * kNpThreads)));
  hipLaunchKernelGGL((k_npair_w<FMT, BIAS>), grid, dim3(kNpThreads), 0, (hipStream_t)stream, S, lds, ids, B, 1.0f / temperature,
                     symmetric ? 1 : 0, lse, 1.0f / ((float)B * temperature), W, ldw, plane, bias);
  return check_launch(who);
}

// W's memory block: M columns from column mem_col
template <int FMT, bool BIAS>
int npm_w_launch(const char *who, const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                 const int32_t *mem_id, const float *mem_bias, int M, float temperature, int symmetric, const float *lse,
                 void *W, int64_t ldw, int64_t plane, cdml_stream_t stream) {
  if (int rc = npm_check(who, S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (BIAS)
    if (int rc = np_bias_check(who, "mem_bias", mem_bias)) return rc;
  if (int rc = np_w_check(who, FMT, mem_col + M, W, ldw, plane)) return rc;
  const dim3 grid((unsigned)B, (unsigned)((M + 4 * kNpThreads - 1) / (4 * kNpThreads)));
  const float scale = (symmetric ? 0.5f : 1.0f) / ((float)B * temperature);
  hipLaunchKernelGGL((k_npair_mem_w<FMT, BIAS>), grid, dim3(kNpThreads), 0, (hipStream_t)stream, S, lds, mem_col, ids, mem_id, M,
                     1.0f / temperature, lse, scale, W, ldw, plane, mem_bias);
  return check_launch(who);
}

template <int FMT>
int np_push_launch(const char *who, const float *P, int64_t ldp, const int32_t *ids, int B, int D, uint64_t step,
                   const uint64_t *step_dev, int64_t start, int M, float *mem, int64_t ldm, int32_t *mem_id, uint16_t *R,
                   int64_t ldr, int64_t plane_r, uint16_t *T, int64_t ldt, int64_t plane_t, cdml_stream_t stream) {
  const dim3 grid((unsigned)((D + kPushTile - 1) / kPushTile), (unsigned)((B + kPushTile - 1) / kPushTile));
  hipLaunchKernelGGL(k_npair_mem_push<FMT>, grid, dim3(kNpThreads), 0, (hipStream_t)stream, P, ldp, ids, B, D, step, step_dev,
                     start, M, mem, ldm, mem_id, reinterpret_cast<__bf16 *>(R), ldr, plane_r, reinterpret_cast<__bf16 *>(T), ldt,
                     plane_t);
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
  return np_w_launch<kWX3, false>("npair_grad_x3", S, lds, ids, B, nullptr, temperature, symmetric, lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                   const float *lse, float *W, int64_t ldw, cdml_stream_t stream) {
  return np_w_launch<kWF32, false>("npair_grad_f32", S, lds, ids, B, nullptr, temperature, symmetric, lse, W, ldw, 0, stream);
}

// ---- the sampling-bias (logQ) corrected loss: bias[2B] per row as ids, laid out by csrc/npair_logq.hip ------------------

extern "C" int cdml_npair_logq_stats(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                     float temperature, int symmetric, float *lse, float *stats, void *workspace,
                                     size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = np_check("npair_logq_stats", S, lds, B, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_logq_stats", "bias", bias)) return rc;
  return np_stats_launch<false, true>("npair_logq_stats", S, lds, ids, B, bias, 0, nullptr, nullptr, 0, temperature, symmetric,
                                      lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_logq_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                       float temperature, int symmetric, const float *lse, uint16_t *W, int64_t ldw,
                                       int64_t plane, cdml_stream_t stream) {
  return np_w_launch<kWX3, true>("npair_logq_grad_x3", S, lds, ids, B, bias, temperature, symmetric, lse, W, ldw, plane,
                                 stream);
}

extern "C" int cdml_npair_logq_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                        float temperature, int symmetric, const float *lse, float *W, int64_t ldw,
                                        cdml_stream_t stream) {
  return np_w_launch<kWF32, true>("npair_logq_grad_f32", S, lds, ids, B, bias, temperature, symmetric, lse, W, ldw, 0, stream);
}

// ---- cross-batch memory (XBM, Wang et al. 2020): a ring of M earlier positives as extra row-term columns of S ----------

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
  return npm_w_launch<kWX3, false>("npair_memory_grad_x3", S, lds, ids, B, mem_col, mem_id, nullptr, M, temperature, symmetric,
                                   lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_memory_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                          const int32_t *mem_id, int M, float temperature, int symmetric, const float *lse,
                                          float *W, int64_t ldw, cdml_stream_t stream) {
  return npm_w_launch<kWF32, false>("npair_memory_grad_f32", S, lds, ids, B, mem_col, mem_id, nullptr, M, temperature,
                                    symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_logq_stats(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                            int64_t mem_col, const int32_t *mem_id, const float *mem_bias, int M,
                                            float temperature, int symmetric, float *lse, float *stats, void *workspace,
                                            size_t workspace_bytes, cdml_stream_t stream) {
  if (int rc = npm_check("npair_memory_logq_stats", S, lds, B, mem_col, mem_id, M, temperature, lse)) return rc;
  if (int rc = np_bias_check("npair_memory_logq_stats", "bias", bias)) return rc;
  if (int rc = np_bias_check("npair_memory_logq_stats", "mem_bias", mem_bias)) return rc;
  return np_stats_launch<true, true>("npair_memory_logq_stats", S, lds, ids, B, bias, mem_col, mem_id, mem_bias, M, temperature,
                                     symmetric, lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int cdml_npair_memory_logq_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                              const int32_t *mem_id, const float *mem_bias, int M, float temperature,
                                              int symmetric, const float *lse, uint16_t *W, int64_t ldw, int64_t plane,
                                              cdml_stream_t stream) {
  return npm_w_launch<kWX3, true>("npair_memory_logq_grad_x3", S, lds, ids, B, mem_col, mem_id, mem_bias, M, temperature,
                                  symmetric, lse, W, ldw, plane, stream);
}

extern "C" int cdml_npair_memory_logq_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                               const int32_t *mem_id, const float *mem_bias, int M, float temperature,
                                               int symmetric, const float *lse, float *W, int64_t ldw, cdml_stream_t stream) {
  return npm_w_launch<kWF32, true>("npair_memory_logq_grad_f32", S, lds, ids, B, mem_col, mem_id, mem_bias, M, temperature,
                                   symmetric, lse, W, ldw, 0, stream);
}

// the ring push: rows + ids, with the slots' three-plane images when R3 / T3 are given (precision f32x3)
extern "C" int cdml_npair_memory_push(const float *P, int64_t ldp, const int32_t *ids, int B, int D, uint64_t step,
                                      const uint64_t *step_dev, int64_t start, int M, float *mem, int64_t ldm,
                                      int32_t *mem_id, uint16_t *R3, int64_t ldr, int64_t plane_r, uint16_t *T3,
                                      int64_t ldt, int64_t plane_t, cdml_stream_t stream) {
  const char *who = "npair_memory_push";
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
  if (R3)
    return np_push_launch<kWX3>(who, P, ldp, ids, B, D, step, step_dev, start, M, mem, ldm, mem_id, R3, ldr, plane_r, T3, ldt,
                                plane_t, stream);
  return np_push_launch<kWF32>(who, P, ldp, ids, B, D, step, step_dev, start, M, mem, ldm, mem_id, nullptr, 0, 0, nullptr, 0, 0,
                               stream);
}

// ---- precision "bf16" (include/cdml_npair_bf16.h): W as ONE bf16 plane, the round-to-nearest-even of the fp32 value the
// _f32 entry points write -- the kWBf16 format of store_w4 -- and the ring push with one-plane slot images.  (The operand
// images of that precision are csrc/npair_bf16.hip.) ----------------------------------------------------------------------

extern "C" int cdml_npair_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                                    const float *lse, uint16_t *W, int64_t ldw, cdml_stream_t stream) {
  return np_w_launch<kWBf16, false>("npair_grad_bf16", S, lds, ids, B, nullptr, temperature, symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_logq_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias,
                                         float temperature, int symmetric, const float *lse, uint16_t *W, int64_t ldw,
                                         cdml_stream_t stream) {
  return np_w_launch<kWBf16, true>("npair_logq_grad_bf16", S, lds, ids, B, bias, temperature, symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                           const int32_t *mem_id, int M, float temperature, int symmetric, const float *lse,
                                           uint16_t *W, int64_t ldw, cdml_stream_t stream) {
  return npm_w_launch<kWBf16, false>("npair_memory_grad_bf16", S, lds, ids, B, mem_col, mem_id, nullptr, M, temperature,
                                     symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_logq_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                                const int32_t *mem_id, const float *mem_bias, int M, float temperature,
                                                int symmetric, const float *lse, uint16_t *W, int64_t ldw,
                                                cdml_stream_t stream) {
  return npm_w_launch<kWBf16, true>("npair_memory_logq_grad_bf16", S, lds, ids, B, mem_col, mem_id, mem_bias, M, temperature,
                                    symmetric, lse, W, ldw, 0, stream);
}

extern "C" int cdml_npair_memory_push_bf16(const float *P, int64_t ldp, const int32_t *ids, int B, int D, uint64_t step,
                                           const uint64_t *step_dev, int64_t start, int M, float *mem, int64_t ldm,
                                           int32_t *mem_id, uint16_t *R, int64_t ldr, uint16_t *T, int64_t ldt,
                                           cdml_stream_t stream) {
  CDML_REQUIRE(P && ids && mem && mem_id && R && T, CDML_E_BADARG, "npair_memory_push_bf16: null pointer");
  CDML_REQUIRE(B >= 1 && D >= 1 && M >= B && M % B == 0, CDML_E_BADARG,
               "npair_memory_push_bf16: needs B >= 1, D >= 1 and M a multiple of B (got B %d, D %d, M %d)", B, D, M);
  CDML_REQUIRE(ldp >= D && ldm >= D && ldr >= D && ldt >= M && start >= 0, CDML_E_BADARG,
               "npair_memory_push_bf16: ldp, ldm and ldr must be >= D (%d), ldt >= M (%d) and start >= 0 (got ldp %lld, ldm "
               "%lld, ldr %lld, ldt %lld, start %lld)", D, M, (long long)ldp, (long long)ldm, (long long)ldr, (long long)ldt,
               (long long)start);
  return np_push_launch<kWBf16>("npair_memory_push_bf16", P, ldp, ids, B, D, step, step_dev, start, M, mem, ldm, mem_id, R, ldr,
                                0, T, ldt, 0, stream);
}

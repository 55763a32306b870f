// Data-parallel multi-class N-pair loss (include/cdml_npair_dp.h): W ranks of B pairs, ONE softmax over the G = W B global
// pairs.  A rank holds the row block S_r = A_r P_all^T [B][G] of the global score matrix (its anchors against every rank's
// positives, gathered); local row i is the global pair g = col0 + i, whose diagonal sits at column g.  The rules and the
// arithmetic are csrc/npair.hip's on the global batch (ids_all laid out like its ids, over G pairs):
//
//   k_npdp_rows       one block per local row: one pass over S[i][0 .. G), four columns per lane (one 16-B load of S, two of
//                     the ids), online (max, sum-exp) per lane, fixed butterfly, then wave by wave -> lse_row_i and the
//                     row's loss / stat partials (k_npair_rows' layout)
//   k_npdp_cols       (symmetric) a 256-row chunk x 256 columns per block, one column per lane over ALL G columns
//   k_npdp_colpart    one lane per column folds the chunks in order -> colpart[j] = (max, sum-exp) over this rank's rows;
//                     (-inf, 0) when no local row counts
//   k_npdp_col_fold   one lane per column folds the gathered partials of ranks 0 .. W - 1 in that order -> lse_col[j]: the
//                     same bits on every rank (lse_merge never forms -inf - -inf)
//   k_npdp_stats      one block: this rank's step scalars in a fixed order; the column term of the columns it owns reads
//                     its own row diagonals
//   k_npdp_w<FMT>     W_r [B][G], four columns per lane, as three exact bf16 planes or fp32; scale 1 / (B t): the LOCAL mean,
//                     the gradient average over the ranks makes it the global one
//   k_npdp_pos_fold   de[2i + 1] = the received partial positive gradients summed in rank order
// All enqueue-only, no atomics, every sum in a fixed order; the log-sum-exp pair, the row pass's tail (row_fold), the step
// scalars (step_scalars), the W store (store_w4) and the common host checks are csrc/npair_common.h.
#include "npair_common.h"
#include "../../include/cdml_npair_dp.h"
#include <math.h>

namespace cdml {
namespace {

constexpr int kDpThreads = 256;
constexpr int kDpChunk = 256;          // rows per block of the column pass

// column j (positive id q) counts for the row of global pair g (ids ida, idp)
__device__ __forceinline__ bool dp_row_counts(bool ids, int g, int j, int q, int ida, int idp) {
  return j == g || !ids || (q != ida && q != idp);
}

// the row of global pair g (anchor id ida) counts for column j (ids idaj, idpj)
__device__ __forceinline__ bool dp_col_counts(bool ids, int g, int j, int ida, int idaj, int idpj) {
  return j == g || !ids || (ida != idaj && ida != idpj);
}

__device__ __forceinline__ void dp_row_add(bool ids, int g, int j, float v, int q, int ida, int idp, float inv_t, float &m,
                                           float &s, float &nsum, float &ncnt) {
  if (!dp_row_counts(ids, g, j, q, ida, idp)) return;
  lse_add(m, s, v * inv_t);
  if (j != g) {
    nsum += 2.f - 2.f * v;
    ncnt += 1.f;
  }
}

// part[4 i .. 4 i + 3] = {lse_i - S_ii / t, 2 - 2 S_ii, sum over the counted j != g of 2 - 2 S_ij, their count}, S_ii =
// S[i][col0 + i]
__global__ void __launch_bounds__(kDpThreads)
k_npdp_rows(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int G, int col0, float inv_t,
            float *__restrict__ lse, float *__restrict__ part) {
  const int i = blockIdx.x, g = col0 + i;
  const float *row = S + (int64_t)i * lds;
  const bool has = ids != nullptr;
  const int ida = has ? ids[2 * g] : 0, idp = has ? ids[2 * g + 1] : 0;
  float m = -INFINITY, s = 0.f, nsum = 0.f, ncnt = 0.f;
  for (int j = 4 * threadIdx.x; j < G; j += 4 * kDpThreads) {
    const float4 v = *reinterpret_cast<const float4 *>(row + j);
    int4 q0 = make_int4(0, 0, 0, 0), q1 = q0;         // the four columns' slots 2j .. 2j + 7: positives odd
    if (has) {
      q0 = *reinterpret_cast<const int4 *>(ids + 2 * (int64_t)j);
      q1 = *reinterpret_cast<const int4 *>(ids + 2 * (int64_t)j + 4);
    }
    dp_row_add(has, g, j, v.x, q0.y, ida, idp, inv_t, m, s, nsum, ncnt);
    dp_row_add(has, g, j + 1, v.y, q0.w, ida, idp, inv_t, m, s, nsum, ncnt);
    dp_row_add(has, g, j + 2, v.z, q1.y, ida, idp, inv_t, m, s, nsum, ncnt);
    dp_row_add(has, g, j + 3, v.w, q1.w, ida, idp, inv_t, m, s, nsum, ncnt);
  }
  float M, Sx, ns, nc;
  if (!row_fold<kDpThreads>(m, s, nsum, ncnt, M, Sx, ns, nc)) return;
  const float sii = row[g];
  row_store(M, Sx, ns, nc, sii, sii * inv_t, i, lse, part);
}

// cm / cs [chunk][G]: the (max, sum-exp) of column j over the local rows chunk * kDpChunk .. + kDpChunk - 1 that count
// (the row's anchor id: one value per row, the same for every lane of the wave)
__global__ void __launch_bounds__(kDpThreads)
k_npdp_cols(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int B, int G, int col0, float inv_t,
            float *__restrict__ cm, float *__restrict__ cs) {
  const int j = blockIdx.x * kDpThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (j >= G) return;
  const bool has = ids != nullptr;
  const int idaj = has ? ids[2 * j] : 0, idpj = has ? ids[2 * j + 1] : 0;
  const int i0 = c * kDpChunk, i1 = min(B, i0 + kDpChunk);
  float m = -INFINITY, s = 0.f;
  for (int i = i0; i < i1; ++i) {
    const int g = col0 + i;
    if (!dp_col_counts(has, g, j, has ? ids[2 * g] : 0, idaj, idpj)) continue;
    lse_add(m, s, S[(int64_t)i * lds + j] * inv_t);
  }
  cm[(int64_t)c * G + j] = m;
  cs[(int64_t)c * G + j] = s;
}

// colpart[j] = (max, sum-exp) of column j over this rank's rows: the chunks folded in order; nothing counted: (-inf, 0)
__global__ void __launch_bounds__(kDpThreads)
k_npdp_colpart(const float *__restrict__ cm, const float *__restrict__ cs, int G, int chunks, float *__restrict__ colpart) {
  const int j = blockIdx.x * kDpThreads + threadIdx.x;
  if (j >= G) return;
  float m = -INFINITY, s = 0.f;
  for (int c = 0; c < chunks; ++c) lse_merge(m, s, cm[(int64_t)c * G + j], cs[(int64_t)c * G + j]);
  *reinterpret_cast<float2 *>(colpart + 2 * (int64_t)j) = make_float2(m, s);
}

// lse_col[j] from colpart_all [world][G][2], ranks 0 .. world - 1 in that order
__global__ void __launch_bounds__(kDpThreads)
k_npdp_col_fold(const float *__restrict__ colpart_all, int world, int G, float *__restrict__ lse_col) {
  const int j = blockIdx.x * kDpThreads + threadIdx.x;
  if (j >= G) return;
  float m = -INFINITY, s = 0.f;
  for (int r = 0; r < world; ++r) {
    const float2 p = *reinterpret_cast<const float2 *>(colpart_all + 2 * ((int64_t)r * G + j));
    lse_merge(m, s, p.x, p.y);
  }
  lse_col[j] = m + logf(s);                            // (nobody counted: -inf + -inf = -inf, not a NaN)
}

// stats[0] = this rank's share of the loss, [1] = mean |a_i - p_i|^2, [2] = mean |a_i - p_j|^2 over the local rows' counted
// negatives, [3] = their fraction of B (G - 1); the column term of the owned column col0 + i: lse_col[col0 + i] - S_ii / t
__global__ void __launch_bounds__(1024)
k_npdp_stats(const float *__restrict__ S, int64_t lds, const float *__restrict__ part, const float *__restrict__ lse_col, int B,
             int G, int col0, float inv_t, int symmetric, float *__restrict__ stats) {
  step_scalars<true>(part, B, symmetric, [&](int i) { return lse_col[col0 + i] - S[(int64_t)i * lds + col0 + i] * inv_t; },
                     (float)B * (float)(G - 1), stats);
}

__device__ __forceinline__ float dp_w(bool ids, int g, int j, int ida, int idp, int idaj, int idpj, float v, float inv_t,
                                      float lse_r, float lse_c, int symmetric, float scale) {
  float r = dp_row_counts(ids, g, j, idpj, ida, idp) ? expf(v * inv_t - lse_r) : 0.f;
  if (j == g) r -= 1.f;
  if (symmetric) {
    float c = dp_col_counts(ids, g, j, ida, idaj, idpj) ? expf(v * inv_t - lse_c) : 0.f;
    if (j == g) c -= 1.f;
    r = 0.5f * (r + c);
  }
  return r * scale;
}

// local row i = blockIdx.x, columns 4 (blockIdx.y * kDpThreads + threadIdx.x) .. + 3 (G a multiple of 4)
template <int FMT>
__global__ void __launch_bounds__(kDpThreads)
k_npdp_w(const float *__restrict__ S, int64_t lds, const int32_t *__restrict__ ids, int G, int col0, float inv_t, int symmetric,
         const float *__restrict__ lse_row, const float *__restrict__ lse_col, float scale, void *__restrict__ Wout,
         int64_t ldw, int64_t plane) {
  const int i = blockIdx.x, g = col0 + i;
  const int j0 = (blockIdx.y * kDpThreads + threadIdx.x) * 4;
  if (j0 >= G) return;
  const bool has = ids != nullptr;
  const int ida = has ? ids[2 * g] : 0, idp = has ? ids[2 * g + 1] : 0;
  const float lr = lse_row[i];
  const float4 v = *reinterpret_cast<const float4 *>(S + (int64_t)i * lds + j0);
  int4 q0 = make_int4(0, 0, 0, 0), q1 = q0;           // (a, p) of columns j0, j0 + 1 | j0 + 2, j0 + 3
  if (has) {
    q0 = *reinterpret_cast<const int4 *>(ids + 2 * (int64_t)j0);
    q1 = *reinterpret_cast<const int4 *>(ids + 2 * (int64_t)j0 + 4);
  }
  float4 lc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (symmetric) lc = *reinterpret_cast<const float4 *>(lse_col + j0);
  const float w[4] = {dp_w(has, g, j0, ida, idp, q0.x, q0.y, v.x, inv_t, lr, lc.x, symmetric, scale),
                      dp_w(has, g, j0 + 1, ida, idp, q0.z, q0.w, v.y, inv_t, lr, lc.y, symmetric, scale),
                      dp_w(has, g, j0 + 2, ida, idp, q1.x, q1.y, v.z, inv_t, lr, lc.z, symmetric, scale),
                      dp_w(has, g, j0 + 3, ida, idp, q1.z, q1.w, v.w, inv_t, lr, lc.w, symmetric, scale)};
  store_w4<FMT>(Wout, i, ldw, plane, j0, w, 4);
}

// one lane per four columns of one positive's row: recv[0][i] + recv[1][i] + ... in that order -> de[2i + 1]
__global__ void __launch_bounds__(kDpThreads)
k_npdp_pos_fold(const float *__restrict__ recv, int64_t ldr, int world, int B, int D4, float *__restrict__ de, int64_t ldde) {
  const int64_t k = (int64_t)blockIdx.x * kDpThreads + threadIdx.x;
  if (k >= (int64_t)B * D4) return;
  const int i = (int)(k / D4), c = (int)(k - (int64_t)i * D4) * 4;
  float4 acc = *reinterpret_cast<const float4 *>(recv + (int64_t)i * ldr + c);
  for (int r = 1; r < world; ++r) {
    const float4 v = *reinterpret_cast<const float4 *>(recv + ((int64_t)r * B + i) * ldr + c);
    acc.x += v.x;
    acc.y += v.y;
    acc.z += v.z;
    acc.w += v.w;
  }
  *reinterpret_cast<float4 *>(de + (int64_t)(2 * i + 1) * ldde + c) = acc;
}

int dp_chunks(int B) { return (B + kDpChunk - 1) / kDpChunk; }

// workspace floats: part [4B] | cm [chunks G] | cs [chunks G]
size_t dp_ws_bytes(int B, int G) {
  if (B < 1 || G < B) return 0;
  const size_t f = 4 * (size_t)B + 2 * (size_t)dp_chunks(B) * (size_t)G;
  return (f * sizeof(float) + 255) / 256 * 256;
}

int dp_check(const char *who, const float *S, int64_t lds, int B, int G, int col0, float temperature) {
  CDML_REQUIRE(S, CDML_E_BADARG, "%s: null pointer (S)", who);
  CDML_REQUIRE(B >= 1 && G >= B && (G & 3) == 0, CDML_E_BADARG,
               "%s: needs B >= 1 and G >= B, G a multiple of 4 (got B %d, G %d)", who, B, G);
  CDML_REQUIRE(col0 >= 0 && (col0 & 3) == 0 && (int64_t)col0 + B <= G, CDML_E_BADARG,
               "%s: col0 must be a multiple of 4 with 0 <= col0 and col0 + B <= G (got col0 %d, B %d, G %d)", who, col0, B, G);
  if (int rc = np_temperature_check(who, temperature)) return rc;
  CDML_REQUIRE(lds >= G && (lds & 3) == 0 && aligned16(S), CDML_E_BADARG,
               "%s: S needs a 16-B aligned base and lds >= G (%d), a multiple of 4 (got %lld)", who, G, (long long)lds);
  return CDML_OK;
}

int dp_ws_check(const char *who, int B, int G, const void *workspace, size_t workspace_bytes) {
  return np_ws_check(who, workspace, workspace_bytes, dp_ws_bytes(B, G), "cdml_npair_dp_workspace(B, G)");
}

int dp_grad_check(const char *who, const int32_t *ids_all, int symmetric, const float *lse_row, const float *lse_col) {
  CDML_REQUIRE(lse_row && (!symmetric || lse_col), CDML_E_BADARG, "%s: null pointer (lse_row / lse_col)", who);
  CDML_REQUIRE(aligned16(ids_all) && aligned16(lse_col), CDML_E_BADARG, "%s: ids_all and lse_col need 16-B aligned bases", who);
  return CDML_OK;
}

template <int FMT>
int dp_w_launch(const char *who, const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0, float temperature,
                int symmetric, const float *lse_row, const float *lse_col, void *W, int64_t ldw, int64_t plane,
                cdml_stream_t stream) {
  if (int rc = dp_check(who, S, lds, B, G, col0, temperature)) return rc;
  if (int rc = dp_grad_check(who, ids_all, symmetric, lse_row, lse_col)) return rc;
  if (int rc = np_w_check(who, FMT, G, W, ldw, plane)) return rc;
  const dim3 grid((unsigned)B, (unsigned)((G + 4 * kDpThreads - 1) / (4 * kDpThreads)));
  hipLaunchKernelGGL(k_npdp_w<FMT>, grid, dim3(kDpThreads), 0, (hipStream_t)stream, S, lds, ids_all, G, col0, 1.0f / temperature,
                     symmetric ? 1 : 0, lse_row, lse_col, 1.0f / ((float)B * temperature), W, ldw, plane);
  return check_launch(who);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" size_t cdml_npair_dp_workspace(int B, int G) { return dp_ws_bytes(B, G); }

extern "C" int cdml_npair_dp_local_stats(const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0,
                                         float temperature, int symmetric, float *lse_row, float *colpart, void *workspace,
                                         size_t workspace_bytes, cdml_stream_t stream) {
  const char *who = "npair_dp_local_stats";
  if (int rc = dp_check(who, S, lds, B, G, col0, temperature)) return rc;
  CDML_REQUIRE(lse_row && (!symmetric || colpart), CDML_E_BADARG, "%s: null pointer (lse_row / colpart)", who);
  CDML_REQUIRE(aligned16(ids_all) && aligned16(colpart), CDML_E_BADARG, "%s: ids_all and colpart need 16-B aligned bases", who);
  if (int rc = dp_ws_check(who, B, G, workspace, workspace_bytes)) return rc;
  const float inv_t = 1.0f / temperature;
  const int chunks = dp_chunks(B);
  float *part = static_cast<float *>(workspace), *cm = part + 4 * (size_t)B, *cs = cm + (size_t)chunks * G;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_npdp_rows, dim3(B), dim3(kDpThreads), 0, st, S, lds, ids_all, G, col0, inv_t, lse_row, part);
  if (int rc = check_launch("npair_dp_local_stats rows")) return rc;
  if (symmetric) {
    const unsigned gx = (unsigned)((G + kDpThreads - 1) / kDpThreads);
    hipLaunchKernelGGL(k_npdp_cols, dim3(gx, chunks), dim3(kDpThreads), 0, st, S, lds, ids_all, B, G, col0, inv_t, cm, cs);
    if (int rc = check_launch("npair_dp_local_stats columns")) return rc;
    hipLaunchKernelGGL(k_npdp_colpart, dim3(gx), dim3(kDpThreads), 0, st, cm, cs, G, chunks, colpart);
  }
  return check_launch(who);
}

extern "C" int cdml_npair_dp_col_fold(const float *colpart_all, int world, int G, float *lse_col, cdml_stream_t stream) {
  const char *who = "npair_dp_col_fold";
  CDML_REQUIRE(colpart_all && lse_col, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(world >= 1 && G >= 1, CDML_E_BADARG, "%s: needs world >= 1 and G >= 1 (got %d, %d)", who, world, G);
  CDML_REQUIRE(aligned16(colpart_all), CDML_E_BADARG, "%s: colpart_all needs a 16-B aligned base", who);
  hipLaunchKernelGGL(k_npdp_col_fold, dim3((unsigned)((G + kDpThreads - 1) / kDpThreads)), dim3(kDpThreads), 0,
                     (hipStream_t)stream, colpart_all, world, G, lse_col);
  return check_launch(who);
}

extern "C" int cdml_npair_dp_stats(const float *S, int64_t lds, int B, int G, int col0, float temperature, int symmetric,
                                   const float *lse_col, float *stats, const void *workspace, size_t workspace_bytes,
                                   cdml_stream_t stream) {
  const char *who = "npair_dp_stats";
  if (int rc = dp_check(who, S, lds, B, G, col0, temperature)) return rc;
  CDML_REQUIRE(stats && (!symmetric || lse_col), CDML_E_BADARG, "%s: null pointer (stats / lse_col)", who);
  if (int rc = dp_ws_check(who, B, G, workspace, workspace_bytes)) return rc;
  hipLaunchKernelGGL(k_npdp_stats, dim3(1), dim3(1024), 0, (hipStream_t)stream, S, lds, static_cast<const float *>(workspace),
                     lse_col, B, G, col0, 1.0f / temperature, symmetric ? 1 : 0, stats);
  return check_launch(who);
}

extern "C" int cdml_npair_dp_grad_x3(const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0,
                                     float temperature, int symmetric, const float *lse_row, const float *lse_col, uint16_t *W,
                                     int64_t ldw, int64_t plane, cdml_stream_t stream) {
  return dp_w_launch<kWX3>("npair_dp_grad_x3", S, lds, ids_all, B, G, col0, temperature, symmetric, lse_row, lse_col, W, ldw,
                           plane, stream);
}

extern "C" int cdml_npair_dp_grad_f32(const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0,
                                      float temperature, int symmetric, const float *lse_row, const float *lse_col, float *W,
                                      int64_t ldw, cdml_stream_t stream) {
  return dp_w_launch<kWF32>("npair_dp_grad_f32", S, lds, ids_all, B, G, col0, temperature, symmetric, lse_row, lse_col, W, ldw, 0,
                            stream);
}

extern "C" int cdml_npair_dp_pos_fold(const float *recv, int64_t ldr, int world, int B, int D, float *de, int64_t ldde,
                                      cdml_stream_t stream) {
  const char *who = "npair_dp_pos_fold";
  CDML_REQUIRE(recv && de, CDML_E_BADARG, "%s: null pointer", who);
  CDML_REQUIRE(world >= 1 && B >= 1 && D >= 4 && (D & 3) == 0, CDML_E_BADARG,
               "%s: needs world >= 1, B >= 1 and D a positive multiple of 4 (got %d, %d, %d)", who, world, B, D);
  CDML_REQUIRE(ldr >= D && ldde >= D && (ldr & 3) == 0 && (ldde & 3) == 0 && aligned16(recv) && aligned16(de), CDML_E_BADARG,
               "%s: recv and de need 16-B aligned bases and leading dimensions >= D (%d), multiples of 4 (got %lld, %lld)", who,
               D, (long long)ldr, (long long)ldde);
  const int64_t n = (int64_t)B * (D / 4);
  hipLaunchKernelGGL(k_npdp_pos_fold, dim3((unsigned)((n + kDpThreads - 1) / kDpThreads)), dim3(kDpThreads), 0,
                     (hipStream_t)stream, recv, ldr, world, B, D / 4, de, ldde);
  return check_launch(who);
}

// Inverted-file (IVF-Flat) index of the kNN (include/cdml_ivf.h; build-defined: the reference's faiss_knn.calc_knn builds
// an approximate HNSW index, knn.py's search is brute force).  k-means cuts the catalogue into nlist lists; a query is
// scored only against the rows of its nprobe nearest lists.  The coarse steps (rows or queries against the centroids)
// are the exact search of knn.py; this file holds what that search has no use for:
//
//   k_ivf_centroid_sum  Lloyd's update: one block per (list, 64-column slab), the list's column means in an order fixed by
//                       the list's length alone (wave w of four takes rows w, w + 4, ...; partials fold in wave order).
//   k_ivf_scan          the grouped (ragged) score product on v_mfma_f32_32x32x2_f32.  A slot is one (query, probed list)
//                       pair; slots are sorted by list, so list c's slots form a dense block S_c [nq_c][ld_c] in one ragged
//                       score buffer.  Work item = (list, 128-slot tile, 128-row tile) from a tile table; 2 x 2 waves of
//                       64 x 64, K-tiles of 32 through LDS; the query rows are fetched through slot_query, the only
//                       difference from a plain NT product.  Plain 64-bit global addressing throughout.
//   k_ivf_merge         one wave per query: k_knn_merge's list keeper (csrc/knn.hip: 256-entry LDS buffer, bitonic
//                       compaction, key (d, id), the clamp that keeps a NaN) over the query's nprobe score segments.
// The list-keeping device functions are a copy of knn.hip's (that file's kernels keep their instructions).
#include "common.h"
#include "../../include/cdml_ivf.h"

namespace cdml {
namespace {

constexpr int kListCap = CDML_KNN_LIST;   // entries kept per query (k <= kListCap)
constexpr int kBuf = 2 * kListCap;        // LDS buffer per wave
constexpr int kRowsPerBlock = 4;          // one wave per query row
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- Lloyd's update ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ivf_centroid_sum(const float *__restrict__ x, int64_t ldx, const int32_t *__restrict__ order,
                   const int32_t *__restrict__ list_start, int D, float *__restrict__ cent, int64_t ldc) {
  __shared__ float part[4][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x, col = blockIdx.y * 64 + lane;
  const int b = list_start[c], L = list_start[c + 1] - b;
  if (L <= 0) return;                          // block-uniform: an empty list keeps its centroid
  float s = 0.f;
  if (col < D)
    for (int r = w; r < L; r += 4) s += x[(int64_t)order[b + r] * ldx + col];
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && col < D)
    cent[(int64_t)c * ldc + col] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (float)L;
}

// ---- the grouped score product ---------------------------------------------------------------------------------------
constexpr int kTile = 128;                // slots x rows per work item
constexpr int kBK = 32;                   // K-tile depth
constexpr int kLdS = kBK + 4;             // LDS row stride in floats: 16-B aligned rows, 144 B apart

__global__ void __launch_bounds__(256)
k_ivf_scan(const float *__restrict__ Q, int64_t ldq, int n_queries, const int32_t *__restrict__ slot_query,
           const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off, const float *__restrict__ rows,
           int64_t ldr, const int32_t *__restrict__ list_start, int Dp, const int4 *__restrict__ tiles,
           float *__restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float sA[kTile * kLdS];
  __shared__ __attribute__((aligned(16))) float sB[kTile * kLdS];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;

  const int4 tl = tiles[blockIdx.x];
  const int c = tl.x, i0 = tl.y, j0 = tl.z;
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const int r0 = list_start[c], len = list_start[c + 1] - r0;
  if (i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len) return;    // block-uniform, before any barrier
  const int ld_c = (len + 3) & ~3;

  // loader: thread t moves chunk t & 7 (16 B) of tile rows (t >> 3) + 32 j; a row past the end is the last valid one
  const int chunk = t & 7, lrow = t >> 3;
  const float *pa[4], *pb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ra = min(i0 + lrow + 32 * j, nq_c - 1);
    const int q = min(max(slot_query[s0 + ra], 0), n_queries - 1);
    pa[j] = Q + (int64_t)q * ldq + 4 * chunk;
    const int rb = min(j0 + lrow + 32 * j, len - 1);
    pb[j] = rows + (int64_t)(r0 + rb) * ldr + 4 * chunk;
  }
  f32x4 ga[4], gb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ga[j] = *reinterpret_cast<const f32x4 *>(pa[j]);
    gb[j] = *reinterpret_cast<const f32x4 *>(pb[j]);
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int n_ktiles = Dp / kBK;
  for (int kt = 0; kt < n_ktiles; ++kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<f32x4 *>(sA + (lrow + 32 * j) * kLdS + 4 * chunk) = ga[j];
      *reinterpret_cast<f32x4 *>(sB + (lrow + 32 * j) * kLdS + 4 * chunk) = gb[j];
    }
    __syncthreads();
    if (kt + 1 < n_ktiles) {                   // the next K-tile's rows travel under this one's MFMAs
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ga[j] = *reinterpret_cast<const f32x4 *>(pa[j] + (kt + 1) * kBK);
        gb[j] = *reinterpret_cast<const f32x4 *>(pb[j] + (kt + 1) * kBK);
      }
    }
    // k-group grp = 8 k values; lane half h owns 4 of them: MFMA u multiplies k = 8 grp + u and 8 grp + 4 + u
#pragma unroll
    for (int grp = 0; grp < kBK / 8; ++grp) {
      f32x4 fa[2], fb[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        fa[mi] = *reinterpret_cast<const f32x4 *>(sA + (wm * 64 + mi * 32 + l31) * kLdS + 8 * grp + 4 * h);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        fb[ni] = *reinterpret_cast<const f32x4 *>(sB + (wn * 64 + ni * 32 + l31) * kLdS + 8 * grp + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][u], fb[ni][u], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();                           // the stage is free again
  }

  // C/D layout: column = lane & 31 (a list row), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (a slot)
  float *blk = scores + slot_off[s0];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int j = j0 + wn * 64 + ni * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i < nq_c && j < len) blk[(int64_t)i * ld_c + j] = acc[mi][ni][r];
      }
    }
}

// ---- the per-query list keeper (csrc/knn.hip's, over ragged segments) --------------------------------------------------
__device__ __forceinline__ bool key_less(float d1, int i1, float d2, int i2) {
  return d1 < d2 || (d1 == d2 && i1 < i2);
}

// In-place bitonic sort of the wave's 256 (d, id) keys in LDS, ascending.  All 64 lanes of ONE wave take part; LDS
// operations of a wave retire in order, so the only fence needed between passes is against compiler reordering.
__device__ __forceinline__ void sort_buffer(float *kd, int *ki, int lane) {
#pragma unroll 1
  for (int size = 2; size <= kBuf; size <<= 1) {
#pragma unroll 1
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int t = 0; t < kBuf / 128; ++t) {
        const int p = lane + 64 * t;
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int j = i + stride;
        const bool up = (i & size) == 0;
        const float di = kd[i], dj = kd[j];
        const int ii = ki[i], ij = ki[j];
        if (key_less(dj, ij, di, ii) == up) {
          kd[i] = dj; ki[i] = ij;
          kd[j] = di; ki[j] = ii;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

__global__ void __launch_bounds__(256)
k_ivf_merge(const float *__restrict__ scores, const int64_t *__restrict__ slot_off, const int32_t *__restrict__ slot_of,
            const int32_t *__restrict__ probe, int nq, int nprobe, const int32_t *__restrict__ list_start,
            const int32_t *__restrict__ ids, const float *__restrict__ r_sq, const float *__restrict__ q_sq, int k,
            float *__restrict__ best_d, int *__restrict__ best_i) {
  __shared__ float s_d[kRowsPerBlock][kBuf];
  __shared__ int s_i[kRowsPerBlock][kBuf];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerBlock + w;
  if (row >= nq) return;                       // whole wave leaves; no block barrier below
  float *kd = s_d[w];
  int *ki = s_i[w];
  const float inf = __builtin_inff();
#pragma unroll
  for (int t = 0; t < kListCap / 64; ++t) {
    const int p = lane + 64 * t;
    kd[p] = inf;
    ki[p] = 0x7fffffff;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float tau_d = inf;
  int tau_i = 0x7fffffff;
  int n_buf = kListCap;                        // wave-uniform

  auto compact = [&]() {
#pragma unroll
    for (int t = 0; t < kBuf / 64; ++t) {
      const int p = lane + 64 * t;
      if (p >= n_buf) { kd[p] = inf; ki[p] = 0x7fffffff; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    sort_buffer(kd, ki, lane);
    tau_d = kd[k - 1];
    tau_i = ki[k - 1];
    n_buf = kListCap;
  };

  const float qs = q_sq[row];
  for (int j = 0; j < nprobe; ++j) {
    const int c = probe[(int64_t)row * nprobe + j];            // wave-uniform
    if (c < 0) continue;
    const int slot = slot_of[(int64_t)row * nprobe + j];
    if (slot < 0) continue;
    const int b = list_start[c], len = list_start[c + 1] - b;
    const float *srow = scores + slot_off[slot];               // 16-B aligned: every slot_off is a multiple of 4
    for (int c0 = 0; c0 < len; c0 += 256) {
      const int cc = c0 + lane * 4;
      f32x4 s = (f32x4)(0.f);
      if (cc < len) s = *reinterpret_cast<const f32x4 *>(srow + cc);   // (reads pad floats of the row; never uses them)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = cc + e < len;
        const float bs = in ? r_sq[b + cc + e] : 0.f;
        const int id = in ? ids[b + cc + e] : 0x7fffffff;
        const float dr = (qs + bs) - 2.f * s[e];
        const float d = dr < 0.f ? 0.f : dr;   // the clamp keeps a NaN; NaN never passes
        const bool pass = in && key_less(d, id, tau_d, tau_i);
        const unsigned long long m = __ballot(pass);
        if (m == 0ull) continue;
        const int cnt = __popcll(m);
        if (n_buf + cnt > kBuf) compact();     // frees kListCap >= 64 slots
        if (pass) {
          const int pos = n_buf + __popcll(m & ((1ull << lane) - 1ull));
          kd[pos] = d;
          ki[pos] = id;
        }
        n_buf += cnt;
      }
    }
  }
  compact();
  float *bd = best_d + (int64_t)row * kListCap;
  int *bi = best_i + (int64_t)row * kListCap;
#pragma unroll
  for (int t = 0; t < kListCap / 64; ++t) {
    const int p = lane + 64 * t;
    bd[p] = kd[p];
    bi[p] = ki[p];
  }
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_ivf_centroid_sums(const float *x, int64_t ldx, const int32_t *order, const int32_t *list_start, int nlist,
                                      int D, float *centroids, int64_t ldc, cdml_stream_t stream) {
  CDML_REQUIRE(x && order && list_start && centroids, CDML_E_BADARG, "ivf_centroid_sums: null pointer");
  CDML_REQUIRE(nlist > 0 && D > 0 && ldx >= D && ldc >= D, CDML_E_BADARG,
               "ivf_centroid_sums: nlist and D positive, ldx and ldc >= D (got %d, %d)", nlist, D);
  CDML_REQUIRE((D + 63) / 64 <= 65535, CDML_E_UNSUPPORTED, "ivf_centroid_sums: D too large (%d)", D);
  hipLaunchKernelGGL(k_ivf_centroid_sum, dim3(nlist, (D + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, ldx, order,
                     list_start, D, centroids, ldc);
  return check_launch("ivf_centroid_sums");
}

extern "C" int cdml_ivf_scan_f32(const float *Q, int64_t ldq, int n_queries, const int32_t *slot_query,
                                 const int32_t *slot_start, const int64_t *slot_off, const float *rows, int64_t ldr,
                                 const int32_t *list_start, int Dp, const int32_t *tiles, int n_tiles, float *scores,
                                 cdml_stream_t stream) {
  CDML_REQUIRE(Q && slot_query && slot_start && slot_off && rows && list_start && tiles && scores, CDML_E_BADARG,
               "ivf_scan_f32: null pointer");
  CDML_REQUIRE(n_queries > 0 && n_tiles > 0 && Dp > 0, CDML_E_BADARG, "ivf_scan_f32: bad size");
  CDML_REQUIRE(Dp % 32 == 0, CDML_E_UNSUPPORTED, "ivf_scan_f32: Dp must be a multiple of 32, got %d", Dp);
  CDML_REQUIRE(!(ldq & 3) && !(ldr & 3) && ldq >= Dp && ldr >= Dp && aligned16(Q) && aligned16(rows) && aligned16(tiles) &&
                   aligned16(scores),
               CDML_E_ALIGN, "ivf_scan_f32: strides multiples of 4 and >= Dp, bases 16-B aligned");
  hipLaunchKernelGGL(k_ivf_scan, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, Q, ldq, n_queries, slot_query, slot_start,
                     slot_off, rows, ldr, list_start, Dp, reinterpret_cast<const int4 *>(tiles), scores);
  return check_launch("ivf_scan_f32");
}

extern "C" int cdml_ivf_merge(const float *scores, const int64_t *slot_off, const int32_t *slot_of, const int32_t *probe, int nq,
                              int nprobe, const int32_t *list_start, const int32_t *ids, const float *r_sq, const float *q_sq,
                              int k, float *best_d, int32_t *best_i, cdml_stream_t stream) {
  CDML_REQUIRE(scores && slot_off && slot_of && probe && list_start && ids && r_sq && q_sq && best_d && best_i, CDML_E_BADARG,
               "ivf_merge: null pointer");
  CDML_REQUIRE(nq > 0, CDML_E_BADARG, "ivf_merge: bad size");
  CDML_REQUIRE(k >= 1 && k <= kListCap, CDML_E_UNSUPPORTED, "ivf_merge: k must be in [1, %d], got %d", kListCap, k);
  CDML_REQUIRE(nprobe >= 1 && nprobe <= kListCap, CDML_E_UNSUPPORTED, "ivf_merge: nprobe must be in [1, %d], got %d", kListCap,
               nprobe);
  CDML_REQUIRE(aligned16(scores), CDML_E_ALIGN, "ivf_merge: the score buffer must be 16-B aligned");
  hipLaunchKernelGGL(k_ivf_merge, dim3((nq + kRowsPerBlock - 1) / kRowsPerBlock), dim3(256), 0, (hipStream_t)stream, scores,
                     slot_off, slot_of, probe, nq, nprobe, list_start, ids, r_sq, q_sq, k, best_d, best_i);
  return check_launch("ivf_merge");
}

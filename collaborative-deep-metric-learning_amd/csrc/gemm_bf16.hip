// Reduced-precision variant of the tower for BASELINE config 4 ("fp16 features +
// bf16 MFMA projection"): the same layers as gemm_f32.hip (models.py:59-60 and
// their autodiff, train.py:141) with bf16 operands, fp32 accumulation
// (v_mfma_f32_32x32x16_bf16) and fp32 master weights.  Build-defined precision --
// the reference computes in fp32 -- so this path has its own, looser stated
// tolerance (tests: 5e-3 on unit-norm embeddings) and is never the default.
//
// One GEMM form serves every layer: C[M][N] = A[M][K] . B[N][K]^T with BOTH
// operands k-contiguous, which is what the bf16 MFMA fragment wants (8 consecutive
// k per lane for A and for B).  Layers whose operands are k-strided in memory
// (weight gradients: contraction over batch rows) get transposed bf16 copies from
// k_transpose_bf16.  Roofline: MFMA (2.5 PFLOP/s dense bf16); tile 128x128x64,
// 4 waves as 2x2, wave tile 64x64, register-staged double-buffered LDS with 144-B
// rows (conflict-free ds_read_b128), split-K slabs for the skinny weight gradient.
// Large products go to the 256x256 ping-pong kernel of gemm_bf16_256.hip; this one
// keeps the shapes that kernel does not take (N % 256, K % 128, few tiles).
#include <stdlib.h>
#include "gemm_bf16.h"
#include "gather_plan.h"

namespace cdml {
namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256;
constexpr int BM = 128, BN = 128, BKB = 64;
constexpr int ROWB = BKB + 8;  // bf16 per LDS row: 144 B, banks 36r mod 64 -> conflict-free b128 reads

template <int EPI>
__global__ void __launch_bounds__(kThreads, 2) k_gemm_bf16_nt(BArgs g) {
  constexpr int A_TILE = BM * ROWB, B_TILE = BN * ROWB;          // bf16 elements
  constexpr int STAGE_BYTES = (A_TILE + B_TILE) * 2;
  constexpr int SMEM_BYTES = 2 * STAGE_BYTES > BM * BN * 4 ? 2 * STAGE_BYTES : BM * BN * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[SMEM_BYTES];
  bf16 *smem = reinterpret_cast<bf16 *>(smem_raw);

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;

  int tm, tn;
  tile_of_block(blockIdx.x, gridDim.x, g.tiles_m, g.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int split = blockIdx.y;
  const int k_begin = split * g.k_per_split;
  const int k_end = min(g.K, k_begin + g.k_per_split);
  const int n_ktiles = (k_end - k_begin + BKB - 1) / BKB;  // K and k_per_split are multiples of 64

  struct Stage { bf16x8 a[4]; bf16x8 b[4]; };
  auto load_tile = [&](int kt) {
    Stage st;
    const int k0 = k_begin + kt * BKB;
#pragma unroll
    for (int p = 0; p < 4; ++p) {  // 128 rows x 8 chunks of 16 B
      const int row = p * 32 + (t >> 3), ch = t & 7;
      st.a[p] = *reinterpret_cast<const bf16x8 *>(g.A + (int64_t)min(m0 + row, g.M - 1) * g.lda + k0 + ch * 8);
      st.b[p] = *reinterpret_cast<const bf16x8 *>(g.B + (int64_t)(n0 + row) * g.ldb + k0 + ch * 8);
    }
    return st;
  };
  auto store_tile = [&](int buf, Stage st) {
    bf16 *sA = smem + buf * (A_TILE + B_TILE);
    bf16 *sB = sA + A_TILE;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = p * 32 + (t >> 3), ch = t & 7;
      *reinterpret_cast<bf16x8 *>(sA + row * ROWB + ch * 8) = st.a[p];
      *reinterpret_cast<bf16x8 *>(sB + row * ROWB + ch * 8) = st.b[p];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  Stage s0;
  if (n_ktiles > 0) {
    s0 = load_tile(0);
    store_tile(0, s0);
  }
  __syncthreads();
  for (int kt = 0; kt < n_ktiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < n_ktiles) s0 = load_tile(kt + 1);
    const bf16 *sA = smem + buf * (A_TILE + B_TILE);
    const bf16 *sB = sA + A_TILE;
#pragma unroll
    for (int kk = 0; kk < BKB / 16; ++kk) {  // lane (l31, h) holds k = 16*kk + 8*h + 0..7
      bf16x8 a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        a[mi] = *reinterpret_cast<const bf16x8 *>(sA + (wm * 64 + mi * 32 + l31) * ROWB + kk * 16 + 8 * h);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        b[ni] = *reinterpret_cast<const bf16x8 *>(sB + (wn * 64 + ni * 32 + l31) * ROWB + kk * 16 + 8 * h);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    if (kt + 1 < n_ktiles) store_tile(buf ^ 1, s0);
    __syncthreads();
  }

  // epilogue through an fp32 LDS C tile (C/D layout as in gemm_f32.hip)
  float *sC = reinterpret_cast<float *>(smem_raw);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        sC[row * BN + wn * 64 + ni * 32 + l31] = acc[mi][ni][r];
      }
  __syncthreads();

  const int c4 = t & 31, lr0 = t >> 5;  // 32 x 16-B segments per row, 8 rows per pass
  const int col = n0 + c4 * 4;
  f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f};
  if (EPI == BE_BIAS_LRELU_BF16 || EPI == BE_BIAS_LRELU_F32) bias4 = *reinterpret_cast<const f32x4 *>(g.bias + col);
  const bool has_aux = (EPI == BE_MASK_BF16) && g.aux != nullptr;
  // the 16 mask loads of a thread go out together (rows clamped): a load under the row branch
  // is waited for on the spot, 16 dependent round trips per tile
  bf16x4 mk[BM / 8];
  if (EPI == BE_MASK_BF16 && has_aux) {
#pragma unroll
    for (int p = 0; p < BM / 8; ++p)
      mk[p] = *reinterpret_cast<const bf16x4 *>(g.aux + (int64_t)min(m0 + p * 8 + lr0, g.M - 1) * g.ldaux + col);
  }
#pragma unroll
  for (int p = 0; p < BM / 8; ++p) {
    const int lr = p * 8 + lr0;
    const int row = m0 + lr;
    f32x4 v = *reinterpret_cast<const f32x4 *>(sC + lr * BN + c4 * 4);
    if (EPI == BE_BIAS_LRELU_BF16 || EPI == BE_BIAS_LRELU_F32) {
      v += bias4;
      v.x = fmaxf(v.x, v.x * g.alpha); v.y = fmaxf(v.y, v.y * g.alpha);
      v.z = fmaxf(v.z, v.z * g.alpha); v.w = fmaxf(v.w, v.w * g.alpha);
    } else if (EPI == BE_MASK_BF16) {
      if (has_aux) {
        const bf16x4 m = mk[p];
        v.x *= ((float)m.x > 0.f) ? 1.f : g.alpha; v.y *= ((float)m.y > 0.f) ? 1.f : g.alpha;
        v.z *= ((float)m.z > 0.f) ? 1.f : g.alpha; v.w *= ((float)m.w > 0.f) ? 1.f : g.alpha;
      }
    }
    if (row >= g.M) continue;                                // stores only below this line
    if (EPI == BE_BIAS_LRELU_BF16 || EPI == BE_MASK_BF16) {
      bf16x4 o;
      o.x = (bf16)v.x; o.y = (bf16)v.y; o.z = (bf16)v.z; o.w = (bf16)v.w;
      *reinterpret_cast<bf16x4 *>(static_cast<bf16 *>(g.C) + (int64_t)row * g.ldc + col) = o;
    } else {
      float *C = static_cast<float *>(g.C) + (EPI == BE_F32 ? (int64_t)split * g.slab_stride : 0);
      *reinterpret_cast<f32x4 *>(C + (int64_t)row * g.ldc + col) = v;
    }
  }
}

// out[c][r] = (bf16) in[r][c]; 64x64 tiles through LDS.  SRC = float or bf16.
template <typename SRC>
__global__ void __launch_bounds__(kThreads)
k_transpose_bf16(const SRC *__restrict__ in, int64_t ldi, int rows, int cols, bf16 *__restrict__ out,
                 int64_t ldo) {
  __shared__ bf16 s[64][66];
  const int t = threadIdx.x;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  for (int i = t; i < 64 * 64; i += kThreads) {
    const int r = i >> 6, c = i & 63;
    const int gr = r0 + r, gc = c0 + c;
    s[r][c] = (gr < rows && gc < cols) ? (bf16)(float)in[(int64_t)gr * ldi + gc] : (bf16)0.f;
  }
  __syncthreads();
  for (int i = t; i < 64 * 64; i += kThreads) {
    const int c = i >> 6, r = i & 63;
    const int gr = r0 + r, gc = c0 + c;
    if (gr < rows && gc < cols) out[(int64_t)gc * ldo + gr] = s[r][c];
  }
}

__global__ void __launch_bounds__(kThreads)
k_cast_f32_bf16(const float *__restrict__ in, int64_t ldi, int rows, int cols, bf16 *__restrict__ out,
                int64_t ldo) {
  const int c4n = cols >> 2;
  const int64_t total = (int64_t)rows * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / c4n;
    const int c = (int)(i - r * c4n) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(in + r * ldi + c);
    bf16x4 o;
    o.x = (bf16)v.x; o.y = (bf16)v.y; o.z = (bf16)v.z; o.w = (bf16)v.w;
    *reinterpret_cast<bf16x4 *>(out + r * ldo + c) = o;
  }
}

// column sums in two deterministic stages: partial[chunk][col] then the chunk sum.
// A block covers 128 columns x one row chunk: 32 four-column lanes x 8 row lanes,
// each thread strides the rows by 8 with 4-wide loads, then the 8 row lanes are
// combined through LDS in a fixed order.
__device__ __forceinline__ f32x4 load4f(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ f32x4 load4f(const bf16 *p) {
  const bf16x4 v = *reinterpret_cast<const bf16x4 *>(p);
  return f32x4{(float)v.x, (float)v.y, (float)v.z, (float)v.w};
}
template <typename SRC>
__global__ void __launch_bounds__(kThreads)
k_colsum_partial(const SRC *__restrict__ in, int64_t ld, int rows, int cols, int rows_per_chunk,
                 float *__restrict__ partial) {
  __shared__ f32x4 red[8][32];
  const int c4 = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 128 + c4 * 4;
  const int r_lo = blockIdx.y * rows_per_chunk, r_hi = min(rows, r_lo + rows_per_chunk);
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c < cols)
    for (int r = r_lo + rl; r < r_hi; r += 8) s += load4f(in + (int64_t)r * ld + c);
  red[rl][c4] = s;
  __syncthreads();
  if (rl == 0 && c < cols) {
#pragma unroll
    for (int j = 1; j < 8; ++j) s += red[j][c4];
    *reinterpret_cast<f32x4 *>(partial + (int64_t)blockIdx.y * cols + c) = s;
  }
}
// out[c] = sum_k partial[k][c], fixed order: a block owns 128 columns; its 8 row groups add every
// 8th partial row (independent loads, pipelined), then the 8 group sums are added in order.
// (One thread per column walking all chunks one after the other took 34 us at 256 chunks.)
__device__ __forceinline__ void colsum_final_block(const float *__restrict__ partial, int chunks, int cols,
                                                   float *__restrict__ out, int blk, bool narrow) {
  // CQ column quads x RL row lanes per block: few columns and many partial rows (the second layer's bias gradient:
  // 480 rows x 256 columns) get 32 row lanes over 8 blocks instead of 8 over 2 (10.5 -> ~4 us)
  __shared__ f32x4 red[kThreads];
  const int CQ = narrow ? 8 : 32, RL = kThreads / CQ;
  const int c4 = threadIdx.x % CQ, rl = threadIdx.x / CQ;
  const int c = blk * (CQ * 4) + c4 * 4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c < cols)
    for (int k = rl; k < chunks; k += RL) s += *reinterpret_cast<const f32x4 *>(partial + (int64_t)k * cols + c);
  red[rl * CQ + c4] = s;
  __syncthreads();
  if (rl == 0 && c < cols) {
    for (int j = 1; j < RL; ++j) s += red[j * CQ + c4];
    *reinterpret_cast<f32x4 *>(out + c) = s;
  }
}
__global__ void __launch_bounds__(kThreads)
k_colsum_final(const float *__restrict__ partial, int chunks, int cols, float *__restrict__ out) {
  colsum_final_block(partial, chunks, cols, out, blockIdx.x, gridDim.x * 32 >= (unsigned)cols);   // (cols + 31) / 32 blocks = narrow
}

// blocks [0, slab_blocks): out = the slabs added in order; the blocks after them (round 4): the bias gradient's final
// sums from its partial rows, in the same launch (cs_narrow: colsum_final_blocks' choice)
__global__ void __launch_bounds__(kThreads)
k_sum_slabs_f32(const float *__restrict__ slabs, int64_t slab_stride, int splits, int rows, int N,
                float *__restrict__ out, int64_t ldo, int slab_blocks, const float *__restrict__ cs_partial, int cs_chunks,
                float *__restrict__ cs_out, int cs_narrow) {
  if ((int)blockIdx.x >= slab_blocks) {
    colsum_final_block(cs_partial, cs_chunks, N, cs_out, blockIdx.x - slab_blocks, cs_narrow != 0);
    return;
  }
  const int n4 = N >> 2;
  const int64_t total = (int64_t)rows * n4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)slab_blocks * blockDim.x) {
    const int64_t r = i / n4;
    const int c = (int)(i - r * n4);
    f32x4 s = reinterpret_cast<const f32x4 *>(slabs)[i];
    for (int z = 1; z < splits; ++z) s += reinterpret_cast<const f32x4 *>(slabs + (int64_t)z * slab_stride)[i];
    reinterpret_cast<f32x4 *>(out + r * ldo)[c] = s;
  }
}

// out = lrelu(sum_z slab[z] + bias): the split-K form of the narrow output layer (N = 256
// gives the big kernel too few tiles; two K-halves fill the chip and this pass finishes it)
__global__ void __launch_bounds__(kThreads)
k_sum_slabs_bias_lrelu(const float *__restrict__ slabs, int64_t slab_stride, int splits, int rows, int N,
                       const float *__restrict__ bias, float alpha, float *__restrict__ out, int64_t ldo) {
  const int n4 = N >> 2;
  const int64_t total = (int64_t)rows * n4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / n4;
    const int c = (int)(i - r * n4);
    f32x4 s = reinterpret_cast<const f32x4 *>(slabs)[i];
    for (int z = 1; z < splits; ++z) s += reinterpret_cast<const f32x4 *>(slabs + (int64_t)z * slab_stride)[i];
    s += reinterpret_cast<const f32x4 *>(bias)[c];
    s.x = fmaxf(s.x, s.x * alpha); s.y = fmaxf(s.y, s.y * alpha);
    s.z = fmaxf(s.z, s.z * alpha); s.w = fmaxf(s.w, s.w * alpha);
    reinterpret_cast<f32x4 *>(out + r * ldo)[c] = s;
  }
}

// fp16 catalogue: Philox table (same stream as the fp32 one, rounded to half) and
// the row gather: fp16 rows in, l2-normalised (fp32 arithmetic) bf16 rows out.
__global__ void __launch_bounds__(kThreads)
k_fill_table_f16(_Float16 *__restrict__ table, int64_t row0, int64_t n_rows, int F, int64_t row_stride,
                 uint64_t seed) {
  const int64_t q_per_row = row_stride >> 2;
  const int64_t total = n_rows * q_per_row;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lr = i / q_per_row;
    const int64_t q = i - lr * q_per_row;
    const uint64_t r = (uint64_t)(row0 + lr);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int64_t j = q * 4;
    if (j < F) {
      const u32x4 w = philox4x32_10(u32x4{(uint32_t)q, (uint32_t)r, (uint32_t)(r >> 32), kTableTag}, k0, k1);
      const float s = 5.9604644775390625e-08f;
      v[0] = (float)(w.x >> 8) * s;
      if (j + 1 < F) v[1] = (float)(w.y >> 8) * s;
      if (j + 2 < F) v[2] = (float)(w.z >> 8) * s;
      if (j + 3 < F) v[3] = (float)(w.w >> 8) * s;
    }
    _Float16 *d = table + i * 4;
    d[0] = (_Float16)v[0]; d[1] = (_Float16)v[1];
    d[2] = (_Float16)v[2]; d[3] = (_Float16)v[3];
  }
}

using half8 = __attribute__((ext_vector_type(8))) _Float16;
template <int NCH>  // 16-B chunks (8 halfs) per lane
__global__ void __launch_bounds__(kThreads)
k_gather_rows_f16(const _Float16 *__restrict__ table, int64_t row0, int64_t n_rows, int64_t row_stride,
                  const int32_t *__restrict__ idx, int n_idx, int F, bf16 *__restrict__ x_out,
                  int64_t out_stride, int32_t *__restrict__ oob_flag) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nq = (F + 7) >> 3, oq = (int)(out_stride >> 3);
  for (int r = blockIdx.x * 4 + wave; r < n_idx; r += gridDim.x * 4) {
    if (idx[r] == -1) continue;                  // padding slot of a fixed-capacity exchange
    int64_t lr = (int64_t)idx[r] - row0;
    if (lr < 0 || lr >= n_rows) {
      if (oob_flag) atomicOr(oob_flag, 1);
      lr = lr < 0 ? 0 : n_rows - 1;
    }
    const half8 *src = reinterpret_cast<const half8 *>(table + lr * row_stride);
    half8 v[NCH];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + 64 * c;
      half8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (q < nq) x = src[q];
      ss = f16_chunk_sumsq(x, q, F, ss);           // (the pad zeroed in x; the same arithmetic as the fused kernel)
      v[c] = x;
    }
    ss = wave_sum(ss);
    const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
    bf16x8 *d = reinterpret_cast<bf16x8 *>(x_out + (int64_t)r * out_stride);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + 64 * c;
      if (q < oq) {
        bf16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = (bf16)((float)v[c][u] * inv);
        d[q] = o;
      }
    }
    for (int q = lane + 64 * NCH; q < oq; q += 64) d[q] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

int bf16_splits(int M, int N, int K) {
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * (N / BN);
  int64_t splits = (480 + tiles - 1) / tiles;
  const int64_t max_by_k = (K + 511) / 512;
  if (splits > max_by_k) splits = max_by_k;
  if (splits > 32) splits = 32;
  return (int)(splits < 1 ? 1 : splits);
}

int grid1d(int64_t n, int per_thread) {
  int64_t b = (n / per_thread + kThreads - 1) / kThreads;
  if (b > kNumCU * 8) b = kNumCU * 8;
  return (int)(b < 1 ? 1 : b);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

// 0 = choose by shape, 128 / 256 = force that kernel where it applies (A/B runs)
static int forced_tile() {
  const char *e = getenv("CDML_BF16_TILE");     // read per call: tests flip it
  return e ? atoi(e) : 0;
}

static bool use_256(int epilogue, int M, int N, int K, int64_t lda, int64_t ldb) {
  if (forced_tile() == 128 || !gemm_bf16_256_usable(M, N, K, lda, ldb)) return false;
  if (forced_tile() == 256) return true;
  const int64_t tiles = (int64_t)((M + 255) / 256) * (N / 256);
  return K >= 256 && (epilogue == BE_F32 ? tiles * gemm_bf16_256_splits(M, N, K) >= 128 : tiles >= 192);
}

// Narrow fp32-output forward layer (epilogue 1) on the 256x256 kernel: split K until most of
// the chip has a block; the bias + leaky-relu then move to the slab combine.  1 = do not split.
static int fwd_f32_splits(int M, int N, int K, int64_t lda, int64_t ldb) {
  if (forced_tile() == 128 || !gemm_bf16_256_usable(M, N, K, lda, ldb)) return 1;
  const int64_t tiles = (int64_t)((M + 255) / 256) * (N / 256);
  if (tiles >= 192) return 1;
  int s = (int)((170 + tiles - 1) / tiles);
  const int max_by_k = K / 512;
  if (s > max_by_k) s = max_by_k;
  if (s > 8) s = 8;
  return s < 2 ? 1 : s;
}

// k_colsum_final's grid: 32 columns per block (32 row lanes) when there are many partial rows for few columns,
// else 128 columns per block (8 row lanes); the kernel tells the two apart by gridDim.x
static int colsum_final_blocks(int chunks, int cols) {
  return (chunks >= 64 && cols <= 1024) ? (cols + 31) / 32 : (cols + 127) / 128;
}

extern "C" size_t cdml_gemm_bf16_workspace(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || N % BN || K % BKB) return 0;
  int splits = bf16_splits(M, N, K);             // enough for whichever kernel / epilogue is dispatched
  if (gemm_bf16_256_usable(M, N, K, K, K))
    splits = max(splits, max(gemm_bf16_256_splits(M, N, K), fwd_f32_splits(M, N, K, K, K)));
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

extern "C" int cdml_gemm_bf16_epilogue_supported(int epilogue, int M, int N, int K, int64_t lda, int64_t ldb,
                                                 int64_t ldc, int64_t ldaux) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if (epilogue >= 0 && epilogue <= 3) return (N % BN == 0 && K % BKB == 0) ? 1 : 0;
  if (epilogue == BE_BIAS_LRELU_BF16_BITS)
    return (gemm_bf16_256_usable(M, N, K, lda, ldb) && ldaux * 8 >= N) ? 1 : 0;
  if (epilogue == BE_MASKBITS_BF16)
    return (K == 256 && N % 256 == 0 && !(lda & 7) && !(ldb & 7) && !(ldc & 7) && ldaux * 8 >= N &&
            gemm_bf16_k256_usable(M, N, K, lda, ldb, ldc, 8, true)) ? 1 : 0;
  return 0;
}

extern "C" int cdml_gemm_bf16_nt(int epilogue, const uint16_t *A, int64_t lda, const uint16_t *B,
                                 int64_t ldb, int M, int N, int K, void *C, int64_t ldc,
                                 const float *bias, const uint16_t *aux, int64_t ldaux, float alpha,
                                 void *workspace, size_t workspace_bytes, cdml_stream_t stream) {
  CDML_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, CDML_E_BADARG, "gemm_bf16_nt: bad argument");
  CDML_REQUIRE(epilogue >= 0 && epilogue <= 5, CDML_E_BADARG, "gemm_bf16_nt: epilogue must be 0..5");
  CDML_REQUIRE(N % BN == 0 && K % BKB == 0, CDML_E_UNSUPPORTED,
               "gemm_bf16_nt: N must be a multiple of 128 and K of 64, got N=%d K=%d", N, K);
  CDML_REQUIRE(aligned16(A) && aligned16(B) && aligned16(C) && (lda & 7) == 0 && (ldb & 7) == 0 &&
                   (ldc & 3) == 0 && lda >= K && ldb >= K && ldc >= N,
               CDML_E_ALIGN, "gemm_bf16_nt: 16-B aligned bases, lda/ldb multiples of 8, ldc of 4");
  CDML_REQUIRE(epilogue > 1 && epilogue != BE_BIAS_LRELU_BF16_BITS ? true : bias != nullptr, CDML_E_BADARG,
               "gemm_bf16_nt: bias required");
  BArgs g{};
  if (epilogue == BE_BIAS_LRELU_BF16_BITS || epilogue == BE_MASKBITS_BF16) {
    CDML_REQUIRE(aux && ldaux * 8 >= N && cdml_gemm_bf16_epilogue_supported(epilogue, M, N, K, lda, ldb, ldc, ldaux),
                 CDML_E_UNSUPPORTED, "gemm_bf16_nt: the bitmask epilogue %d does not take M=%d N=%d K=%d "
                 "(cdml_gemm_bf16_epilogue_supported); use epilogue %d", epilogue, M, N, K, epilogue == 4 ? 0 : 2);
  }
  g.A = reinterpret_cast<const bf16 *>(A); g.lda = lda;
  g.B = reinterpret_cast<const bf16 *>(B); g.ldb = ldb;
  g.C = C; g.ldc = ldc; g.bias = bias;
  g.aux = reinterpret_cast<const bf16 *>(aux); g.ldaux = ldaux; g.alpha = alpha;
  g.M = M; g.N = N; g.K = K; g.k_per_split = K;
  g.tiles_m = (M + BM - 1) / BM; g.tiles_n = N / BN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kThreads);
  if (epilogue == BE_BIAS_LRELU_BF16_BITS) {       // epilogue 0 on the 256x256 kernel + the sign bitmask
    g.mask_out = reinterpret_cast<uint8_t *>(const_cast<uint16_t *>(aux)); g.ldmask = ldaux;
    g.aux = nullptr; g.ldaux = 0;
    g.tiles_m = (M + 255) / 256; g.tiles_n = N / 256;
    return launch_gemm_bf16_256(g, BE_BIAS_LRELU_BF16, 1, s);
  }
  if (epilogue == BE_MASKBITS_BF16) {              // the K = 256 streaming kernel reading the bitmask
    g.aux_bits = 1;
    return launch_gemm_bf16_k256(g, s);
  }
  if (epilogue == BE_BIAS_LRELU_F32) {
    const int fs = fwd_f32_splits(M, N, K, lda, ldb);
    const size_t need = (size_t)fs * M * N * sizeof(float);
    if (fs > 1 && workspace && workspace_bytes >= need && aligned16(workspace)) {   // else: one-pass kernels below
      g.k_per_split = ((K + fs - 1) / fs + 2 * BKB - 1) / (2 * BKB) * (2 * BKB);
      g.slab_stride = (int64_t)M * N;
      g.C = workspace; g.ldc = N;
      g.tiles_m = (M + 255) / 256; g.tiles_n = N / 256;
      int rc = launch_gemm_bf16_256(g, BE_F32, fs, s);
      if (rc) return rc;
      hipLaunchKernelGGL(k_sum_slabs_bias_lrelu, dim3(grid1d((int64_t)M * N / 4, 1)), block, 0, s,
                         static_cast<const float *>(workspace), g.slab_stride, fs, M, N, bias, alpha,
                         static_cast<float *>(C), ldc);
      return check_launch("gemm_bf16_nt combine + bias + lrelu");
    }
  }
  // the K = 256 data gradient is a streaming problem, not a tiled one (gemm_bf16_k256.hip)
  if (epilogue == BE_MASK_BF16 && forced_tile() == 0 && (int64_t)M * N >= ((int64_t)1 << 22) &&
      gemm_bf16_k256_usable(M, N, K, lda, ldb, ldc, ldaux, aux != nullptr) && (!aux || aligned16(aux)))
    return launch_gemm_bf16_k256(g, s);
  const bool big = use_256(epilogue, M, N, K, lda, ldb);
  int splits = 1;
  if (epilogue == BE_F32) {
    splits = big ? gemm_bf16_256_splits(M, N, K) : bf16_splits(M, N, K);
    if (splits > 1) {
      const size_t need = (size_t)splits * M * N * sizeof(float);
      CDML_REQUIRE(workspace && workspace_bytes >= need && aligned16(workspace), CDML_E_BADARG,
                   "gemm_bf16_nt: split-K workspace of %zu bytes required", need);
      const int kq = big ? 2 * BKB : BKB;        // the 256 kernel walks K-tiles in pairs
      int kps = (K + splits - 1) / splits;
      g.k_per_split = (kps + kq - 1) / kq * kq;
      g.slab_stride = (int64_t)M * N;
      g.C = workspace; g.ldc = N;
    }
  }
  int rc;
  if (big) {
    g.tiles_m = (M + 255) / 256; g.tiles_n = N / 256;
    rc = launch_gemm_bf16_256(g, epilogue, splits, s);
  } else {
  const dim3 grid(g.tiles_m * g.tiles_n, splits);
  switch (epilogue) {
    case BE_BIAS_LRELU_BF16: hipLaunchKernelGGL((k_gemm_bf16_nt<BE_BIAS_LRELU_BF16>), grid, block, 0, s, g); break;
    case BE_BIAS_LRELU_F32: hipLaunchKernelGGL((k_gemm_bf16_nt<BE_BIAS_LRELU_F32>), grid, block, 0, s, g); break;
    case BE_MASK_BF16: hipLaunchKernelGGL((k_gemm_bf16_nt<BE_MASK_BF16>), grid, block, 0, s, g); break;
    default: hipLaunchKernelGGL((k_gemm_bf16_nt<BE_F32>), grid, block, 0, s, g); break;
  }
  rc = check_launch("gemm_bf16_nt");
  }
  if (rc || splits == 1) return rc;
  const int sbn = grid1d((int64_t)M * N / 4, 1);
  hipLaunchKernelGGL(k_sum_slabs_f32, dim3(sbn), block, 0, s, static_cast<const float *>(workspace), g.slab_stride, splits, M, N,
                     static_cast<float *>(C), ldc, sbn, static_cast<const float *>(nullptr), 0, static_cast<float *>(nullptr), 0);
  return check_launch("gemm_bf16_nt combine");
}

extern "C" int cdml_gemm_bf16_tn_supported(int M, int N, int K, int64_t lda, int64_t ldb) {
  return gemm_bf16_tn_usable(M, N, K, lda, ldb) ? 1 : 0;
}

extern "C" size_t cdml_gemm_bf16_tn_workspace(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return bf16_tn_plan(M, N, K, true).need;                  // slabs + the column sums of B
}

extern "C" int cdml_gemm_bf16_tn(const uint16_t *A, int64_t lda, const uint16_t *B, int64_t ldb, int M,
                                 int N, int K, float *C, int64_t ldc, float *colsum, void *workspace,
                                 size_t workspace_bytes, cdml_stream_t stream) {
  CDML_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, CDML_E_BADARG, "gemm_bf16_tn: bad argument");
  CDML_REQUIRE(aligned16(A) && aligned16(B) && aligned16(C) && (lda & 7) == 0 && (ldb & 7) == 0 &&
                   (ldc & 3) == 0 && lda >= M && ldb >= N && ldc >= N,
               CDML_E_ALIGN, "gemm_bf16_tn: 16-B aligned bases, lda/ldb multiples of 8, ldc of 4");
  CDML_REQUIRE(gemm_bf16_tn_usable(M, N, K, lda, ldb), CDML_E_UNSUPPORTED,
               "gemm_bf16_tn: needs M, N multiples of 256 and K of 128 (got M=%d N=%d K=%d); use "
               "cdml_transpose_to_bf16 + cdml_gemm_bf16_nt for other shapes", M, N, K);
  BArgs g{};
  g.A = reinterpret_cast<const bf16 *>(A); g.lda = lda;
  g.B = reinterpret_cast<const bf16 *>(B); g.ldb = ldb;
  g.C = C; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.k_per_split = K;
  g.tiles_m = M / 256; g.tiles_n = N / 256;
  const KSplitPlan p = bf16_tn_plan(M, N, K, colsum != nullptr);
  const int chunks = (int)p.cs_rows;
  hipStream_t s = (hipStream_t)stream;
  CDML_REQUIRE(p.need == 0 || (workspace && workspace_bytes >= p.need && aligned16(workspace)), CDML_E_BADARG,
               "gemm_bf16_tn: workspace of %zu bytes required", p.need);
  if (p.slabs) {
    g.k_per_split = p.per * 64;
    g.slab_stride = (int64_t)M * N;
    g.C = workspace; g.ldc = N;
  }
  if (colsum) g.colsum_partial = reinterpret_cast<float *>(static_cast<char *>(workspace) + p.slab_bytes);
  int rc = launch_gemm_bf16_tn(g, p.splits, s);
  if (rc) return rc;
  if (p.slabs) {                                           // the slab sum and, in extra blocks, the bias gradient's final sums
    const int sb = grid1d((int64_t)M * N / 4, 1), cb = colsum ? colsum_final_blocks(chunks, N) : 0;
    hipLaunchKernelGGL(k_sum_slabs_f32, dim3(sb + cb), dim3(kThreads), 0, s, static_cast<const float *>(workspace), g.slab_stride,
                       p.splits, M, N, C, ldc, sb, g.colsum_partial, chunks, colsum, (cb * 32 >= N) ? 1 : 0);
    return check_launch("gemm_bf16_tn combine");
  }
  if (colsum) {
    hipLaunchKernelGGL(k_colsum_final, dim3(colsum_final_blocks(chunks, N)), dim3(kThreads), 0, s,
                       g.colsum_partial, chunks, N, colsum);
    rc = check_launch("gemm_bf16_tn bias gradient");
  }
  return rc;
}

extern "C" size_t cdml_gemm_bf16_tn2_workspace(int M1, int N1, int M2, int N2, int K) {
  if (M1 <= 0 || N1 <= 0 || M2 <= 0 || N2 <= 0 || K <= 0) return 0;
  return gemm_bf16_tn2_workspace(M1, N1, M2, N2, K);
}

extern "C" int cdml_gemm_bf16_tn2(const uint16_t *A1, int64_t lda1, const uint16_t *B1, int64_t ldb1, int M1, int N1,
                                  float *C1, int64_t ldc1, float *colsum1, const uint16_t *A2, int64_t lda2,
                                  const uint16_t *B2, int64_t ldb2, int M2, int N2, float *C2, int64_t ldc2,
                                  float *colsum2, int K, void *workspace, size_t workspace_bytes,
                                  cdml_stream_t stream) {
  CDML_REQUIRE(A1 && B1 && C1 && A2 && B2 && C2 && M1 > 0 && N1 > 0 && M2 > 0 && N2 > 0 && K > 0, CDML_E_BADARG,
               "gemm_bf16_tn2: bad argument");
  CDML_REQUIRE(aligned16(A1) && aligned16(B1) && aligned16(C1) && aligned16(A2) && aligned16(B2) && aligned16(C2) &&
                   !(lda1 & 7) && !(ldb1 & 7) && !(ldc1 & 3) && !(lda2 & 7) && !(ldb2 & 7) && !(ldc2 & 3) &&
                   lda1 >= M1 && ldb1 >= N1 && ldc1 >= N1 && lda2 >= M2 && ldb2 >= N2 && ldc2 >= N2 && aligned16(workspace),
               CDML_E_ALIGN, "gemm_bf16_tn2: 16-B aligned bases, lda/ldb multiples of 8, ldc of 4");
  CDML_REQUIRE(gemm_bf16_tn_usable(M1, N1, K, lda1, ldb1) && gemm_bf16_tn_usable(M2, N2, K, lda2, ldb2) &&
                   gemm_bf16_tn2_workspace(M1, N1, M2, N2, K) > 0,
               CDML_E_UNSUPPORTED, "gemm_bf16_tn2: needs M, N multiples of 256 and K of 128 for both products "
               "(cdml_gemm_bf16_tn2_workspace returns 0 otherwise); use cdml_gemm_bf16_tn per product");
  BArgs g1{}, g2{};
  g1.A = reinterpret_cast<const bf16 *>(A1); g1.lda = lda1; g1.B = reinterpret_cast<const bf16 *>(B1); g1.ldb = ldb1;
  g1.C = C1; g1.ldc = ldc1; g1.M = M1; g1.N = N1; g1.K = K; g1.k_per_split = K;
  g2.A = reinterpret_cast<const bf16 *>(A2); g2.lda = lda2; g2.B = reinterpret_cast<const bf16 *>(B2); g2.ldb = ldb2;
  g2.C = C2; g2.ldc = ldc2; g2.M = M2; g2.N = N2; g2.K = K; g2.k_per_split = K;
  return launch_gemm_bf16_tn2(g1, g2, colsum1, colsum2, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int cdml_transpose_to_bf16(int src_is_f32, const void *src, int64_t lds_, int rows, int cols,
                                      uint16_t *dst, int64_t ldd, cdml_stream_t stream) {
  CDML_REQUIRE(src && dst && rows > 0 && cols > 0 && lds_ >= cols && ldd >= rows, CDML_E_BADARG,
               "transpose_to_bf16: bad argument");
  const dim3 grid((cols + 63) / 64, (rows + 63) / 64);
  if (src_is_f32)
    hipLaunchKernelGGL((k_transpose_bf16<float>), grid, dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const float *>(src), lds_, rows, cols, reinterpret_cast<bf16 *>(dst), ldd);
  else
    hipLaunchKernelGGL((k_transpose_bf16<bf16>), grid, dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const bf16 *>(src), lds_, rows, cols, reinterpret_cast<bf16 *>(dst), ldd);
  return check_launch("transpose_to_bf16");
}

extern "C" int cdml_cast_f32_bf16(const float *src, int64_t lds_, int rows, int cols, uint16_t *dst,
                                  int64_t ldd, cdml_stream_t stream) {
  CDML_REQUIRE(src && dst && rows > 0 && cols > 0, CDML_E_BADARG, "cast_f32_bf16: bad argument");
  CDML_REQUIRE((cols & 3) == 0 && (lds_ & 3) == 0 && (ldd & 3) == 0 && aligned16(src) &&
                   (reinterpret_cast<uintptr_t>(dst) & 7) == 0,
               CDML_E_ALIGN, "cast_f32_bf16: widths and strides must be multiples of 4");
  hipLaunchKernelGGL(k_cast_f32_bf16, dim3(grid1d((int64_t)rows * cols / 4, 1)), dim3(kThreads), 0,
                     (hipStream_t)stream, src, lds_, rows, cols, reinterpret_cast<bf16 *>(dst), ldd);
  return check_launch("cast_f32_bf16");
}

// enough row chunks to fill the chip (~1024 blocks), at least 64 rows each, at most
// 64 chunks so the final pass stays short
static int colsum_chunks(int rows, int cols) {
  const int gx = (cols + 127) / 128;
  int chunks = (1024 + gx - 1) / gx;
  const int max_chunks = (rows + 63) / 64;
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks > 256) chunks = 256;   // (64 left a 24 576 x 256 sum on 128 blocks: 23 us for 25 MB)
  return chunks < 1 ? 1 : chunks;
}

extern "C" size_t cdml_colsum_workspace_floats(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return (size_t)colsum_chunks(rows, cols) * cols;
}

extern "C" int cdml_colsum(int src_is_bf16, const void *src, int64_t ld, int rows, int cols, float *out,
                           float *workspace, cdml_stream_t stream) {
  CDML_REQUIRE(src && out && workspace && rows > 0 && cols > 0 && ld >= cols, CDML_E_BADARG,
               "colsum: bad argument");
  CDML_REQUIRE((cols & 3) == 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0, CDML_E_ALIGN,
               "colsum: cols and ld must be multiples of 4, base 16-B aligned");
  const int chunks = colsum_chunks(rows, cols);
  const int rpc = (rows + chunks - 1) / chunks;
  const dim3 grid((cols + 127) / 128, chunks);
  hipStream_t s = (hipStream_t)stream;
  if (src_is_bf16)
    hipLaunchKernelGGL((k_colsum_partial<bf16>), grid, dim3(kThreads), 0, s, static_cast<const bf16 *>(src),
                       ld, rows, cols, rpc, workspace);
  else
    hipLaunchKernelGGL((k_colsum_partial<float>), grid, dim3(kThreads), 0, s,
                       static_cast<const float *>(src), ld, rows, cols, rpc, workspace);
  hipLaunchKernelGGL(k_colsum_final, dim3(colsum_final_blocks(chunks, cols)), dim3(kThreads), 0, s, workspace,
                     chunks, cols, out);
  return check_launch("colsum");
}

extern "C" int cdml_fill_uniform_table_f16(uint16_t *table, int64_t row0, int64_t n_rows,
                                           int feature_size, int64_t row_stride, uint64_t seed,
                                           cdml_stream_t stream) {
  CDML_REQUIRE(table && n_rows > 0 && feature_size > 0 && row0 >= 0, CDML_E_BADARG,
               "fill_uniform_table_f16: bad argument");
  CDML_REQUIRE(row_stride >= feature_size && (row_stride & 7) == 0 && aligned16(table), CDML_E_ALIGN,
               "fill_uniform_table_f16: row_stride must be >= F and a multiple of 8");
  hipLaunchKernelGGL(k_fill_table_f16, dim3(grid1d(n_rows * (row_stride >> 2), 1)), dim3(kThreads), 0,
                     (hipStream_t)stream, reinterpret_cast<_Float16 *>(table), row0, n_rows, feature_size,
                     row_stride, seed);
  return check_launch("fill_uniform_table_f16");
}

extern "C" int cdml_gather_rows_f16(const uint16_t *table, int64_t row0, int64_t n_rows,
                                    int64_t row_stride, const int32_t *idx, int n_idx, int F,
                                    uint16_t *x_out_bf16, int64_t out_stride, int32_t *oob_flag,
                                    cdml_stream_t stream) {
  const GatherRowsArgs a = {table, row0, n_rows, row_stride, idx, n_idx, F, x_out_bf16, out_stride};
  GatherPlan p;
  if (int rc = plan_gather_rows("gather_rows_f16", kGatherF16, a, p)) return rc;
  const int rc = with_nch<kGatherF16, false>("gather_rows_f16", p.nch, [&](auto nch) {
    hipLaunchKernelGGL(k_gather_rows_f16<decltype(nch)::value>, dim3(p.grid), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const _Float16 *>(table), row0, n_rows, row_stride, idx, n_idx, F,
                       reinterpret_cast<bf16 *>(x_out_bf16), out_stride, oob_flag);
  });
  return rc ? rc : check_launch("gather_rows_f16");
}

// Triplet sampler + feature-row gather (+ fused input l2-normalise) for gfx950.
//
// Replaces the reference's host input pipe: MPTripletPipe.subprocess
// (inputs.py:102-142: pair stream + negative draw), get_batch's numpy
// fancy-index gather FEATURES[idx] (inputs.py:158), the reshape + feed_dict H2D
// copy (train.py:313,318) and the tower's first op tf.nn.l2_normalize
// (models.py:58).  The catalogue lives in HBM; nothing touches the host.
//
// Roofline: HBM.  Algorithmic bytes per gathered row = F*4 read + F*4 written.
// One wave owns one row: 16 B/lane loads (1 KiB per wave-instruction), all of
// a row's loads issued before the first use, wave-shuffle reduction for the
// norm.  Rows start 128-B aligned when row_stride*4 is a multiple of 128.
#include "common.h"
#include "gather_plan.h"
#include "../../include/cdml_hardneg.h"
#include "../../include/cdml_negweights.h"
#include "../../include/cdml_f8.h"

namespace cdml {
namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / kWave;

#ifndef CDML_GATHER_NT_STORE
#define CDML_GATHER_NT_STORE 0   // 1: non-temporal stores of the gathered rows
#endif
#ifndef CDML_GATHER_NT
#define CDML_GATHER_NT 1   // non-temporal table loads: a row is read once, keep it out of L2 / Infinity Cache
                           // (A/B on MI355X, 32 768 rows per launch: 5.3 -> 6.2 TB/s; profiles/r02_gather_variants.txt)
#endif
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float4 load_row_chunk(const float4 *p) {
#if CDML_GATHER_NT
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return *p;
#endif
}

// ---------------------------------------------------------------- table fill --
__global__ void __launch_bounds__(kThreads)
k_fill_table(float *__restrict__ table, int64_t row0, int64_t n_rows, int F,
             int64_t row_stride, uint64_t seed) {
  const int64_t q_per_row = row_stride >> 2;
  const int64_t total = n_rows * q_per_row;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lr = i / q_per_row;
    const int64_t q = i - lr * q_per_row;
    const uint64_t r = (uint64_t)(row0 + lr);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t j = q * 4;
    if (j < F) {
      u32x4 w = philox4x32_10(u32x4{(uint32_t)q, (uint32_t)r, (uint32_t)(r >> 32), kTableTag}, k0, k1);
      const float s = 5.9604644775390625e-08f;  // 2^-24
      v.x = (float)(w.x >> 8) * s;
      v.y = (j + 1 < F) ? (float)(w.y >> 8) * s : 0.f;
      v.z = (j + 2 < F) ? (float)(w.z >> 8) * s : 0.f;
      v.w = (j + 3 < F) ? (float)(w.w >> 8) * s : 0.f;
    }
    reinterpret_cast<float4 *>(table)[i] = v;
  }
}

// ------------------------------------------------------------------- sampler --
__global__ void __launch_bounds__(kThreads)
k_sample_uniform(const int32_t *__restrict__ pairs, int64_t n_pairs, uint32_t n_rows,
                 uint64_t seed, uint64_t step_imm, const uint64_t *__restrict__ step_dev,
                 int batch, int64_t slot0, int64_t batch_global, int32_t *__restrict__ idx_out) {
  const uint64_t step = step_imm + (step_dev ? *step_dev : 0);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const uint64_t slot = (uint64_t)(slot0 + i);
  const uint64_t q = (step * (uint64_t)batch_global + slot) % (uint64_t)n_pairs;
  const int32_t a = pairs[2 * q], p = pairs[2 * q + 1];
  const int32_t n = sample_uniform_negative(seed, step, (uint32_t)slot, a, p, n_rows);
  idx_out[3 * i + 0] = a;
  idx_out[3 * i + 1] = p;
  idx_out[3 * i + 2] = n;
}

// Listed ("hard") negatives (include/cdml_hardneg.h; host model: tests/hardneg_ref.py).  Word 0 of the purpose-2 stream
// decides hard or not; a hard draw takes its four list positions FIRST, so the four list loads do not depend on one
// another, and returns the first entry that is a catalogue row other than a and p.  Everything else is the uniform draw.
constexpr uint32_t kPurposeListedNeg = 2;
struct ListedNeg {
  const int32_t *lists = nullptr;   // [n_rows][ldl], L valid columns per row, -1 = empty
  int64_t ldl = 0;
  uint32_t L = 1;
  uint64_t hard_thresh = 0;         // round(hard_fraction * 2^32)
  int32_t *kind_out = nullptr;      // [n_steps][batch], steps kind_step_stride apart; null = not wanted
  int64_t kind_step_stride = 0;
};

__device__ __forceinline__ int32_t sample_listed_negative(uint64_t seed, uint64_t step, uint32_t slot, int32_t a, int32_t p,
                                                          uint32_t n_rows, const ListedNeg &ln, int32_t &kind) {
  WordStream hs(seed, step, slot, kPurposeListedNeg);
  const uint32_t w0 = hs.next();
  if ((uint64_t)w0 < ln.hard_thresh && a >= 0 && (uint32_t)a < n_rows) {
    int64_t j[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) j[t] = hs.bounded(ln.L);
    const int32_t *row = ln.lists + (int64_t)a * ln.ldl;
    int32_t c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = j[t] >= 0 ? row[j[t]] : -1;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (c[t] >= 0 && (uint32_t)c[t] < n_rows && c[t] != a && c[t] != p) {
        kind = 1;
        return c[t];
      }
  }
  kind = 0;
  return sample_uniform_negative(seed, step, slot, a, p, n_rows);
}

__global__ void __launch_bounds__(kThreads)
k_sample_listed(const int32_t *__restrict__ pairs, int64_t n_pairs, uint32_t n_rows, uint64_t seed, uint64_t step_imm,
                const uint64_t *__restrict__ step_dev, int batch, int64_t slot0, int64_t batch_global, ListedNeg ln,
                int32_t *__restrict__ idx_out) {
  const uint64_t step = step_imm + (step_dev ? *step_dev : 0);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const uint64_t slot = (uint64_t)(slot0 + i);
  const uint64_t q = (step * (uint64_t)batch_global + slot) % (uint64_t)n_pairs;
  const int32_t a = pairs[2 * q], p = pairs[2 * q + 1];
  int32_t kind;
  const int32_t n = sample_listed_negative(seed, step, (uint32_t)slot, a, p, n_rows, ln, kind);
  idx_out[3 * i + 0] = a;
  idx_out[3 * i + 1] = p;
  idx_out[3 * i + 2] = n;
  if (ln.kind_out) ln.kind_out[i] = kind;
}

// Weighted negatives (include/cdml_negweights.h; host model: tests/negweights_ref.py).  A 32-bit word r of the purpose-3
// stream falls into the interval of exactly one row: owner(r) = the largest v < n_live with start[v] <= r, found by one
// load of coarse[r >> shift] (the owners of the bucket's two ends bracket it) and a binary search in start[lo..hi].  A
// word that lands on a or p is redrawn; a stream that runs out leaves the triplet to the uniform draw.
constexpr uint32_t kPurposeWeightedNeg = 3;
struct WeightedNeg {
  const uint32_t *start = nullptr;  // [n_live] exclusive prefix sums of the quanta
  const int32_t *coarse = nullptr;  // [2^bits + 1]
  int32_t n_live = 1;
  int32_t shift = 16;               // 32 - bits
  int32_t *kind_out = nullptr;      // as ListedNeg's
  int64_t kind_step_stride = 0;
};

__device__ __forceinline__ int32_t weighted_owner(uint32_t r, const WeightedNeg &wn) {
  const uint32_t b = r >> wn.shift;
  const int32_t last = wn.n_live - 1;
  // the bounds are clamped into [0, n_live): a malformed table cannot index outside start
  int32_t lo = min(max(wn.coarse[b], 0), last);
  int32_t hi = min(max(wn.coarse[b + 1], lo), last);
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo + 1) >> 1);     // in (lo, hi]
    if (wn.start[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int32_t sample_weighted_negative(uint64_t seed, uint64_t step, uint32_t slot, int32_t a, int32_t p,
                                                            uint32_t n_rows, const WeightedNeg &wn, int32_t &kind) {
  WordStream hs(seed, step, slot, kPurposeWeightedNeg);
  while (!hs.exhausted()) {
    const int32_t v = weighted_owner(hs.next(), wn);
    if (v != a && v != p) {
      kind = 1;
      return v;
    }
  }
  kind = 0;
  return sample_uniform_negative(seed, step, slot, a, p, n_rows);
}

__global__ void __launch_bounds__(kThreads)
k_sample_weighted(const int32_t *__restrict__ pairs, int64_t n_pairs, uint32_t n_rows, uint64_t seed, uint64_t step_imm,
                  const uint64_t *__restrict__ step_dev, int batch, int64_t slot0, int64_t batch_global, WeightedNeg wn,
                  int32_t *__restrict__ idx_out) {
  const uint64_t step = step_imm + (step_dev ? *step_dev : 0);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const uint64_t slot = (uint64_t)(slot0 + i);
  const uint64_t q = (step * (uint64_t)batch_global + slot) % (uint64_t)n_pairs;
  const int32_t a = pairs[2 * q], p = pairs[2 * q + 1];
  int32_t kind;
  const int32_t n = sample_weighted_negative(seed, step, (uint32_t)slot, a, p, n_rows, wn, kind);
  idx_out[3 * i + 0] = a;
  idx_out[3 * i + 1] = p;
  idx_out[3 * i + 2] = n;
  if (wn.kind_out) wn.kind_out[i] = kind;
}

__global__ void __launch_bounds__(kThreads)
k_sample_inbatch(const int32_t *__restrict__ pairs, int64_t n_pairs, uint64_t seed,
                 uint64_t step_imm, const uint64_t *__restrict__ step_dev, int batch,
                 int64_t slot0, int64_t batch_global, int32_t *__restrict__ rows_out,
                 int32_t *__restrict__ shift_out) {
  const uint64_t step = step_imm + (step_dev ? *step_dev : 0);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *shift_out = sample_inbatch_shift(seed, step, batch);
  if (i >= batch) return;
  const uint64_t slot = (uint64_t)(slot0 + i);
  const uint64_t q = (step * (uint64_t)batch_global + slot) % (uint64_t)n_pairs;
  rows_out[2 * i + 0] = pairs[2 * q];
  rows_out[2 * i + 1] = pairs[2 * q + 1];
}

__global__ void k_step_advance(uint64_t *step_dev) { *step_dev += 1; }

// -------------------------------------------------------------------- gather --
// The arithmetic every fp32-table row shares, whatever it is stored as.  v: the row in registers, chunk c of lane l =
// columns 4 * (l + 64 c) .. + 3.
// The pad of the last chunk is masked, so the table's pad content never leaks in.
template <int NCH>
__device__ __forceinline__ void mask_row_pad(float4 (&v)[NCH], int F, int lane) {
  if (F & 3) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = 4 * (lane + kWave * c);
      if (j + 1 >= F && j < F) v[c].y = 0.f;
      if (j + 2 >= F && j < F) v[c].z = 0.f;
      if (j + 3 >= F && j < F) v[c].w = 0.f;
    }
  }
}

// 1 / max(|row|, 1e-6) of the (masked) row a wave holds
template <int NCH>
__device__ __forceinline__ float row_inv_norm(const float4 (&v)[NCH]) {
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    ss += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
  ss = wave_sum(ss);
  return 1.0f / sqrtf(fmaxf(ss, 1e-12f));
}

// The four ROUNDED products v * inv, the values the fp32 gather stores: what the plane formats split.  No contraction --
// a product fused with the residual subtraction of the split into an fma on the unrounded one gives other planes, and two
// evaluations contracted differently once moved a few rows by one ulp (RowF32X3::chunk_planes).
__device__ __forceinline__ void scaled4(const float4 &v, float inv, float (&r)[4]) {
#pragma clang fp contract(off)
  r[0] = v.x * inv, r[1] = v.y * inv, r[2] = v.z * inv, r[3] = v.w * inv;
}

// The next bf16 plane of four columns: r rounded, and r left holding the residual.  Three calls: hi | mid | lo with
// hi + mid + lo = r exactly (split3_bf16, four columns at a time).
template <typename V4>
__device__ __forceinline__ V4 next_plane4(float (&r)[4]) {
#pragma clang fp contract(off)
  V4 o;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    o[u] = (__bf16)r[u];
    r[u] -= (float)o[u];
  }
  return o;
}

// One wave gathers (and optionally l2-normalises) one row.  NCH = float4 chunks
// per lane held in registers (covers F <= 256*NCH).
template <int NCH>
__device__ __forceinline__ void gather_one_row(const float *__restrict__ table, int64_t local_row,
                                               int64_t row_stride, int F, int normalize,
                                               float *__restrict__ dst, int64_t out_stride,
                                               float *__restrict__ inv_out, int lane) {
  const float4 *src = reinterpret_cast<const float4 *>(table + local_row * row_stride);
  const int nq = (F + 3) >> 2;
  float4 v[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int q = lane + kWave * c;
    v[c] = (q < nq) ? load_row_chunk(src + q) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (F & 3) {  // (mask_row_pad, spelled out: through the helper this kernel's branch came out with the other polarity)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = 4 * (lane + kWave * c);
      if (j + 1 >= F && j < F) v[c].y = 0.f;
      if (j + 2 >= F && j < F) v[c].z = 0.f;
      if (j + 3 >= F && j < F) v[c].w = 0.f;
    }
  }
  float inv = 1.f;
  if (normalize) inv = row_inv_norm(v);
  if (inv_out && lane == 0) *inv_out = inv;
  float4 *d = reinterpret_cast<float4 *>(dst);
  const int oq = (int)(out_stride >> 2);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int q = lane + kWave * c;
    if (q < oq) d[q] = make_float4(v[c].x * inv, v[c].y * inv, v[c].z * inv, v[c].w * inv);
  }
  for (int q = lane + kWave * NCH; q < oq; q += kWave) d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ int64_t clamp_row(int32_t id, int64_t row0, int64_t n_rows,
                                             int32_t *oob_flag) {
  int64_t lr = (int64_t)id - row0;
  if (lr < 0 || lr >= n_rows) {
    if (oob_flag) atomicOr(oob_flag, 1);
    lr = lr < 0 ? 0 : n_rows - 1;
  }
  return lr;
}

template <int NCH>
__global__ void __launch_bounds__(kThreads)
k_gather_rows(const float *__restrict__ table, int64_t row0, int64_t n_rows, int64_t row_stride,
              const int32_t *__restrict__ idx, int n_idx, int F, int normalize,
              float *__restrict__ x_out, int64_t out_stride, float *__restrict__ inv_norm_out,
              int32_t *__restrict__ oob_flag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int r = blockIdx.x * kWavesPerBlock + wave; r < n_idx; r += gridDim.x * kWavesPerBlock) {
    const int32_t id = idx[r];
    if (id == -1) {
      // owner side of a fixed-capacity exchange: a padding slot, left untouched.  Requester side
      // (flag bit 1 set): a request that found no slot -- the row is filled with all-ones words
      // (NaN as fp32 and as bf16 pairs), so the same step's loss shows the overflow
      if (normalize & 2) {
        float4 *d = reinterpret_cast<float4 *>(x_out + (int64_t)r * out_stride);
        const float nanf_ = __uint_as_float(0xFFFFFFFFu);
        for (int q = lane; q < (int)(out_stride >> 2); q += kWave) d[q] = make_float4(nanf_, nanf_, nanf_, nanf_);
      }
      continue;
    }
    const int64_t lr = clamp_row(id, row0, n_rows, oob_flag);
    gather_one_row<NCH>(table, lr, row_stride, F, normalize & 1, x_out + (int64_t)r * out_stride,
                        out_stride, inv_norm_out ? inv_norm_out + r : nullptr, lane);
  }
}

// out planes[r] = the three bf16 planes hi | mid | lo of the fp32 row src[idx[r]] AS STORED (no normalisation): the last step
// of the row exchange on the split-fp32 path (round 5) -- the received rows go into request order and into the GEMMs' operand
// form in one pass on the prefetch stream, instead of fp32 rows there and a split launch on the compute stream every step.
// idx -1 (flag bit 1): a request that found no slot -> all-ones words (NaN in every plane), as k_gather_rows.
template <int NCH>
__global__ void __launch_bounds__(kThreads)
k_gather_rows_planes(const float *__restrict__ src, int64_t n_rows, int64_t row_stride, const int32_t *__restrict__ idx, int n_idx,
                     int F, int flags, __bf16 *__restrict__ out, int64_t out_stride, int32_t *__restrict__ oob_flag) {
  using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
  using u32x2v = __attribute__((ext_vector_type(2))) uint32_t;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t plane = out_stride / 3;
  const int oq = (int)(plane >> 2), nq = (F + 3) >> 2;
  for (int r = blockIdx.x * kWavesPerBlock + wave; r < n_idx; r += gridDim.x * kWavesPerBlock) {
    const int32_t id = idx[r];
    __bf16 *dst = out + (int64_t)r * out_stride;
    if (id == -1) {
      if (flags & 2)
        for (int q = lane; q < 3 * oq; q += kWave) *reinterpret_cast<u32x2v *>(dst + 4 * q) = u32x2v{0xFFFFFFFFu, 0xFFFFFFFFu};
      continue;
    }
    const int64_t lr = clamp_row(id, 0, n_rows, oob_flag);
    const float4 *s4 = reinterpret_cast<const float4 *>(src + lr * row_stride);
    float4 v[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      v[c] = (q < nq) ? s4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      if (q < oq) {
        float x[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
        if (F & 3) {                                        // the pad of the source row never leaks in
#pragma unroll
          for (int u = 0; u < 4; ++u) if (4 * q + u >= F) x[u] = 0.f;
        }
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<bf16x4v *>(dst + pl * plane + 4 * q) = next_plane4<bf16x4v>(x);
      }
    }
    const bf16x4v z4 = {0, 0, 0, 0};
    for (int q = lane + kWave * NCH; q < oq; q += kWave)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<bf16x4v *>(dst + pl * plane + 4 * q) = z4;
  }
}

// Persistent fused sampler + gather + input l2-normalise, one launch for n_steps consecutive
// training steps (the sampler is counter-based, so the triplets of step t+1 are known at step
// t; two or more steps per launch amortise the launch ramp and the ids -> row latency chain of
// a kernel that is otherwise only ~16 us of HBM traffic long).
//   * the launch's rows (n_steps x RPT x batch; RPT = 3 uniform or listed, 2 in-batch) are cut into
//     chunks of kChunkRows; a block walks chunks c, c + grid, ...;
//   * the ids of a chunk are produced once by the block's first lanes -- pair stream position,
//     pair load, the Philox negative where the row is one -- and STAGED IN LDS (also written to
//     idx_out); the ids of the NEXT chunk are computed while this chunk's row loads are in
//     flight (two LDS buffers);
//   * every wave then owns kRowsPerWave = 2 rows of the chunk: both rows' loads (NCH x 1 KiB
//     each, 16 B per lane = whole 128-B lines) are issued before the first use, then the
//     wave-shuffle norm and the stores.
// MODE 0 = uniform negatives, MODE 1 = in-batch negatives, MODE 2 = listed negatives (3 rows per triplet as MODE 0; only
// the id-staging lanes differ: the negative's lane reads the anchor's list, one more hop of the chain pair -> id -> row),
// MODE 3 = weighted negatives (as MODE 2, the hop being the search in the weight tables).  NEG: the struct of the mode's own
// arguments -- ListedNeg for modes 0 - 2 (their kernel arguments are what they were), WeightedNeg for mode 3.
constexpr int kRowsPerWave = CDML_GATHER_ROWS_PER_WAVE;   // (gather_plan.h, which sizes the grid by it)
constexpr int kChunkRows = kRowsPerWave * kWavesPerBlock;

template <int NCH>
struct RowRegs { float4 v[NCH]; };

template <int NCH>
__device__ __forceinline__ void row_issue(RowRegs<NCH> &R, const float *__restrict__ table, int64_t local_row,
                                          int64_t row_stride, int nq, int lane) {
  const float4 *src = reinterpret_cast<const float4 *>(table + local_row * row_stride);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int q = lane + kWave * c;
    R.v[c] = (q < nq) ? load_row_chunk(src + q) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// same arithmetic as gather_one_row (normalize = 1), on rows already in registers
template <int NCH>
__device__ __forceinline__ void row_finish(RowRegs<NCH> &R, int F, float *__restrict__ dst, int64_t out_stride,
                                           int lane) {
  mask_row_pad(R.v, F, lane);
  const float inv = row_inv_norm(R.v);
  float4 *d = reinterpret_cast<float4 *>(dst);
  const int oq = (int)(out_stride >> 2);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int q = lane + kWave * c;
    if (q < oq) {
#if CDML_GATHER_NT_STORE
      const f32x4 o = f32x4{R.v[c].x * inv, R.v[c].y * inv, R.v[c].z * inv, R.v[c].w * inv};
      __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(d + q));
#else
      d[q] = make_float4(R.v[c].x * inv, R.v[c].y * inv, R.v[c].z * inv, R.v[c].w * inv);
#endif
    }
  }
  for (int q = lane + kWave * NCH; q < oq; q += kWave) d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Row policies of the fused kernel: how a wave loads one catalogue row into registers and how it
// normalises and stores it.  RowF32: fp32 table -> fp32 rows (configs 1-3).  RowF16: fp16 table ->
// bf16 rows, fp32 arithmetic (config 4; same formulas as k_gather_rows_f16).
template <int NCH>
struct RowF32 {
  using In = float;
  using Out = float;
  using Regs = RowRegs<NCH>;
  static constexpr int kPerChunk = 4;          // elements per 16-B chunk
  static constexpr int kRows = kRowsPerWave;   // rows a wave keeps in flight (6 KB each)
  __device__ static __forceinline__ void issue(Regs &R, const In *table, int64_t lr, int64_t stride, int F, int lane) {
    row_issue<NCH>(R, table, lr, stride, (F + 3) >> 2, lane);
  }
  __device__ static __forceinline__ void finish(Regs &R, int F, Out *dst, int64_t out_stride, int lane) {
    row_finish<NCH>(R, F, dst, out_stride, lane);
  }
};

// RowF32X3: fp32 table -> the l2-normalised row as three bf16 planes hi | mid | lo (hi + mid + lo = the fp32 value,
// exactly; the split-fp32 GEMMs of gemm_bf16x3.hip read them) -- out_stride = 3 planes of out_stride / 3 columns.
template <int NCH>
struct RowF32X3 {
  using In = float;
  using Out = __bf16;
  using Regs = RowRegs<NCH>;
  static constexpr int kPerChunk = 4;
  static constexpr int kRows = kRowsPerWave;
  // The k8-interleaved copy (round 5; k_sample_gather's x_ki): after finish() the registers hold the row with its pad
  // masked; the planes of chunk c are recomputed from the SAME rounded products (same expression, no contraction) with the
  // norm factor finish() RETURNS -- a second evaluation of the sum of squares in the same kernel was contracted into fmas
  // differently from the first and moved a few rows' factor by one ulp (tests: the copy == the interleaved row-major planes).
  template <typename V4>
  __device__ static __forceinline__ void chunk_planes(const Regs &R, int c, float inv, V4 (&o)[3]) {
    float r[4];
    scaled4(R.v[c], inv, r);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) o[pl] = next_plane4<V4>(r);
  }
  __device__ static __forceinline__ void issue(Regs &R, const In *table, int64_t lr, int64_t stride, int F, int lane) {
    row_issue<NCH>(R, table, lr, stride, (F + 3) >> 2, lane);
  }
  __device__ static __forceinline__ float finish(Regs &R, int F, Out *dst, int64_t out_stride, int lane) {
    using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
    mask_row_pad(R.v, F, lane);
    const float inv = row_inv_norm(R.v);
    const int64_t plane = out_stride / 3;
    const int oq = (int)(plane >> 2);
    const bf16x4v z4 = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      if (q < oq) {
        float r[4];
        scaled4(R.v[c], inv, r);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          const bf16x4v o = next_plane4<bf16x4v>(r);
#if CDML_GATHER_NT_STORE
          __builtin_nontemporal_store(o, reinterpret_cast<bf16x4v *>(dst + pl * plane + 4 * q));
#else
          *reinterpret_cast<bf16x4v *>(dst + pl * plane + 4 * q) = o;
#endif
        }
      }
    }
    for (int q = lane + kWave * NCH; q < oq; q += kWave)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<bf16x4v *>(dst + pl * plane + 4 * q) = z4;
    return inv;
  }
};

// RowF32H2: fp32 table -> the l2-normalised row as TWO fp16 planes hi | lo of x_hat * 2^14 (precision "f16x2":
// gemm_f16x2_256.hip reads them).  |x_hat| <= 1, so the scale is a constant of the format (cdml.h: CDML_F16X2_X_SCALE) and
// nothing saturates; out_stride = 2 planes of out_stride / 2 columns: 6 000 B written per 1500-d row where the three bf16
// planes are 9 000.
constexpr float kH2XScale = 16384.f;
template <int NCH>
struct RowF32H2 {
  using In = float;
  using Out = _Float16;
  using Regs = RowRegs<NCH>;
  static constexpr int kPerChunk = 4;
  static constexpr int kRows = kRowsPerWave;
  __device__ static __forceinline__ void issue(Regs &R, const In *table, int64_t lr, int64_t stride, int F, int lane) {
    row_issue<NCH>(R, table, lr, stride, (F + 3) >> 2, lane);
  }
  __device__ static __forceinline__ void finish(Regs &R, int F, Out *dst, int64_t out_stride, int lane) {
    using half4v = __attribute__((ext_vector_type(4))) _Float16;
    mask_row_pad(R.v, F, lane);
    const float inv = row_inv_norm(R.v);
    const int64_t plane = out_stride / 2;
    const int oq = (int)(plane >> 2);
    const half4v z4 = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      if (q < oq) {
        // the planes are those of the ROUNDED product (scaled4: the value the fp32 gather stores) times 2^14, exactly; the
        // pragma is for the arithmetic BELOW -- r * 2^14 and the hi / lo residual must not be contracted either
#pragma clang fp contract(off)
        float r[4];
        scaled4(R.v[c], inv, r);
        half4v hi, lo;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float sv = r[u] * kH2XScale;
          hi[u] = (_Float16)sv;
          lo[u] = (_Float16)(sv - (float)hi[u]);
        }
#if CDML_GATHER_NT_STORE
        __builtin_nontemporal_store(hi, reinterpret_cast<half4v *>(dst + 4 * q));
        __builtin_nontemporal_store(lo, reinterpret_cast<half4v *>(dst + plane + 4 * q));
#else
        *reinterpret_cast<half4v *>(dst + 4 * q) = hi;
        *reinterpret_cast<half4v *>(dst + plane + 4 * q) = lo;
#endif
      }
    }
    for (int q = lane + kWave * NCH; q < oq; q += kWave) {
      *reinterpret_cast<half4v *>(dst + 4 * q) = z4;
      *reinterpret_cast<half4v *>(dst + plane + 4 * q) = z4;
    }
  }
};

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
template <int NCH>
struct RowF16 {
  using In = _Float16;
  using Out = __bf16;
  struct Regs { half8 v[NCH]; };
  static constexpr int kPerChunk = 8;
  static constexpr int kRows = CDML_GATHER_ROWS_PER_WAVE_F16;   // 3-KB rows: four in flight per wave
  __device__ static __forceinline__ void issue(Regs &R, const In *table, int64_t lr, int64_t stride, int F, int lane) {
    const half8 *src = reinterpret_cast<const half8 *>(table + lr * stride);
    const int nq = (F + 7) >> 3;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      half8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (q < nq) {
#if CDML_GATHER_NT
        x = __builtin_nontemporal_load(src + q);
#else
        x = src[q];
#endif
      }
      R.v[c] = x;
    }
  }
  __device__ static __forceinline__ void finish(Regs &R, int F, Out *dst, int64_t out_stride, int lane) {
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) ss = f16_chunk_sumsq(R.v[c], lane + kWave * c, F, ss);
    ss = wave_sum(ss);
    const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
    bf16x8v *d = reinterpret_cast<bf16x8v *>(dst);
    const int oq = (int)(out_stride >> 3);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      if (q < oq) {
        bf16x8v o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = (__bf16)((float)R.v[c][u] * inv);
#if CDML_GATHER_NT_STORE
        __builtin_nontemporal_store(o, d + q);
#else
        d[q] = o;
#endif
      }
    }
    const bf16x8v z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = lane + kWave * NCH; q < oq; q += kWave) d[q] = z8;
  }
};

// RowF8: fp8 (OCP e4m3) table -> bf16 rows (include/cdml_f8.h).  A lane keeps the EIGHT codes of its chunk (one 8-B load: 512
// contiguous bytes per wave instruction) -- the columns 8 (l + 64 c) .. + 7 a lane of RowF16 holds -- converts them exactly
// to fp16 (every e4m3 value is an fp16 value: v_cvt_pk_f32_fp8, then f32 -> f16 of a value with 3 mantissa bits and an
// exponent in [-9, 8]; a NaN code stays NaN) and hands the row to RowF16::finish: the same instructions in the same order,
// so the output is bit for bit that of the fp16 gather of the same values.  (A 16-B load per lane would change which
// columns a lane sums, hence the rounding of the sum of squares.)  The per-row scale cancels in the normalisation.
using u32x2c = __attribute__((ext_vector_type(2))) uint32_t;
using f32x2c = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ half8 f8x8_to_half8(u32x2c w) {
  half8 h;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const f32x2c lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[k], false);   // bytes 0, 1
    const f32x2c hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[k], true);    // bytes 2, 3
    h[4 * k + 0] = (_Float16)lo[0], h[4 * k + 1] = (_Float16)lo[1];
    h[4 * k + 2] = (_Float16)hi[0], h[4 * k + 3] = (_Float16)hi[1];
  }
  return h;
}

template <int NCH>
struct RowF8 {
  using In = uint8_t;
  using Out = __bf16;
  struct Regs { u32x2c v[NCH]; };
  static constexpr int kPerChunk = 8;
  static constexpr int kRows = CDML_GATHER_ROWS_PER_WAVE_F8;   // 1.5-KB rows, two registers per chunk while in flight
  __device__ static __forceinline__ void issue(Regs &R, const In *table, int64_t lr, int64_t stride, int F, int lane) {
    const u32x2c *src = reinterpret_cast<const u32x2c *>(table + lr * stride);
    const int nq = (F + 7) >> 3;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = lane + kWave * c;
      u32x2c x = {0u, 0u};
      if (q < nq) {
#if CDML_GATHER_NT
        x = __builtin_nontemporal_load(src + q);
#else
        x = src[q];
#endif
      }
      R.v[c] = x;
    }
  }
  __device__ static __forceinline__ void finish(Regs &R, int F, Out *dst, int64_t out_stride, int lane) {
    typename RowF16<NCH>::Regs H;
#pragma unroll
    for (int c = 0; c < NCH; ++c) H.v[c] = f8x8_to_half8(R.v[c]);
    RowF16<NCH>::finish(H, F, dst, out_stride, lane);
  }
};

// The unfused twin of k_gather_rows_f16 on the fp8 table: one wave per row, RowF8's load and arithmetic.  idx -1: a
// padding slot, left untouched.
template <int NCH>
__global__ void __launch_bounds__(kThreads)
k_gather_rows_f8(const uint8_t *__restrict__ table, int64_t row0, int64_t n_rows, int64_t row_stride,
                 const int32_t *__restrict__ idx, int n_idx, int F, __bf16 *__restrict__ x_out, int64_t out_stride,
                 int32_t *__restrict__ oob_flag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int r = blockIdx.x * kWavesPerBlock + wave; r < n_idx; r += gridDim.x * kWavesPerBlock) {
    const int32_t id = idx[r];
    if (id == -1) continue;
    const int64_t lr = clamp_row(id, row0, n_rows, oob_flag);
    typename RowF8<NCH>::Regs R;
    RowF8<NCH>::issue(R, table, lr, row_stride, F, lane);
    RowF8<NCH>::finish(R, F, x_out + (int64_t)r * out_stride, out_stride, lane);
  }
}

// KI (RowF32X3 only; round 5): the chunk's 8 rows = ONE row group of the k8-interleaved copy x_ki -- per step
// [3 planes][rows_per_step / 8][plane columns][8 rows] bf16, what the weight gradient's k-strided product reads with one
// 16-B LDS read per fragment (gemm_bf16_256.hip, KI).  After the row-major planes are stored the block walks the plane in
// slices of 256 columns: every wave drops its two rows' planes of the slice into 12 KiB of LDS as [plane][row][column]
// (8-B writes), then 192 threads each read one 4-column group of all 8 rows (8-B reads), transpose 8 x 4 in registers and
// store 4 x 16 B = 64 contiguous bytes of x_ki.
template <int MODE, typename ROW, bool KI = false, typename NEG = ListedNeg>
__global__ void __launch_bounds__(kThreads)
k_sample_gather(const int32_t *__restrict__ pairs, int64_t n_pairs, uint64_t seed,
                uint64_t step_imm, const uint64_t *__restrict__ step_dev, int batch,
                int64_t slot0, int64_t batch_global, const typename ROW::In *__restrict__ table,
                int64_t n_rows, int64_t row_stride, int F, int32_t *__restrict__ idx_out,
                int32_t *__restrict__ shift_out, typename ROW::Out *__restrict__ x_out, int64_t out_stride,
                int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                int32_t *__restrict__ oob_flag, __bf16 *__restrict__ x_ki = nullptr, int64_t ki_step_stride = 0,
                NEG ln = NEG()) {
  constexpr int RPT = (MODE == 1) ? 2 : 3;  // rows per triplet
  constexpr int kRPW = ROW::kRows, kCR = kRPW * kWavesPerBlock;   // rows per wave / per chunk
  __shared__ int32_t s_id[2][kCR];
  __shared__ __attribute__((aligned(16))) __bf16 s_il[KI ? 3 : 1][KI ? 8 : 1][KI ? 256 : 4];
  static_assert(!KI || kCR == 8, "the interleaved copy takes a chunk of 8 rows = one row group");
  const uint64_t step0 = step_imm + (step_dev ? *step_dev : 0);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t rows_per_step = (int64_t)RPT * batch;
  const int64_t total_rows = rows_per_step * n_steps;
  const int64_t n_chunks = (total_rows + kCR - 1) / kCR;

  // ids of chunk c -> LDS buffer b (threads 0..kCR-1), and to idx_out / shift_out
  auto stage_ids = [&](int64_t c, int b) {
    if (threadIdx.x < kCR) {
      const int64_t g = c * kCR + threadIdx.x;
      int32_t id = 0;
      if (g < total_rows) {
        const int s = (int)(g / rows_per_step);
        const int r = (int)(g - (int64_t)s * rows_per_step);
        const int i = r / RPT, k = r - i * RPT;
        const uint64_t step = step0 + (uint64_t)s;
        const uint64_t slot = (uint64_t)(slot0 + i);
        const uint64_t q = (step * (uint64_t)batch_global + slot) % (uint64_t)n_pairs;
        if (MODE == 0 && k == 2) {
          id = sample_uniform_negative(seed, step, (uint32_t)slot, pairs[2 * q], pairs[2 * q + 1], (uint32_t)n_rows);
        } else if (MODE == 2 && k == 2) {
          if constexpr (MODE == 2) {
            int32_t kind;
            id = sample_listed_negative(seed, step, (uint32_t)slot, pairs[2 * q], pairs[2 * q + 1], (uint32_t)n_rows, ln, kind);
            if (ln.kind_out) ln.kind_out[(int64_t)s * ln.kind_step_stride + i] = kind;
          }
        } else if (MODE == 3 && k == 2) {
          if constexpr (MODE == 3) {
            int32_t kind;
            id = sample_weighted_negative(seed, step, (uint32_t)slot, pairs[2 * q], pairs[2 * q + 1], (uint32_t)n_rows, ln, kind);
            if (ln.kind_out) ln.kind_out[(int64_t)s * ln.kind_step_stride + i] = kind;
          }
        } else {
          id = pairs[2 * q + (k ? 1 : 0)];
          // a pair id outside the catalogue (the reference raises IndexError, inputs.py:158): the row
          // load below clamps it for memory safety, the flag tells the caller (off the load path)
          if (oob_flag && (id < 0 || id >= n_rows)) atomicOr(oob_flag, 1);
        }
        idx_out[(int64_t)s * idx_step_stride + r] = id;
        if (MODE == 1 && r == 0) shift_out[s] = sample_inbatch_shift(seed, step, batch);
      }
      s_id[b][threadIdx.x] = id;
    }
  };

  int64_t c = blockIdx.x;
  if (c >= n_chunks) return;
  stage_ids(c, 0);
  __syncthreads();
  int b = 0;
  for (; c < n_chunks; c += gridDim.x, b ^= 1) {
    const int64_t g0 = c * kCR + wave * kRPW;
    typename ROW::Regs R[kRPW];
#pragma unroll
    for (int u = 0; u < kRPW; ++u) {
      const int32_t id = __builtin_amdgcn_readfirstlane(s_id[b][wave * kRPW + u]);
      if (g0 + u < total_rows) ROW::issue(R[u], table, clamp_row(id, 0, n_rows, nullptr), row_stride, F, lane);
    }
    const int64_t cn = c + gridDim.x;
    if (cn < n_chunks) stage_ids(cn, b ^ 1);       // under the row loads in flight
    float inv[KI ? kRPW : 1];
#pragma unroll
    for (int u = 0; u < kRPW; ++u) {
      const int64_t g = g0 + u;
      if (g < total_rows) {
        const int64_t s = g / rows_per_step, r = g - s * rows_per_step;
        if constexpr (KI) inv[u] = ROW::finish(R[u], F, x_out + s * x_step_stride + r * out_stride, out_stride, lane);
        else ROW::finish(R[u], F, x_out + s * x_step_stride + r * out_stride, out_stride, lane);
      }
    }
    if constexpr (KI) {
      using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
      using u32x2v = __attribute__((ext_vector_type(2))) uint32_t;
      using u32x4v = __attribute__((ext_vector_type(4))) uint32_t;
      // (host: rows_per_step % 8 == 0, so the chunk's 8 rows are whole, of one step, and one row group of it)
      const int64_t gc = c * kCR;
      const int64_t sidx = gc / rows_per_step;
      const int64_t kg = (gc - sidx * rows_per_step) >> 3, kgs = rows_per_step >> 3;
      const int plane = (int)(out_stride / 3);
      __bf16 *const kbase = x_ki + sidx * ki_step_stride;
      constexpr int kSlices = (int)(sizeof(R[0].v) / sizeof(R[0].v[0]));   // the row registers: NCH chunks of 256 columns
#pragma unroll
      for (int sl = 0; sl < kSlices; ++sl) {                            // chunk sl of the row registers = columns 256 sl .. + 255
        if (sl * 256 >= plane) break;                                  // (uniform)
#pragma unroll
        for (int u = 0; u < kRPW; ++u) {
          bf16x4v o[3];
          ROW::chunk_planes(R[u], sl, inv[u], o);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<bf16x4v *>(&s_il[pl][wave * kRPW + u][4 * lane]) = o[pl];
        }
        __syncthreads();
        if (threadIdx.x < 192) {
          const int pl = threadIdx.x >> 6, fg = threadIdx.x & 63;
          u32x2v in[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) in[j] = *reinterpret_cast<const u32x2v *>(&s_il[pl][j][4 * fg]);
          __bf16 *dstp = kbase + (((int64_t)pl * kgs + kg) * plane + sl * 256 + 4 * fg) * 8;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            u32x4v o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const uint32_t a = in[2 * k][e >> 1], b = in[2 * k + 1][e >> 1];
              o[k] = (e & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
            }
            *reinterpret_cast<u32x4v *>(dstp + e * 8) = o;
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();                               // ids of the next chunk are staged; this buffer is free
  }
}

// ------------------------------------------------ row exchange: routing (multi-GPU) --
// Row-sharded catalogue, fixed-capacity all-to-all (cdml_amd/dist.py): every rank sends each
// peer exactly `cap` id slots and gets `cap` row slots back, so nothing on the step path depends
// on a host-side count (enqueue-only, hipGraph-capturable).  k_route_rows puts request r of this
// rank (global id ids[r], owner = id / rows_per_shard) into the owner's segment of the send
// buffer in ASCENDING r (deterministic: the owner of a trainable table sums duplicate rows in the
// order it was asked), pads the rest with -1 and records the slot for the way back.  One block:
// R is a few 10^4 ids and the kernel sits on the prefetch stream, off the critical path.
constexpr int kRouteThreads = 1024;
constexpr int kRouteMaxWorld = 64;

__global__ void __launch_bounds__(kRouteThreads)
k_route_rows(const int32_t *__restrict__ ids, int n, int64_t rows_per_shard, int world, int cap,
             int32_t *__restrict__ send_ids, int32_t *__restrict__ slot, int32_t *__restrict__ overflow) {
  __shared__ int s_cnt[kRouteMaxWorld];
  __shared__ int s_wave[kRouteThreads / kWave][kRouteMaxWorld];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  for (int i = tid; i < world * cap; i += kRouteThreads) send_ids[i] = -1;
  if (tid < world) s_cnt[tid] = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kRouteThreads) {
    const int r = base + tid;
    int id = 0, o = -1;
    if (r < n) {
      id = ids[r];
      const int64_t q = (int64_t)id / rows_per_shard;
      if (id < 0 || q >= world) { atomicOr(overflow, 2); o = -1; }     // not a catalogue row
      else o = (int)q;
    }
    int my_rank = 0;
    for (int ow = 0; ow < world; ++ow) {
      const unsigned long long m = __ballot(o == ow);
      if (o == ow) my_rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_wave[wave][ow] = __popcll(m);
    }
    __syncthreads();
    if (o >= 0) {
      int pos = s_cnt[o] + my_rank;
      for (int w = 0; w < wave; ++w) pos += s_wave[w][o];
      if (pos < cap) {
        send_ids[o * cap + pos] = id;
        slot[r] = o * cap + pos;
      } else {
        slot[r] = -1;                                                  // the row is not fetched: fatal, flagged
        atomicOr(overflow, 1);
      }
    } else if (r < n) {
      slot[r] = -1;
    }
    __syncthreads();
    if (tid < world) {
      int c = s_cnt[tid];
      for (int w = 0; w < kRouteThreads / kWave; ++w) c += s_wave[w][tid];
      s_cnt[tid] = c;
    }
    __syncthreads();
  }
}

// dst[slot[r]] = src[r] for r < n (slot -1: dropped): the reverse trip of the exchange (row
// gradients to their owners).  One wave per row, 16-B lanes.
__global__ void __launch_bounds__(kThreads)
k_scatter_rows(const float *__restrict__ src, int64_t lds, const int32_t *__restrict__ slot, int n, int width,
               float *__restrict__ dst, int64_t ldd) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int nq = width >> 2;
  for (int r = blockIdx.x * kWavesPerBlock + wave; r < n; r += gridDim.x * kWavesPerBlock) {
    const int t = slot[r];
    if (t < 0) continue;
    const float4 *a = reinterpret_cast<const float4 *>(src + (int64_t)r * lds);
    float4 *d = reinterpret_cast<float4 *>(dst + (int64_t)t * ldd);
    for (int q = lane; q < nq; q += kWave) d[q] = a[q];
  }
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_fill_uniform_table(float *table, int64_t row0, int64_t n_rows, int feature_size,
                                       int64_t row_stride, uint64_t seed, cdml_stream_t stream) {
  CDML_REQUIRE(table && n_rows > 0 && feature_size > 0 && row0 >= 0, CDML_E_BADARG,
               "fill_uniform_table: bad argument");
  CDML_REQUIRE(row_stride >= feature_size && (row_stride & 3) == 0 && aligned16(table), CDML_E_ALIGN,
               "fill_uniform_table: row_stride must be >= F and a multiple of 4, base 16-B aligned");
  const int64_t total = n_rows * (row_stride >> 2);
  hipLaunchKernelGGL(k_fill_table, dim3(grid_for(total, kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, table, row0, n_rows, feature_size, row_stride, seed);
  return check_launch("fill_uniform_table");
}

extern "C" int cdml_sample_uniform(const int32_t *pairs, int64_t n_pairs, int64_t n_rows,
                                   uint64_t seed, uint64_t step, const uint64_t *step_dev,
                                   int batch, int64_t slot0, int64_t batch_global,
                                   int32_t *idx_out, cdml_stream_t stream) {
  CDML_REQUIRE(pairs && idx_out && n_pairs > 0 && batch > 0 && slot0 >= 0, CDML_E_BADARG,
               "sample_uniform: bad argument");
  CDML_REQUIRE(n_rows >= 3 && n_rows <= 0x7FFFFFFFll, CDML_E_BADARG,
               "sample_uniform: n_rows must be in [3, 2^31)");
  CDML_REQUIRE(batch_global >= slot0 + batch, CDML_E_BADARG,
               "sample_uniform: batch_global < slot0 + batch");
  hipLaunchKernelGGL(k_sample_uniform, dim3((batch + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     (hipStream_t)stream, pairs, n_pairs, (uint32_t)n_rows, seed, step, step_dev,
                     batch, slot0, batch_global, idx_out);
  return check_launch("sample_uniform");
}

extern "C" int cdml_sample_listed(const int32_t *pairs, int64_t n_pairs, int64_t n_rows, uint64_t seed, uint64_t step,
                                  const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                  const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh, int32_t *idx_out,
                                  int32_t *kind_out, cdml_stream_t stream) {
  CDML_REQUIRE(pairs && idx_out && n_pairs > 0 && batch > 0 && slot0 >= 0, CDML_E_BADARG, "sample_listed: bad argument");
  CDML_REQUIRE(n_rows >= 3 && n_rows <= 0x7FFFFFFFll, CDML_E_BADARG, "sample_listed: n_rows must be in [3, 2^31)");
  CDML_REQUIRE(batch_global >= slot0 + batch, CDML_E_BADARG, "sample_listed: batch_global < slot0 + batch");
  int rc = check_listed("sample_listed", lists, ldl, L, hard_thresh);
  if (rc) return rc;
  ListedNeg ln;
  ln.lists = lists, ln.ldl = ldl, ln.L = (uint32_t)L, ln.hard_thresh = hard_thresh, ln.kind_out = kind_out;
  hipLaunchKernelGGL(k_sample_listed, dim3((batch + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     pairs, n_pairs, (uint32_t)n_rows, seed, step, step_dev, batch, slot0, batch_global, ln, idx_out);
  return check_launch("sample_listed");
}

extern "C" int cdml_sample_weighted(const int32_t *pairs, int64_t n_pairs, int64_t n_rows, uint64_t seed, uint64_t step,
                                    const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                    const int32_t *start, int64_t n_live, const int32_t *coarse, int bits, int32_t *idx_out,
                                    int32_t *kind_out, cdml_stream_t stream) {
  CDML_REQUIRE(pairs && idx_out && n_pairs > 0 && batch > 0 && slot0 >= 0, CDML_E_BADARG, "sample_weighted: bad argument");
  CDML_REQUIRE(n_rows >= 3 && n_rows <= 0x7FFFFFFFll, CDML_E_BADARG, "sample_weighted: n_rows must be in [3, 2^31)");
  CDML_REQUIRE(batch_global >= slot0 + batch, CDML_E_BADARG, "sample_weighted: batch_global < slot0 + batch");
  int rc = check_weighted("sample_weighted", start, coarse, n_live, n_rows, bits);
  if (rc) return rc;
  WeightedNeg wn;
  wn.start = reinterpret_cast<const uint32_t *>(start), wn.coarse = coarse, wn.n_live = (int32_t)n_live, wn.shift = 32 - bits;
  wn.kind_out = kind_out;
  hipLaunchKernelGGL(k_sample_weighted, dim3((batch + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     pairs, n_pairs, (uint32_t)n_rows, seed, step, step_dev, batch, slot0, batch_global, wn, idx_out);
  return check_launch("sample_weighted");
}

extern "C" int cdml_sample_inbatch(const int32_t *pairs, int64_t n_pairs, uint64_t seed,
                                   uint64_t step, const uint64_t *step_dev, int batch,
                                   int64_t slot0, int64_t batch_global, int32_t *rows_out,
                                   int32_t *shift_out, cdml_stream_t stream) {
  CDML_REQUIRE(pairs && rows_out && shift_out && n_pairs > 0 && slot0 >= 0, CDML_E_BADARG,
               "sample_inbatch: bad argument");
  CDML_REQUIRE(batch >= 2, CDML_E_BADARG, "sample_inbatch: in-batch negatives need batch >= 2");
  CDML_REQUIRE(batch_global >= slot0 + batch, CDML_E_BADARG,
               "sample_inbatch: batch_global < slot0 + batch");
  hipLaunchKernelGGL(k_sample_inbatch, dim3((batch + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     (hipStream_t)stream, pairs, n_pairs, seed, step, step_dev, batch, slot0,
                     batch_global, rows_out, shift_out);
  return check_launch("sample_inbatch");
}

extern "C" int cdml_step_advance(uint64_t *step_dev, cdml_stream_t stream) {
  CDML_REQUIRE(step_dev, CDML_E_BADARG, "step_advance: null pointer");
  hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
  return check_launch("step_advance");
}

// ---- the gather launches: gather_plan.h checks the call and plans it, the launcher picks the instantiation the plan names ----
static_assert(kWave == kGatherWave && kWavesPerBlock == kGatherWavesPerBlock, "gather_plan.h plans for these blocks");

extern "C" int cdml_gather_rows(const float *table, int64_t row0, int64_t n_rows, int64_t row_stride,
                                const int32_t *idx, int n_idx, int F, int normalize, float *x_out,
                                int64_t out_stride, float *inv_norm_out, int32_t *oob_flag,
                                cdml_stream_t stream) {
  const GatherRowsArgs a = {table, row0, n_rows, row_stride, idx, n_idx, F, x_out, out_stride};
  GatherPlan p;
  if (int rc = plan_gather_rows("gather_rows", kGatherF32, a, p)) return rc;
  const int rc = with_nch<kGatherF32, false>("gather_rows", p.nch, [&](auto nch) {
    hipLaunchKernelGGL(k_gather_rows<decltype(nch)::value>, dim3(p.grid), dim3(kThreads), 0, (hipStream_t)stream, table, row0,
                       n_rows, row_stride, idx, n_idx, F, normalize, x_out, out_stride, inv_norm_out, oob_flag);
  });
  return rc ? rc : check_launch("gather_rows");
}

// rows AS STORED (fp32, e.g. the receive buffer of the row exchange) -> request order AND the three bf16 planes of the split-fp32
// GEMMs: x_out_planes[r] = planes of src[idx[r]] (out_stride = 3 planes of out_stride / 3 >= F columns); flags bit 1: idx -1 =
// a request that found no slot -> NaN planes (else: left untouched).
extern "C" int cdml_gather_rows_x3(const float *src, int64_t n_rows, int64_t row_stride, const int32_t *idx, int n_idx, int F,
                                   int flags, uint16_t *x_out_planes, int64_t out_stride, int32_t *oob_flag,
                                   cdml_stream_t stream) {
  const GatherRowsArgs a = {src, 0, n_rows, row_stride, idx, n_idx, F, x_out_planes, out_stride};
  GatherPlan p;
  if (int rc = plan_gather_rows("gather_rows_x3", kGatherX3, a, p)) return rc;
  const int rc = with_nch<kGatherX3, false>("gather_rows_x3", p.nch, [&](auto nch) {
    hipLaunchKernelGGL(k_gather_rows_planes<decltype(nch)::value>, dim3(p.grid), dim3(kThreads), 0, (hipStream_t)stream, src, n_rows,
                       row_stride, idx, n_idx, F, flags, reinterpret_cast<__bf16 *>(x_out_planes), out_stride, oob_flag);
  });
  return rc ? rc : check_launch("gather_rows_x3");
}

// The fused launch of one row format: k_sample_gather<MODE, ROW<NCH>, KI> for the plan's mode, bucket and interleaved copy.
// Modes 2 and 3 and KI are instantiated only for the formats that have them.
template <const GatherFormat &FMT, template <int> class ROW>
static int sample_gather(const char *who, const SampleGatherArgs &a, cdml_stream_t stream) {
  static_assert(ROW<8>::kRows * kWavesPerBlock == FMT.rows_per_chunk && ROW<8>::kPerChunk == FMT.per_chunk,
                "the format describes these row policies");
  GatherPlan p;
  if (int rc = plan_sample_gather(who, FMT, a, p)) return rc;
  ListedNeg ln;
  if (a.listed) {
    ln.lists = a.listed->lists, ln.ldl = a.listed->ldl, ln.L = (uint32_t)a.listed->L, ln.hard_thresh = a.listed->hard_thresh;
    ln.kind_out = a.listed->kind_out, ln.kind_step_stride = a.listed->kind_step_stride;
  }
  WeightedNeg wn;
  if (a.weighted) {
    wn.start = reinterpret_cast<const uint32_t *>(a.weighted->start), wn.coarse = a.weighted->coarse;
    wn.n_live = (int32_t)a.weighted->n_live, wn.shift = 32 - a.weighted->bits;
    wn.kind_out = a.weighted->kind_out, wn.kind_step_stride = a.weighted->kind_step_stride;
  }
  auto launch = [&](auto mode, auto ki, auto ln) {
    return with_nch<FMT, true>(who, p.nch, [&](auto nch) {
      using Row = ROW<decltype(nch)::value>;
      hipLaunchKernelGGL((k_sample_gather<decltype(mode)::value, Row, decltype(ki)::value, decltype(ln)>), dim3(p.grid), dim3(kThreads), 0,
                         (hipStream_t)stream, a.pairs, a.n_pairs, a.seed, a.step, a.step_dev, a.batch, a.slot0, a.batch_global,
                         static_cast<const typename Row::In *>(a.table), a.n_rows, a.row_stride, a.F, a.idx_out, a.shift_out,
                         static_cast<typename Row::Out *>(a.x_out), a.out_stride, a.n_steps, a.x_step_stride, a.idx_step_stride,
                         a.oob_flag, static_cast<__bf16 *>(a.x_ki), a.ki_step_stride, ln);
    });
  };
  auto by_mode = [&](auto ki) {
    if (a.mode == 0) return launch(std::integral_constant<int, 0>{}, ki, ln);
    if (a.mode == 1) return launch(std::integral_constant<int, 1>{}, ki, ln);
    if constexpr (FMT.who_listed != nullptr) {
      if (a.mode == 2) return launch(std::integral_constant<int, 2>{}, ki, ln);
      return launch(std::integral_constant<int, 3>{}, ki, wn);
    }
    return fail(CDML_E_UNSUPPORTED, "%s: no kernel for mode %d", who, a.mode);      // (the plan refuses it first)
  };
  int rc;
  if constexpr (FMT.ki) rc = p.ki ? by_mode(std::true_type{}) : by_mode(std::false_type{});
  else rc = by_mode(std::false_type{});
  return rc ? rc : check_launch(who);
}

// The eight fused entry points: fill the struct, plan, launch.  (x_out: fp32 rows | bf16 [rows][3 planes of out_stride / 3 >= F
// columns] (precision "f32x3") | fp16 [rows][2 planes of x_hat * 2^14] (precision "f16x2") | bf16 rows of an fp16 table.)
extern "C" int cdml_sample_gather(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed,
                                  uint64_t step, const uint64_t *step_dev, int batch, int64_t slot0,
                                  int64_t batch_global, const float *table, int64_t n_rows,
                                  int64_t row_stride, int F, int32_t *idx_out, int32_t *shift_out,
                                  float *x_out, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                  int64_t idx_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const SampleGatherArgs a = {mode, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, shift_out, x_out, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr};
  return sample_gather<kGatherF32, RowF32>("sample_gather", a, stream);
}

extern "C" int cdml_sample_gather_x3(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed,
                                     uint64_t step, const uint64_t *step_dev, int batch, int64_t slot0,
                                     int64_t batch_global, const float *table, int64_t n_rows,
                                     int64_t row_stride, int F, int32_t *idx_out, int32_t *shift_out,
                                     uint16_t *x_out_planes, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                     int64_t idx_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const SampleGatherArgs a = {mode, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, shift_out, x_out_planes, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr};
  return sample_gather<kGatherX3, RowF32X3>("sample_gather_x3", a, stream);
}

// cdml_sample_gather_x3 that ALSO writes every step's rows k8-interleaved (x_ki: bf16 [3][rows per step / 8][out_stride / 3][8]
// per step, steps ki_step_stride elements apart): the operand layout of cdml_gemm_bf16x3_tnk
extern "C" int cdml_sample_gather_x3k(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed,
                                      uint64_t step, const uint64_t *step_dev, int batch, int64_t slot0,
                                      int64_t batch_global, const float *table, int64_t n_rows,
                                      int64_t row_stride, int F, int32_t *idx_out, int32_t *shift_out,
                                      uint16_t *x_out_planes, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                      int64_t idx_step_stride, int32_t *oob_flag, uint16_t *x_ki, int64_t ki_step_stride,
                                      cdml_stream_t stream) {
  const SampleGatherArgs a = {mode, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, shift_out, x_out_planes, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              x_ki, ki_step_stride, true, nullptr};
  return sample_gather<kGatherX3, RowF32X3>("sample_gather_x3", a, stream);
}

extern "C" int cdml_sample_gather_h2(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed,
                                     uint64_t step, const uint64_t *step_dev, int batch, int64_t slot0,
                                     int64_t batch_global, const float *table, int64_t n_rows,
                                     int64_t row_stride, int F, int32_t *idx_out, int32_t *shift_out,
                                     uint16_t *x_out_planes, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                     int64_t idx_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const SampleGatherArgs a = {mode, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, shift_out, x_out_planes, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr};
  return sample_gather<kGatherH2, RowF32H2>("sample_gather_h2", a, stream);
}

extern "C" int cdml_sample_gather_f16(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed,
                                      uint64_t step, const uint64_t *step_dev, int batch, int64_t slot0,
                                      int64_t batch_global, const uint16_t *table, int64_t n_rows,
                                      int64_t row_stride, int F, int32_t *idx_out, int32_t *shift_out,
                                      uint16_t *x_out_bf16, int64_t out_stride, int n_steps,
                                      int64_t x_step_stride, int64_t idx_step_stride, int32_t *oob_flag,
                                      cdml_stream_t stream) {
  const SampleGatherArgs a = {mode, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, shift_out, x_out_bf16, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr};
  return sample_gather<kGatherF16, RowF16>("sample_gather_f16", a, stream);
}

// ---- listed negatives (include/cdml_hardneg.h): the fused launch in sampler mode 2, one entry point per row format that has
// one; the common checks report under the format's unlisted name ----
extern "C" int cdml_sample_gather_listed(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                         const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                         const float *table, int64_t n_rows, int64_t row_stride, int F,
                                         const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh, int32_t *idx_out,
                                         int32_t *kind_out, float *x_out, int64_t out_stride, int n_steps,
                                         int64_t x_step_stride, int64_t idx_step_stride, int64_t kind_step_stride,
                                         int32_t *oob_flag, cdml_stream_t stream) {
  const ListedArgs l = {lists, ldl, L, hard_thresh, kind_out, kind_step_stride};
  const SampleGatherArgs a = {2, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, &l};
  return sample_gather<kGatherF32, RowF32>("sample_gather", a, stream);
}

// three-plane rows; x_ki null = no k8-interleaved copy (cdml_sample_gather_x3's form), else _x3k's
extern "C" int cdml_sample_gather_listed_x3(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                            const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                            const float *table, int64_t n_rows, int64_t row_stride, int F,
                                            const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh,
                                            int32_t *idx_out, int32_t *kind_out, uint16_t *x_out_planes, int64_t out_stride,
                                            int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                                            int64_t kind_step_stride, int32_t *oob_flag, uint16_t *x_ki,
                                            int64_t ki_step_stride, cdml_stream_t stream) {
  const ListedArgs l = {lists, ldl, L, hard_thresh, kind_out, kind_step_stride};
  const SampleGatherArgs a = {2, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out_planes, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              x_ki, ki_step_stride, false, &l};
  return sample_gather<kGatherX3, RowF32X3>("sample_gather_x3", a, stream);
}

// fp16 table -> bf16 rows
extern "C" int cdml_sample_gather_listed_f16(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                             const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                             const uint16_t *table, int64_t n_rows, int64_t row_stride, int F,
                                             const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh,
                                             int32_t *idx_out, int32_t *kind_out, uint16_t *x_out_bf16, int64_t out_stride,
                                             int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                                             int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const ListedArgs l = {lists, ldl, L, hard_thresh, kind_out, kind_step_stride};
  const SampleGatherArgs a = {2, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out_bf16, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, &l};
  return sample_gather<kGatherF16, RowF16>("sample_gather_f16", a, stream);
}

// ---- weighted negatives (include/cdml_negweights.h): the fused launch in sampler mode 3, the listed entry points' twins ----
extern "C" int cdml_sample_gather_weighted(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                           const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                           const float *table, int64_t n_rows, int64_t row_stride, int F,
                                           const int32_t *start, int64_t n_live, const int32_t *coarse, int bits,
                                           int32_t *idx_out, int32_t *kind_out, float *x_out, int64_t out_stride, int n_steps,
                                           int64_t x_step_stride, int64_t idx_step_stride, int64_t kind_step_stride,
                                           int32_t *oob_flag, cdml_stream_t stream) {
  const WeightedArgs w = {"sample_gather_weighted", start, coarse, n_live, bits, kind_out, kind_step_stride};
  const SampleGatherArgs a = {3, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr, &w};
  return sample_gather<kGatherF32, RowF32>("sample_gather", a, stream);
}

// three-plane rows; x_ki null = no k8-interleaved copy
extern "C" int cdml_sample_gather_weighted_x3(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                              const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                              const float *table, int64_t n_rows, int64_t row_stride, int F,
                                              const int32_t *start, int64_t n_live, const int32_t *coarse, int bits,
                                              int32_t *idx_out, int32_t *kind_out, uint16_t *x_out_planes, int64_t out_stride,
                                              int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                                              int64_t kind_step_stride, int32_t *oob_flag, uint16_t *x_ki,
                                              int64_t ki_step_stride, cdml_stream_t stream) {
  const WeightedArgs w = {"sample_gather_weighted_x3", start, coarse, n_live, bits, kind_out, kind_step_stride};
  const SampleGatherArgs a = {3, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out_planes, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              x_ki, ki_step_stride, false, nullptr, &w};
  return sample_gather<kGatherX3, RowF32X3>("sample_gather_x3", a, stream);
}

// fp16 table -> bf16 rows
extern "C" int cdml_sample_gather_weighted_f16(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                               const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                               const uint16_t *table, int64_t n_rows, int64_t row_stride, int F,
                                               const int32_t *start, int64_t n_live, const int32_t *coarse, int bits,
                                               int32_t *idx_out, int32_t *kind_out, uint16_t *x_out_bf16, int64_t out_stride,
                                               int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                                               int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const WeightedArgs w = {"sample_gather_weighted_f16", start, coarse, n_live, bits, kind_out, kind_step_stride};
  const SampleGatherArgs a = {3, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out_bf16, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr, &w};
  return sample_gather<kGatherF16, RowF16>("sample_gather_f16", a, stream);
}

// ---- the fp8 catalogue (include/cdml_f8.h): e4m3 codes -> bf16 rows, the _f16 entry points' twins ----
extern "C" int cdml_gather_rows_f8(const uint8_t *table, int64_t row0, int64_t n_rows, int64_t row_stride, const int32_t *idx,
                                   int n_idx, int F, uint16_t *x_out_bf16, int64_t out_stride, int32_t *oob_flag,
                                   cdml_stream_t stream) {
  const GatherRowsArgs a = {table, row0, n_rows, row_stride, idx, n_idx, F, x_out_bf16, out_stride};
  GatherPlan p;
  if (int rc = plan_gather_rows("gather_rows_f8", kGatherF8, a, p)) return rc;
  const int rc = with_nch<kGatherF8, false>("gather_rows_f8", p.nch, [&](auto nch) {
    hipLaunchKernelGGL(k_gather_rows_f8<decltype(nch)::value>, dim3(p.grid), dim3(kThreads), 0, (hipStream_t)stream, table, row0,
                       n_rows, row_stride, idx, n_idx, F, reinterpret_cast<__bf16 *>(x_out_bf16), out_stride, oob_flag);
  });
  return rc ? rc : check_launch("gather_rows_f8");
}

extern "C" int cdml_sample_gather_f8(int mode, const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                     const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                     const uint8_t *table, int64_t n_rows, int64_t row_stride, int F, int32_t *idx_out,
                                     int32_t *shift_out, uint16_t *x_out_bf16, int64_t out_stride, int n_steps,
                                     int64_t x_step_stride, int64_t idx_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const SampleGatherArgs a = {mode, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, shift_out, x_out_bf16, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr};
  return sample_gather<kGatherF8, RowF8>("sample_gather_f8", a, stream);
}

extern "C" int cdml_sample_gather_listed_f8(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                            const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                            const uint8_t *table, int64_t n_rows, int64_t row_stride, int F,
                                            const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh,
                                            int32_t *idx_out, int32_t *kind_out, uint16_t *x_out_bf16, int64_t out_stride,
                                            int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                                            int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const ListedArgs l = {lists, ldl, L, hard_thresh, kind_out, kind_step_stride};
  const SampleGatherArgs a = {2, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out_bf16, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, &l};
  return sample_gather<kGatherF8, RowF8>("sample_gather_f8", a, stream);
}

extern "C" int cdml_sample_gather_weighted_f8(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                              const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                              const uint8_t *table, int64_t n_rows, int64_t row_stride, int F,
                                              const int32_t *start, int64_t n_live, const int32_t *coarse, int bits,
                                              int32_t *idx_out, int32_t *kind_out, uint16_t *x_out_bf16, int64_t out_stride,
                                              int n_steps, int64_t x_step_stride, int64_t idx_step_stride,
                                              int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream) {
  const WeightedArgs w = {"sample_gather_weighted_f8", start, coarse, n_live, bits, kind_out, kind_step_stride};
  const SampleGatherArgs a = {3, pairs, n_pairs, seed, step, step_dev, batch, slot0, batch_global, table, n_rows, row_stride, F,
                              idx_out, nullptr, x_out_bf16, out_stride, n_steps, x_step_stride, idx_step_stride, oob_flag,
                              nullptr, 0, false, nullptr, &w};
  return sample_gather<kGatherF8, RowF8>("sample_gather_f8", a, stream);
}

extern "C" int cdml_route_rows(const int32_t *ids, int n, int64_t rows_per_shard, int world, int capacity,
                               int32_t *send_ids, int32_t *slot_out, int32_t *overflow_flag,
                               cdml_stream_t stream) {
  CDML_REQUIRE(ids && send_ids && slot_out && overflow_flag && n > 0 && rows_per_shard > 0 && capacity > 0,
               CDML_E_BADARG, "route_rows: bad argument");
  CDML_REQUIRE(world >= 1 && world <= kRouteMaxWorld, CDML_E_UNSUPPORTED, "route_rows: world size %d outside [1, %d]",
               world, kRouteMaxWorld);
  hipLaunchKernelGGL(k_route_rows, dim3(1), dim3(kRouteThreads), 0, (hipStream_t)stream, ids, n, rows_per_shard,
                     world, capacity, send_ids, slot_out, overflow_flag);
  return check_launch("route_rows");
}

extern "C" int cdml_scatter_rows(const float *src, int64_t ld_src, const int32_t *slot, int n, int width,
                                 float *dst, int64_t ld_dst, cdml_stream_t stream) {
  CDML_REQUIRE(src && slot && dst && n > 0 && width > 0, CDML_E_BADARG, "scatter_rows: bad argument");
  CDML_REQUIRE((width & 3) == 0 && ld_src >= width && ld_dst >= width && (ld_src & 3) == 0 && (ld_dst & 3) == 0 &&
                   aligned16(src) && aligned16(dst),
               CDML_E_ALIGN, "scatter_rows: width and leading dimensions multiples of 4, 16-B aligned bases");
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid_for(n, kWavesPerBlock)), dim3(kThreads), 0, (hipStream_t)stream, src,
                     ld_src, slot, n, width, dst, ld_dst);
  return check_launch("scatter_rows");
}

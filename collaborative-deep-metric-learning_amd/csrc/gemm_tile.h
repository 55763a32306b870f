// What the 256 x 256 tile GEMM (gemm_bf16_256.hip; gemm_f16x2_256.hip compiles it again under CDML_F16X2) is written in:
// the vector types, the tile and LDS-image constants, the LDS-DMA and 16-bit packing helpers, the barrier, the compile-time
// unroll helper, and Variant -- the one traits type that names a variant of the kernel.  Everything here is internal to a
// translation unit (anonymous namespace).
#pragma once
#include "gemm_bf16.h"
#include <type_traits>
#include <utility>

namespace cdml {
namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int kT = 512;
constexpr int kTileM = 256, kTileN = 256, kTileK = 64;
constexpr int IMG = 16384;       // one half image: 128 rows x 128 B
constexpr int BUF = 4 * IMG;     // one K-tile: A-h0, A-h1, B-h0, B-h1
// LDS by OPERAND: [A: buf0 h0 | buf0 h1 | buf1 h0 | buf1 h1][B: likewise] (round 4; rounds 1-3 laid it out by buffer).  Every
// fragment read of an operand is then within 64 KiB of ONE lane base, i.e. inside the 16-bit offset immediate of a ds_read:
// the second buffer costs no v_add per read (k-strided form: 24 fewer VALU per K-tile, -2 % measured) and no second set
// of base registers (k-contiguous forms: 229-240 -> 205-226 VGPRs).
constexpr int SMEM = 2 * BUF;    // 128 KiB
constexpr int SMEM_R6 = 10 * IMG;  // 160 KiB (the whole LDS of a CU): the resident-plane walk's 3 A slots + 2 B slots

__device__ __forceinline__ uint32_t lds_off(const void *p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}
// 64 lanes x 16 B through a buffer descriptor into LDS at m0 + lane*16; lanes whose
// offset is outside the descriptor's range deliver zeros.  Inline asm: invisible to
// hipcc's wait-count pass, the kernel counts these loads itself.
__device__ __forceinline__ void dma(i32x4 srd, uint32_t voff, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :: "s"(lds_base), "v"(voff), "s"(srd) : "memory", "m0");
}
// the same with the wave-uniform part of the source offset in an SGPR (the instruction's soffset field): the per-lane
// offset register is then loop-invariant -- no v_add per piece, and nothing for the compiler to hoist into extra VGPRs
// when a loop is unrolled over many (plane, half, K-tile) combinations
__device__ __forceinline__ void dma_s(i32x4 srd, uint32_t voff, uint32_t soff, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(lds_base), "v"(voff), "s"(srd), "s"(soff) : "memory", "m0");
}
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
// CDML_F16X2 (gemm_f16x2_256.hip compiles THIS file with it): the 16-bit operands are fp16 -- v_mfma_f32_16x16x32_f16 -- and
// the plane-output epilogues write TWO fp16 planes hi | lo of (value * BArgs::c_scale) instead of three bf16 planes.  The
// tile, images, DMA schedule, fragment layouts and phases are those of the bf16 form (both types are 16 bits wide; a
// fragment is eight of them in four registers either way).  Only the split-fp32 (X3) launchers are exported from that build.
#ifdef CDML_F16X2
constexpr bool kF16 = true;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half2v = __attribute__((ext_vector_type(2))) _Float16;
#define CDML_MFMA16(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0)
// two fp32 -> one dword of two fp16 (round to nearest even; element 0 in the low half), and the halves back as fp32
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  uint32_t w = __builtin_bit_cast(uint32_t, half2v{(_Float16)a, (_Float16)b});
  asm("" : "+v"(w));
  return w;
}
__device__ __forceinline__ float lo_of(uint32_t w) { return (float)__builtin_bit_cast(half2v, w)[0]; }
__device__ __forceinline__ float hi_of(uint32_t w) { return (float)__builtin_bit_cast(half2v, w)[1]; }
#else
constexpr bool kF16 = false;
#define CDML_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
// two fp32 -> one dword of two bf16 (round to nearest even; element 0 in the low half), and the halves back as fp32
// (the dword is made opaque: hipcc otherwise sees through `pack << 16` and converts the low element a second time on its own)
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  uint32_t w = __builtin_bit_cast(uint32_t, bf16x2{(__bf16)a, (__bf16)b});
  asm("" : "+v"(w));
  return w;
}
__device__ __forceinline__ float lo_of(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float hi_of(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
#endif
constexpr int kPlanesOut = kF16 ? 2 : 3;             // planes a plane-output epilogue writes
__device__ __forceinline__ i32x4 make_srd(const void *base, int64_t bytes) {
  const uint64_t a = (uint64_t)(uintptr_t)base;
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  r.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)((a >> 32) & 0xffff));  // stride 0
  r.z = __builtin_amdgcn_readfirstlane((int)(bytes > 0 ? bytes : 0));
  r.w = 0x00020000;
  return r;
}

// Every half image is waited for one phase before the phase that reads it, which
// always leaves the five newest images (10 wave-instructions) in flight.
// f(integral_constant<int, 0>{}) ... f(integral_constant<int, N - 1>{}): the phases of a period, each with its number at compile time
template <class F, int... I>
__device__ __forceinline__ void unroll_seq(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void unroll(F &&f) {
  unroll_seq(f, std::make_integer_sequence<int, N>{});
}

#define CDML_BARRIER()                         \
  do {                                         \
    __builtin_amdgcn_sched_barrier(0);         \
    asm volatile("s_barrier" ::: "memory");    \
    __builtin_amdgcn_sched_barrier(0);         \
  } while (0)

// One variant of the tile kernel: its switches (described at run_tile, gemm_bf16_256.hip), what follows from them, and which combinations
// exist.  run_tile, block_of_launch and k_gemm_bf16_256 take this one type; launch sites use the names below it.
template <bool TN_, int EPI_, bool S16_, bool X3_ = false, bool F6_ = false, bool NTCS_ = false, bool R6_ = false,
          bool NARROW_ = false, bool KI_ = false, bool WIDEB_ = false>
struct Variant {
  static constexpr bool TN = TN_, S16 = S16_, X3 = X3_, F6 = F6_, NTCS = NTCS_, R6 = R6_, NARROW = NARROW_, KI = KI_, WIDEB = WIDEB_;
  static constexpr int EPI = EPI_;
  static constexpr bool KIA = KI, KIB = KI || WIDEB;           // which operand is stored k8-interleaved
  static constexpr bool kR6 = X3 && S16 && R6;                 // the resident-plane walk
  static constexpr bool kFast6 = X3 && S16 && F6;              // the unrolled six-step period
  static constexpr bool kSwap = EPI == BE_MINE_X3 || EPI == BE_KNN_X3 || EPI == BE_RANK_X3;   // mfma(b, a): a row's columns per lane
  static constexpr bool kRowBias = EPI == BE_ROWBIAS_LRELU_X3;
  static constexpr bool kBiasEpi = EPI == BE_BIAS_LRELU_BF16 || EPI == BE_BIAS_LRELU_X3 || kRowBias;
  static constexpr bool kMaskEpi = EPI == BE_MASK_BF16 || EPI == BE_MASK_X3;
  static constexpr bool kPlanes = EPI == BE_BIAS_LRELU_X3 || EPI == BE_MASK_X3 || kRowBias;   // writes planes of its output
  static constexpr int kSmem = R6 ? SMEM_R6 : SMEM;            // dynamic LDS of a launch
  static_assert(!TN || EPI == BE_F32, "the k-strided form only serves the weight gradients");
  static_assert(!NARROW || (X3 && S16 && R6 && !TN && (EPI == BE_BIAS_LRELU_X3 || EPI == BE_MASK_X3 || EPI == BE_ROWBIAS_LRELU_X3 || EPI == BE_F32)),
                "the 128 x 256 half tile exists for the plane-output products of the resident-plane walk and for the fp32 slabs of the narrow layer");
  static_assert(X3 || (EPI != BE_BIAS_LRELU_X3 && EPI != BE_MASK_X3 && EPI != BE_ROWBIAS_LRELU_X3),
                "plane outputs belong to the split-fp32 form");
  static_assert((EPI != BE_MINE_X3 && EPI != BE_KNN_X3 && EPI != BE_RANK_X3) || (X3 && S16 && R6 && !TN && !NARROW),
                "the mining / kNN-filter / rank-count epilogues ride on the resident-plane walk");
  static_assert(!KI || (TN && X3 && S16 && R6), "the k8-interleaved operands exist for the k-strided resident-plane walk");
  static_assert(!WIDEB || (TN && X3 && S16 && R6 && !KI && !kF16 && !NARROW && EPI == BE_F32),
                "the wide column operand exists for the bf16 k-strided resident-plane walk");
  static_assert(!(kF16 && kR6) || (!NARROW && !KI), "the fp16 form has the full tile on row-major operands only");
};
template <bool TN, int EPI, bool S16> using PlainLoop = Variant<TN, EPI, S16>;                         // one plane per operand
template <bool TN, int EPI> using X3General = Variant<TN, EPI, true, true>;                            // plane products, general loop
template <int EPI> using X3GeneralColsum = Variant<false, EPI, true, true, false, true>;               // ... with B's column sums (NTCS)
template <int EPI> using X3SixStep = Variant<false, EPI, true, true, true>;                            // the unrolled six-step walk (F6)
template <bool TN, int EPI> using X3Resident = Variant<TN, EPI, true, true, false, false, true>;       // the resident-plane walk (R6), full tile
template <int EPI> using X3ResidentHalf = Variant<false, EPI, true, true, false, false, true, true>;   // ... 128 x 256 half tile (NARROW)
using X3ResidentK8 = Variant<true, BE_F32, true, true, false, false, true, false, true>;               // dW on k8-interleaved operands (KI)
using X3ResidentWideB = Variant<true, BE_F32, true, true, false, false, true, false, false, true>;     // dW with dz1 as the wide operand (WIDEB)
using X3Mine = X3Resident<false, BE_MINE_X3>;                                                          // epilogues that store no tile:
using X3Knn = X3Resident<false, BE_KNN_X3>;                                                            // semi-hard miner, kNN filter,
using X3Rank = X3Resident<false, BE_RANK_X3>;                                                          // rank count

}  // namespace
}  // namespace cdml

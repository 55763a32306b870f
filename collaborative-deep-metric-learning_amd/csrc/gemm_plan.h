// How a GEMM entry cuts K into slabs: the ONE place where the partition is decided, shared by the workspace queries
// and the launches (gemm_bf16x3.hip, gemm_bf16.hip).  The partition sets the last bits of every gradient; it is what
// makes "a batch whole or in row blocks gives the same bits" true and cdml_gemm_bf16x3_tn / _tnk / _tn_kb bit-identical.
// Host arithmetic only -- no HIP, no environment: this header compiles with a plain C++17 compiler
// (tests/host/gemm_plan_table.cpp prints the table tests/data/gemm_plan_table.txt pins).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cdml {

constexpr int kPlanNumCU = 256;          // == kNumCU (common.h asserts it)

// split-K for the skinny weight gradients: fill one round of 256 CUs as evenly as
// possible with the fewest slabs (256 x 256 tiles)
inline int gemm_bf16_256_splits(int M, int N, int K) {
  const int64_t tiles = (int64_t)((M + 255) / 256) * (N / 256);
  const int max_by_k = K / 1024 > 0 ? K / 1024 : 1;
  int best = 1;
  double best_eff = 0.0;
  for (int s = 1; s <= 16 && s <= max_by_k; ++s) {
    const int64_t blocks = tiles * s;
    const double eff = (double)blocks / (double)(((blocks + kPlanNumCU - 1) / kPlanNumCU) * kPlanNumCU);
    if (eff > best_eff + 0.02) { best_eff = eff; best = s; }
  }
  return best;
}

// split-K for the k-contiguous forms whose output is ONE tile column wide (N = 256: the narrow forward layer, whose
// M / 256 tiles alone would leave most of the chip idle; fp32 slab output only).  The K partition is a function of K
// ALONE -- slabs of twenty six-step periods (120 K-tile steps), at most 16 of them, summed in slab order by k_x3_sum_slabs
// -- so the result does not depend on how many rows the call carries: a batch computed whole and the same batch computed
// in row blocks (two ranks against one) give the same bits.  (Round 3 chose the slab count from the tile count: 8
// slabs at 8 192 rows, none at 49 152, and leaky-relu' flips near zero then loosened the two-rank gradient bound.)
// Round 5: 120 steps instead of 60 -- four slabs at K = 5 120 -- which halves the slab round trip (the forward layer at
// 16 384 rows: 64 tiles x 4 slabs = one round of the chip instead of two rounds of half-length blocks); where four slabs
// leave the chip under-filled (8 192 rows: 128 blocks) the SAME slabs run as 128 x 256 half tiles (gemm_bf16_256.hip),
// so the partition stays a function of K alone.
// Wider outputs are never split: their tiles fill the chip at every batch size the step uses.
// Round 6: the slab length is a function of K and of the ROW-TILE CLASS.  The 120-step slabs were chosen for BASELINE's
// batches; the reference's own recipe (B = 1 024: 3 072 rows = 12 row tiles) fills 96 half-tile blocks with them and ran
// 0.622 against 0.643 ms/step with 60-step slabs (profiles/r05_reference_recipe_slab_steps_ab.txt).  Rule: where the
// 120-step slabs give at most 64 full tiles (128 half-tile blocks: half the chip) the slabs are 60 steps long -- twice the
// blocks -- else 120.  Within a class the partition is still a function of K alone (a batch whole or in row blocks of the
// same class: the same bits); ACROSS the class boundary the last bits of z differ.  A caller that needs one partition for
// every call size pins it: cdml_x3_slab_steps(120) (thread-local; catalogue inference does, so an embedding has the same
// bits in 4 096- and 49 152-row chunks: test_embedding_bits_do_not_depend_on_the_chunk).
// `slab_steps`: the pinned slab length (>= 12, whole six-step periods), 0 = by class.
// (half_steps: the two-plane fp16 form walks THREE steps per K-tile where the bf16 form walks six -- its slabs are half as
// many steps long, so that the partition of K itself is the same: 20 or 10 K-tiles of every plane per slab)
inline int x3_nt_splits(int N, int ktiles, int tiles_m, int slab_steps, bool half_steps = false) {
  if (N / 256 != 1) return 1;
  if (half_steps) ktiles *= 2;
  int steps = slab_steps;
  if (steps < 12) {
    int s120 = ktiles / 120;
    s120 = s120 < 1 ? 1 : (s120 > 16 ? 16 : s120);
    steps = tiles_m * s120 <= 64 ? 60 : 120;
  }
  const int s = ktiles / steps;
  return s < 1 ? 1 : (s > 16 ? 16 : s);
}

// K-tile steps per split, rounded up to whole walk periods (`period` = 6 for the six-product K-major walk, else 2), and
// the number of splits that then actually carry K-tiles: rounding `per` up can leave the last of the requested splits
// empty (ktiles = 288 in 11 splits: per = 30, ten splits cover it) -- an empty split would still launch its blocks, write
// a zero slab and be read back by the combine pass
inline void x3_split_geometry(int ktiles, int requested, int period, int &per, int &splits) {
  per = (ktiles + requested - 1) / requested;
  per = (per + period - 1) / period * period;
  splits = (ktiles + per - 1) / per;
}

// The plan of one launch.  K-tile steps (64 k of one plane product each): `ktiles` in all, `per` a split (whole walk
// periods), `splits` slabs.  Workspace layout: [slab_bytes of fp32 slabs, M x N each, when `slabs`][cs_bytes of column-sum
// partials, cs_rows rows of N]; `need` = what this launch asks of the workspace (the partials only when it sums columns).
struct KSplitPlan {
  int ktiles, period, per, splits;
  bool slabs;
  size_t slab_bytes, cs_rows, cs_bytes, need;
};

// the byte counts of a plan whose ktiles / period / per / splits are set; unsplit_slab: the result goes through one slab even
// when K is not split
inline void ksplit_bytes(KSplitPlan &p, int M, int N, bool unsplit_slab, bool colsum) {
  p.slabs = p.splits > 1 || unsplit_slab;
  p.slab_bytes = p.slabs ? (size_t)p.splits * M * N * sizeof(float) : 0;
  p.cs_rows = (size_t)p.splits * ((M + 255) / 256) * 2;      // per (split, row tile, row group of the tile's waves)
  p.cs_bytes = p.cs_rows * N * sizeof(float);
  p.need = p.slab_bytes + (colsum ? p.cs_bytes : 0);
}

// `requested` splits of `ktiles` steps in whole periods
inline KSplitPlan ksplit_plan(int M, int N, int ktiles, int requested, int period, bool unsplit_slab, bool colsum) {
  KSplitPlan p{};
  p.ktiles = ktiles; p.period = period;
  x3_split_geometry(ktiles, requested, period, p.per, p.splits);
  ksplit_bytes(p, M, N, unsplit_slab, colsum);
  return p;
}

// the k-strided forms' walk period: whole six-step periods of the six-product K-major walk per block (the unrolled loops need
// them) and whole three-step periods, an even count, of the fp16 form; three products or the product-major walk: an even count
inline int x3_tn_period(int products, bool kmajor, bool f16) { return ((products == 6 && kmajor) || f16) ? 6 : 2; }

// k-strided ("tn") plane products -- cdml_gemm_bf16x3_tn / _tnk / _tn_kb, cdml_gemm_f16x2_tn: C[M][N] = sum_k A[k][M] B[k][N].
// period: x3_tn_period of the walk (the interleaved forms: six products, K-major);
// bias: bias + leaky-relu are applied by the combine pass, which then reads a slab even when K is not split.
inline KSplitPlan x3_plan_tn(int M, int N, int K, int products, int period, bool bias, bool colsum) {
  const int ktiles = products * (K / 64);
  return ksplit_plan(M, N, ktiles, gemm_bf16_256_splits(M, N, ktiles * 64), period, bias, colsum);
}

// k-contiguous ("nt") plane products -- cdml_gemm_bf16x3_nt, cdml_gemm_f16x2_nt (f16: three steps per K-tile).  A plane
// output is never split.  The slab form needs the workspace: have_workspace = false is the caller's explicit choice of ONE
// pass over K (fewer, longer blocks; no slab round trip) -- its sums are associated differently, so the result's last bits
// differ from the slab form's and the "same bits whole or in row blocks" property holds only among calls that all pass a
// workspace.  A workspace that is given but smaller than `need` is the caller's error, not a change of arithmetic.
inline KSplitPlan x3_plan_nt(int M, int N, int K, int products, bool f16, bool planes_out, bool colsum, int slab_steps,
                             int period, bool have_workspace) {
  const int ktiles = products * (K / 64);
  int requested = planes_out ? 1 : x3_nt_splits(N, ktiles, (M + 255) / 256, slab_steps, f16);
  if (requested > 1) {
    const KSplitPlan p = ksplit_plan(M, N, ktiles, requested, period, false, colsum);
    if (p.splits > 1 && have_workspace) return p;
  }
  KSplitPlan p = ksplit_plan(M, N, ktiles, 1, 1, false, colsum);     // one pass: per = ktiles whatever the period
  p.period = period;
  return p;
}

// What cdml_gemm_bf16x3_workspace answers: the largest `need` over everything a launch of this shape can pick -- slab
// lengths 60 / 120 (a workspace serves any pin of cdml_x3_slab_steps; `slab_steps`: the pin in force, if it is another),
// the K-major and the product-major (A/B) walk's periods, with column sums -- and never less than one slab (the k-strided
// form's bias pass reads one even unsplit), plus one row of slack the query has always carried.  0: arguments no entry takes.
inline size_t x3_workspace_bytes(int tn, int M, int N, int K, int products, int slab_steps = 0) {
  if (M <= 0 || N <= 0 || K <= 0 || (products != 3 && products != 6) || K % 64) return 0;
  size_t need = 0;
  auto take = [&](const KSplitPlan &p) { if (p.need > need) need = p.need; };
  const int periods[2] = {6, 2}, lengths[3] = {60, 120, slab_steps};
  for (int period : periods) {
    take(ksplit_plan(M, N, products * (K / 64), 1, period, true, true));
    if (tn) take(x3_plan_tn(M, N, K, products, period, true, true));
    else for (int steps : lengths) take(x3_plan_nt(M, N, K, products, false, false, true, steps, period, true));
  }
  return need + (size_t)N * sizeof(float);
}

// Plain-bf16 k-strided product (cdml_gemm_bf16_tn and its workspace query): `splits` slabs of `per` K-tile steps, rounded
// to 128 k (period 2), every requested split launched; cs_rows = the column-sum chunks (splits * tiles_m * 2)
inline KSplitPlan bf16_tn_plan(int M, int N, int K, bool colsum) {
  KSplitPlan p{};
  p.ktiles = K / 64; p.period = 2;
  p.splits = gemm_bf16_256_splits(M, N, K);
  p.per = p.splits > 1 ? ((K + p.splits - 1) / p.splits + 127) / 128 * 2 : p.ktiles;
  ksplit_bytes(p, M, N, false, colsum);
  return p;
}

}  // namespace cdml

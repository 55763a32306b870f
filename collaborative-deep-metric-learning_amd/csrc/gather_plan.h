// The sampler + gather launches' argument checks and launch geometry: the ONE place where they are decided, for the eight
// fused entry points (cdml_sample_gather*, sampler_gather.hip) and the three unfused ones (cdml_gather_rows, _x3, _f16),
// and for their fp8-table twins (include/cdml_f8.h).
// A row format says what the kernels of that format are built for; plan_sample_gather / plan_gather_rows check a call
// against it -- every check returns before any HIP call -- and fill the GatherPlan the launcher selects the kernel
// instantiation from (with_nch: the NCH buckets of the format ARE the instantiations that exist).
// Host arithmetic only -- no HIP: this header compiles with a plain C++17 compiler
// (tests/host/gather_plan_table.cpp prints the table tests/data/gather_plan_table.txt pins).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "gemm_plan.h"
#include "require.h"

#ifndef CDML_GATHER_ROWS_PER_WAVE
#define CDML_GATHER_ROWS_PER_WAVE 2   // rows a wave keeps in flight (A/B'd: tools/gather_variants.sh)
#endif
#ifndef CDML_GATHER_ROWS_PER_WAVE_F16
#define CDML_GATHER_ROWS_PER_WAVE_F16 4   // 3-KB rows: four in flight per wave
#endif
#ifndef CDML_GATHER_ROWS_PER_WAVE_F8
#define CDML_GATHER_ROWS_PER_WAVE_F8 4    // 1.5-KB rows of e4m3 codes (include/cdml_f8.h): the fp16 rows' value
#endif

namespace cdml {

constexpr int kGatherWave = 64, kGatherWavesPerBlock = 4;     // == kWave, kThreads / kWave of the kernels (asserted there)

// NCH = 16-B chunks per lane a kernel instantiation holds in registers (one wave per row: covers 64 * NCH chunks)
struct NchBuckets { int n; int v[4]; };

// how a format's entry points word their F and layout errors (the texts are part of the ABI's behaviour)
enum class LayoutWording {
  kRows32,   // F with its value; "strides must be >= F and multiples of 4", then "bases must be 16-B aligned"
  kPlanes,   // F with its value; "out_stride must be <planes> planes of >= F columns (multiples of 4)"
  kRows16,   // F without its value; "strides must be >= F and multiples of 8, bases 16-B aligned"
  kRows8,    // fp8 table: F with its value; the table's stride a multiple of 16 bytes, the bf16 rows' of 8 elements
};

struct GatherFormat {
  const char *who_listed;    // the name the listed entry point's own checks report under; null = the format has no mode 2
  int planes;                // planes per output row, out_stride / planes columns each
  int per_chunk;             // elements per lane and chunk of a table row: 4 (fp32, 16 B), 8 (fp16, 16 B; fp8, 8 B); strides are multiples of it
  int max_f;
  int rows_per_chunk;        // rows a block takes per walk step of the fused kernel: ROW::kRows * waves per block
  NchBuckets fused, rows;    // the instantiations of k_sample_gather / of the format's unfused kernel
  bool ki;                   // the k8-interleaved copy (x_ki) exists
  LayoutWording wording;
};

constexpr int kRowsF32 = CDML_GATHER_ROWS_PER_WAVE * kGatherWavesPerBlock, kRowsF16 = CDML_GATHER_ROWS_PER_WAVE_F16 * kGatherWavesPerBlock;
constexpr int kRowsF8 = CDML_GATHER_ROWS_PER_WAVE_F8 * kGatherWavesPerBlock;
// fp32 rows | three bf16 planes | two fp16 planes (no listed form, no unfused kernel) | fp16 table -> bf16 rows
inline constexpr GatherFormat kGatherF32 = {"sample_gather_listed", 1, 4, 2048, kRowsF32, {3, {2, 6, 8}}, {4, {2, 4, 6, 8}}, false, LayoutWording::kRows32};
inline constexpr GatherFormat kGatherX3 = {"sample_gather_listed_x3", 3, 4, 2048, kRowsF32, {2, {6, 8}}, {4, {2, 4, 6, 8}}, true, LayoutWording::kPlanes};
inline constexpr GatherFormat kGatherH2 = {nullptr, 2, 4, 2048, kRowsF32, {2, {6, 8}}, {0, {}}, false, LayoutWording::kPlanes};
inline constexpr GatherFormat kGatherF16 = {"sample_gather_listed_f16", 1, 8, 4096, kRowsF16, {3, {1, 3, 8}}, {3, {1, 3, 8}}, false, LayoutWording::kRows16};
// fp8 (e4m3) table -> bf16 rows (include/cdml_f8.h): the fp16 format's lane -> column mapping and buckets, 8-B chunks
inline constexpr GatherFormat kGatherF8 = {"sample_gather_listed_f8", 1, 8, 4096, kRowsF8, {3, {1, 3, 8}}, {3, {1, 3, 8}}, false, LayoutWording::kRows8};

// the listed draw's own arguments (cdml_hardneg.h); kind_out null = not wanted
struct ListedArgs {
  const int32_t *lists;
  int64_t ldl;
  int L;
  uint64_t hard_thresh;
  int32_t *kind_out;
  int64_t kind_step_stride;
};

// the weighted draw's own arguments (cdml_negweights.h); `who`: the name the entry point's own checks report under
struct WeightedArgs {
  const char *who;
  const int32_t *start, *coarse;             // start: uint32 bits [n_live]; coarse [2^bits + 1]
  int64_t n_live;
  int bits;
  int32_t *kind_out;
  int64_t kind_step_stride;
};

// One fused launch, in the order of the C entry points' parameters.
struct SampleGatherArgs {
  int mode;                                  // 0 uniform, 1 in-batch, 2 listed (with `listed`), 3 weighted (with `weighted`)
  const int32_t *pairs; int64_t n_pairs;     // the pair stream
  uint64_t seed, step; const uint64_t *step_dev;
  int batch; int64_t slot0, batch_global;
  const void *table; int64_t n_rows, row_stride; int F;
  int32_t *idx_out, *shift_out;
  void *x_out; int64_t out_stride;
  int n_steps; int64_t x_step_stride, idx_step_stride;
  int32_t *oob_flag;
  void *x_ki; int64_t ki_step_stride;        // optional (formats with ki)
  bool ki_entry;                             // cdml_sample_gather_x3k: x_ki is not optional
  const ListedArgs *listed;                  // optional (formats with who_listed)
  const WeightedArgs *weighted = nullptr;    // optional (the same formats)
};

struct GatherRowsArgs {
  const void *table; int64_t row0, n_rows, row_stride;
  const int32_t *idx; int n_idx; int F;
  void *x_out; int64_t out_stride;
};

struct GatherPlan { int rpt, grid, nch, plane; bool ki; };    // rows per triplet, blocks, NCH bucket, columns per plane

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// at most 8 resident blocks per CU
// (round 5: a grid with every block walking the same number of chunks -- 1 536 blocks x 3 chunks instead of 2 048 blocks x
// 2.25 -- was measured SLOWER for the fp16 gather, 0.600 against 0.675 of 8 TB/s: what counts is 8 resident blocks per CU,
// not an even chunk count)
inline int grid_for(int64_t work_items, int per_block) {
  int64_t b = (work_items + per_block - 1) / per_block;
  const int64_t cap = (int64_t)kPlanNumCU * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// the smallest bucket whose registers hold a row of F elements (F <= max_f: the last one does)
inline int nch_bucket(const GatherFormat &f, const NchBuckets &b, int F) {
  const int need = ((F + f.per_chunk - 1) / f.per_chunk + kGatherWave - 1) / kGatherWave;
  for (int i = 0; i < b.n - 1; ++i)
    if (need <= b.v[i]) return b.v[i];
  return b.v[b.n - 1];
}

inline int check_listed(const char *who, const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh) {
  CDML_REQUIRE(lists, CDML_E_BADARG, "%s: lists is null", who);
  CDML_REQUIRE(L >= 1 && L <= 1024, CDML_E_BADARG, "%s: L = %d outside [1, 1024]", who, L);
  CDML_REQUIRE(ldl >= L, CDML_E_BADARG, "%s: ldl < L", who);
  CDML_REQUIRE(hard_thresh <= (1ull << 32), CDML_E_BADARG, "%s: hard_thresh > 2^32", who);
  return CDML_OK;
}

inline int check_weighted(const char *who, const int32_t *start, const int32_t *coarse, int64_t n_live, int64_t n_rows, int bits) {
  CDML_REQUIRE(start && coarse, CDML_E_BADARG, "%s: the start / coarse tables are null", who);
  CDML_REQUIRE(n_live >= 3 && n_live <= n_rows, CDML_E_BADARG, "%s: n_live = %lld outside [3, n_rows = %lld]", who,
               (long long)n_live, (long long)n_rows);
  CDML_REQUIRE(bits >= 8 && bits <= 24, CDML_E_BADARG, "%s: bits = %d outside [8, 24]", who, bits);
  return CDML_OK;
}

// F, strides and bases of a table -> rows copy.  Every format words its rule its own way (and the fp32 one in two steps).
inline int check_gather_layout(const char *who, const GatherFormat &f, bool fused, const void *table, int64_t row_stride, int F,
                               const void *x_out, int64_t out_stride) {
  const bool f_ok = F > 0 && F <= f.max_f;
  if (f.wording == LayoutWording::kRows16) CDML_REQUIRE(f_ok, CDML_E_UNSUPPORTED, "%s: feature size outside (0, %d]", who, f.max_f);
  else if (f.wording == LayoutWording::kRows8) CDML_REQUIRE(f_ok, CDML_E_UNSUPPORTED, "%s: F = %d outside (0, %d] of the fp8 gather", who, F, f.max_f);
  else CDML_REQUIRE(f_ok, CDML_E_UNSUPPORTED, "%s: feature size %d outside (0, %d]", who, F, f.max_f);
  const int64_t m = f.per_chunk - 1, plane = out_stride / f.planes;
  const int64_t mt = f.wording == LayoutWording::kRows8 ? 15 : m;       // (the fp8 table's rows: whole 16-B units)
  const bool strides = row_stride >= F && (row_stride & mt) == 0 && out_stride % f.planes == 0 && plane >= F && (plane & m) == 0;
  const bool bases = aligned_to(table, 16) && aligned_to(x_out, f.planes > 1 ? 8 : 16);
  if (f.wording == LayoutWording::kPlanes) {
    CDML_REQUIRE(strides && bases, CDML_E_ALIGN, "%s: out_stride must be %d planes of >= F columns (multiples of 4)%s", who, f.planes,
                 fused ? "" : ", 16-B aligned rows");
  } else if (f.wording == LayoutWording::kRows16) {
    CDML_REQUIRE(strides && bases, CDML_E_ALIGN, "%s: strides must be >= F and multiples of 8, bases 16-B aligned", who);
  } else if (f.wording == LayoutWording::kRows8) {
    CDML_REQUIRE(strides && bases, CDML_E_ALIGN,
                 "%s: row_stride must be >= F and a multiple of 16, out_stride >= F and a multiple of 8, bases 16-B aligned", who);
  } else {
    CDML_REQUIRE(strides, CDML_E_ALIGN, "%s: strides must be >= F and multiples of 4", who);
    CDML_REQUIRE(bases, CDML_E_ALIGN, "%s: bases must be 16-B aligned", who);
  }
  return CDML_OK;
}

// Every check of a fused launch, in ONE order for all formats: the entry's own arguments (x_ki of _x3k, the listed block
// and the weighted block, under the entry's name), mode, n_steps, per-step strides, pointers, n_rows, batch, shift_out,
// batch_global, F, layout, the interleave rule (under _x3k's name, whichever entry passed x_ki).  `who`: the name the
// format's checks report under.
inline int plan_sample_gather(const char *who, const GatherFormat &f, const SampleGatherArgs &a, GatherPlan &p) {
  CDML_REQUIRE(!a.ki_entry || a.x_ki, CDML_E_BADARG, "sample_gather_x3k: x_ki required (cdml_sample_gather_x3 without it)");
  const bool listed = a.listed && f.who_listed;
  if (listed) {
    const ListedArgs &l = *a.listed;
    const int rc = check_listed(f.who_listed, l.lists, l.ldl, l.L, l.hard_thresh);
    if (rc) return rc;
    CDML_REQUIRE(!l.kind_out || a.n_steps <= 1 || l.kind_step_stride >= a.batch, CDML_E_BADARG, "%s: kind_step_stride < batch",
                 f.who_listed);
  }
  const bool weighted = a.weighted && f.who_listed;
  if (weighted) {
    const WeightedArgs &w = *a.weighted;
    const int rc = check_weighted(w.who, w.start, w.coarse, w.n_live, a.n_rows, w.bits);
    if (rc) return rc;
    CDML_REQUIRE(!w.kind_out || a.n_steps <= 1 || w.kind_step_stride >= a.batch, CDML_E_BADARG, "%s: kind_step_stride < batch", w.who);
  }
  CDML_REQUIRE(a.mode == 0 || a.mode == 1 || (a.mode == 2 && listed) || (a.mode == 3 && weighted), CDML_E_BADARG,
               "%s: mode must be 0 or 1", who);
  CDML_REQUIRE(a.n_steps >= 1 && a.n_steps <= 64, CDML_E_BADARG, "%s: n_steps must be in [1, 64]", who);
  p.rpt = a.mode == 1 ? 2 : 3;
  const int64_t rows_per_step = (int64_t)a.batch * p.rpt;
  CDML_REQUIRE(a.n_steps == 1 || (a.x_step_stride >= rows_per_step * a.out_stride && (a.x_step_stride & (f.per_chunk - 1)) == 0 &&
                                  a.idx_step_stride >= rows_per_step),
               CDML_E_BADARG, "%s: per-step strides too small for the batch", who);
  CDML_REQUIRE(a.pairs && a.table && a.idx_out && a.x_out && a.n_pairs > 0 && a.slot0 >= 0, CDML_E_BADARG, "%s: bad argument", who);
  CDML_REQUIRE(a.n_rows >= 3 && a.n_rows <= 0x7FFFFFFFll, CDML_E_BADARG, "%s: n_rows must be in [3, 2^31)", who);
  CDML_REQUIRE(a.batch >= (a.mode == 1 ? 2 : 1), CDML_E_BADARG, "%s: batch too small", who);
  CDML_REQUIRE(a.mode != 1 || a.shift_out, CDML_E_BADARG, "%s: shift_out required in mode 1", who);
  CDML_REQUIRE(a.batch_global >= a.slot0 + a.batch, CDML_E_BADARG, "%s: batch_global < slot0 + batch", who);
  const int rc = check_gather_layout(who, f, true, a.table, a.row_stride, a.F, a.x_out, a.out_stride);
  if (rc) return rc;
  p.grid = grid_for(rows_per_step * a.n_steps, f.rows_per_chunk);
  p.nch = nch_bucket(f, f.fused, a.F);
  p.plane = (int)(a.out_stride / f.planes);
  p.ki = f.ki && a.x_ki;
  if (p.ki) {
    // the interleaved copy: [3][rows_per_step / 8][plane][8] per step; whole row groups per step (a chunk of the kernel = one
    // group of 8 rows), plane in 256-column slices that the row registers cover (NCH x 256 columns)
    CDML_REQUIRE(rows_per_step % 8 == 0 && p.plane % 256 == 0 && p.plane <= p.nch * 256 && aligned_to(a.x_ki, 16) &&
                     (a.n_steps == 1 || a.ki_step_stride >= 3 * rows_per_step * p.plane) && f.rows_per_chunk == 8,
                 CDML_E_UNSUPPORTED, "sample_gather_x3k: needs 8 | rows per step, plane columns a multiple of 256 (<= %d), 16-B aligned x_ki",
                 p.nch * 256);
  }
  return CDML_OK;
}

// cdml_gather_rows (fp32), _x3 (row0 = 0) and _f16: one wave per row, a block of four waves per grid step
inline int plan_gather_rows(const char *who, const GatherFormat &f, const GatherRowsArgs &a, GatherPlan &p) {
  CDML_REQUIRE(a.table && a.idx && a.x_out && a.n_rows > 0 && a.n_idx > 0 && a.row0 >= 0, CDML_E_BADARG, "%s: bad argument", who);
  const int rc = check_gather_layout(who, f, false, a.table, a.row_stride, a.F, a.x_out, a.out_stride);
  if (rc) return rc;
  p.rpt = 0;
  p.grid = grid_for(a.n_idx, kGatherWavesPerBlock);
  p.nch = nch_bucket(f, f.rows, a.F);
  p.plane = (int)(a.out_stride / f.planes);
  p.ki = false;
  return CDML_OK;
}

// Calls launch(std::integral_constant<int, NCH>) for the bucket `nch` of the format's fused (or unfused) kernels: the
// instantiations a launcher can reach are the format's buckets, no more and no fewer.  An `nch` that is no bucket of the
// format launches nothing and is an error here (a plan of this header never names one).
template <const GatherFormat &FMT, bool FUSED, typename L, size_t... I>
inline bool with_nch_impl(int nch, L &&launch, std::index_sequence<I...>) {
  constexpr NchBuckets b = FUSED ? FMT.fused : FMT.rows;
  return ((nch == b.v[I] ? (launch(std::integral_constant<int, b.v[I]>{}), true) : false) || ...);
}
template <const GatherFormat &FMT, bool FUSED, typename L>
inline int with_nch(const char *who, int nch, L &&launch) {
  const bool found = with_nch_impl<FMT, FUSED>(nch, launch, std::make_index_sequence<(size_t)(FUSED ? FMT.fused : FMT.rows).n>{});
  CDML_REQUIRE(found, CDML_E_UNSUPPORTED, "%s: no kernel holds %d chunks per lane", who, nch);
  return CDML_OK;
}

}  // namespace cdml

// The filter scan over product-quantised lists (include/cdml_ivf_range.h): the launch behind
// IVFIndex.range_search on storage "pq".  The 8-bit ADC scan of csrc/pq_common.h (pq_scan_body: the tile decode, the lane's
// code words in registers, the S lookup tables in LDS, the sums in ascending m with or without a base) with another last step:
// no score is written; a (slot, row) whose distance is within the query's tau is appended to the query's candidate list, as
// the filter scans of csrc/ivf_filter.hip append it.
//
//   k_ivf_filter_pq    pq_scan_body<M8, false, RangeAppend>
//   k_ivf_filter_pqr   pq_scan_body<M8, true, RangeAppend>: the sums start from slot_base[slot]
// The slot is block-uniform, so the query, its q_sq and its tau are scalar loads and cnt + q is the same address in every lane
// of a wave: the compiler folds the lanes' atomicAdd(cnt + q, 1) into one add of the active lanes' count per wave (section
// 9f.8 quotes the assembly).  A lane loads r_sq / ids of its two rows once per tile.
#include "pq_common.h"
#include "../../include/cdml_ivf_range.h"

namespace cdml {
namespace {

struct RangeArgs {
  const int32_t *slot_query;
  int n_queries;
  const float *q_sq, *tau;                // per query of the chunk
  int32_t *cnt;                           // per query of the chunk: candidates appended so far (dropped ones included)
  const float *r_sq;                      // per listed row
  const int32_t *ids;                     // per listed row
  uint2 *cand;                            // [n_queries][cap] (bits of d, id)
  int cap;
};

// pq_scan_body's last step (csrc/pq_common.h says when it calls what)
struct RangeAppend : RangeArgs {
  float rs[kRowsPerLane];                 // the lane's two rows: r_sq, id, inside the list
  int id[kRowsPerLane];
  bool row_in[kRowsPerLane];
  __device__ __forceinline__ explicit RangeAppend(const RangeArgs &a) : RangeArgs(a) {}

  __device__ __forceinline__ void begin(const ScanTile &tile, int t) {
#pragma unroll
    for (int u = 0; u < kRowsPerLane; ++u) {
      const int j = tile.j0 + t + kScanThreads * u;
      row_in[u] = j < tile.len;
      const int row = tile.r0 + min(j, tile.len - 1);        // clamped: a valid listed row (a valid tile has len >= 1)
      rs[u] = r_sq[row];
      id[u] = ids[row];
    }
  }

  __device__ __forceinline__ void slot(const ScanTile &tile, int s, int, const float (&acc)[kRowsPerLane]) const {
    const int q = slot_query[tile.s0 + tile.i0 + s];         // block-uniform: scalar loads, here and of q_sq / tau
    if ((unsigned)q >= (unsigned)n_queries) return;          // (the tables were staged from a clamped query: nothing is appended)
    const float qs = q_sq[q], ta = tau[q];
#pragma unroll
    for (int u = 0; u < kRowsPerLane; ++u) {
      const float dr = (qs + rs[u]) - 2.f * acc[u];
      const float d = dr < 0.f ? 0.f : dr;                   // the clamp keeps a NaN; NaN never passes
      if (d <= ta && row_in[u]) {
        const int pos = atomicAdd(cnt + q, 1);
        if ((unsigned)pos < (unsigned)cap) cand[(int64_t)q * cap + pos] = make_uint2(__float_as_uint(d), (uint32_t)id[u]);
      }
    }
  }
};

template <int M8>
__global__ void __launch_bounds__(kScanThreads)
k_ivf_filter_pq(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
                const int32_t *__restrict__ slot_start, const uint8_t *__restrict__ codes, int64_t ldc,
                const int32_t *__restrict__ list_start, const int4 *__restrict__ tiles, RangeArgs f) {
  pq_scan_body<M8, false>(lut, n_queries, slot_query, slot_start, nullptr, nullptr, codes, ldc, list_start, tiles, nullptr,
                          RangeAppend(f));
}

template <int M8>
__global__ void __launch_bounds__(kScanThreads)
k_ivf_filter_pqr(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
                 const int32_t *__restrict__ slot_start, const float *__restrict__ slot_base, const uint8_t *__restrict__ codes,
                 int64_t ldc, const int32_t *__restrict__ list_start, const int4 *__restrict__ tiles, RangeArgs f) {
  pq_scan_body<M8, true>(lut, n_queries, slot_query, slot_start, nullptr, slot_base, codes, ldc, list_start, tiles, nullptr,
                         RangeAppend(f));
}

// the checks of both launches: check_pq_scan_args for what the scans share (there is no score buffer to align), then the
// candidate list's
int check_range_args(const char *name, bool pointers, const float *lut, int n_queries, const uint8_t *codes, int64_t ldc, int M,
                     const int32_t *tiles, int n_tiles, const void *cand, int cap) {
  if (int rc = check_pq_scan_args(name, pointers, lut, n_queries, codes, ldc, M, tiles, n_tiles, nullptr)) return rc;
  CDML_REQUIRE(cap > 0 && !(cap & (cap - 1)), CDML_E_UNSUPPORTED, "%s: cap must be a positive power of two, got %d", name, cap);
  CDML_REQUIRE((reinterpret_cast<uintptr_t>(cand) & 7) == 0, CDML_E_ALIGN, "%s: cand must be 8-B aligned", name);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_ivf_filter_pq(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                                  const float *q_sq, const float *tau, int32_t *cnt, const uint8_t *codes, int64_t ldc,
                                  const int32_t *list_start, const float *r_sq, const int32_t *ids, int M, const int32_t *tiles,
                                  int n_tiles, void *cand, int cap, cdml_stream_t stream) {
  if (int rc = check_range_args("ivf_filter_pq",
                                lut && slot_query && slot_start && q_sq && tau && cnt && codes && list_start && r_sq && ids && tiles && cand,
                                lut, n_queries, codes, ldc, M, tiles, n_tiles, cand, cap))
    return rc;
  const RangeArgs f{slot_query, n_queries, q_sq, tau, cnt, r_sq, ids, reinterpret_cast<uint2 *>(cand), cap};
  const int4 *tl = reinterpret_cast<const int4 *>(tiles);
  hipStream_t st = (hipStream_t)stream;
  dispatch_m8(M, [&](auto m8) {
    hipLaunchKernelGGL(k_ivf_filter_pq<decltype(m8)::value>, dim3(n_tiles), dim3(kScanThreads), 0, st, lut, n_queries, slot_query,
                       slot_start, codes, ldc, list_start, tl, f);
  });
  return check_launch("ivf_filter_pq");
}

extern "C" int cdml_ivf_filter_pqr(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                                   const float *slot_base, const float *q_sq, const float *tau, int32_t *cnt, const uint8_t *codes,
                                   int64_t ldc, const int32_t *list_start, const float *r_sq, const int32_t *ids, int M,
                                   const int32_t *tiles, int n_tiles, void *cand, int cap, cdml_stream_t stream) {
  if (int rc = check_range_args(
          "ivf_filter_pqr",
          lut && slot_query && slot_start && slot_base && q_sq && tau && cnt && codes && list_start && r_sq && ids && tiles && cand, lut,
          n_queries, codes, ldc, M, tiles, n_tiles, cand, cap))
    return rc;
  const RangeArgs f{slot_query, n_queries, q_sq, tau, cnt, r_sq, ids, reinterpret_cast<uint2 *>(cand), cap};
  const int4 *tl = reinterpret_cast<const int4 *>(tiles);
  hipStream_t st = (hipStream_t)stream;
  dispatch_m8(M, [&](auto m8) {
    hipLaunchKernelGGL(k_ivf_filter_pqr<decltype(m8)::value>, dim3(n_tiles), dim3(kScanThreads), 0, st, lut, n_queries, slot_query,
                       slot_start, slot_base, codes, ldc, list_start, tl, f);
  });
  return check_launch("ivf_filter_pqr");
}

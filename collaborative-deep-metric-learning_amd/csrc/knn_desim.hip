// Near-duplicate suppression of the kNN export (reference: faiss_knn.py:146-244, `fliter_fI` + `iter_desim_mp`).
//
// The reference takes a second kNN over the RAW features (fD, fI: raw-feature distances and ids, k = desim_nearest_num)
// and then walks every embedding-neighbour list eI[i, :] left to right: a neighbour that is still kept removes, from the
// columns at or after its own, every neighbour that lies among ITS raw-feature near-duplicates (fI[j, :fI_end] with
// fD <= threshold, j itself and -1 excluded); at the end the query's own id is removed.  The reference runs this as a
// 22-process pool of per-row np.isin calls (one pool per column); here it is two launches:
//
//   k_desim_prep   the filtered raw-feature lists, once per catalogue: out[r][t] = fI[r][t] if t < fI_end, !(fD[r][t] > thr)
//                  (the float32 compare numpy makes: fD == float32(thr) is kept), fI[r][t] != r and fI[r][t] >= 0; else -1.
//                  Rows padded to kp = 32 | 64 int32 = one | two whole 128-B lines, so that a gather reads whole lines.
//   k_knn_desim    one wave per query row: the row's ke <= 128 ids in two registers per lane (columns lane, lane + 64), the
//                  filtered lists of ALL its initially valid neighbours gathered into LDS up front (ke x kp x 4 B: 10 KB at
//                  ke = 81, kp = 32; rows that the walk will drop are fetched too -- the loads are independent and in
//                  flight together, where a gather per kept column would be one dependent global load per column), then
//                  the serial greedy walk in LDS: column c's keep bit is a bit of the wave's ballot (wave-uniform), its
//                  list is read as broadcast int4 loads, and every lane tests its own two columns against it.
//
// Rows are independent, nothing is accumulated across waves: no atomics, the result is a function of the inputs only.
// Ids < 0 and ids >= n_f in eI are "not kept" (the reference has no such ids: -1 is faiss' "no neighbour", and an id past
// its fI would raise).
#include "common.h"

namespace cdml {
namespace {

constexpr int kDesimMaxCols = CDML_KNN_LIST;   // 128: two columns per lane

template <typename IdT>
__global__ void __launch_bounds__(256)
k_desim_prep(const IdT *__restrict__ fI, int64_t ldf, const float *__restrict__ fD, int64_t ldd, int n_f, int fI_end,
             float thr, int32_t *__restrict__ out, int kp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_f * kp) return;
  const int r = (int)(e / kp), t = (int)(e - (int64_t)r * kp);
  int32_t v = -1;
  if (t < fI_end) {
    const int64_t id = (int64_t)fI[(int64_t)r * ldf + t];
    const float d = fD[(int64_t)r * ldd + t];
    // !(d > thr): numpy's fD > fD_threshold drops, so a NaN distance is kept as the reference keeps it
    if (!(d > thr) && id >= 0 && id != r && id <= 0x7fffffff) v = (int32_t)id;
  }
  out[e] = v;
}

__global__ void __launch_bounds__(64)
k_knn_desim(const int32_t *__restrict__ eI, int64_t lde, int nq, int ke, const int32_t *__restrict__ query_id, int row0,
            const int32_t *__restrict__ ff, int kp, int n_f, int32_t *__restrict__ out, int64_t ldo) {
  extern __shared__ int4 s_rows[];                 // [ke][kp / 4] int4: the filtered lists of the row's neighbours
  __shared__ int32_t s_id[kDesimMaxCols];          // the row's ids, -1 where not kept from the start
  const int row = blockIdx.x, lane = threadIdx.x;  // one wave per block, one block per row
  const int32_t *er = eI + (int64_t)row * lde;
  const int c1 = lane + 64;
  int32_t e0 = lane < ke ? er[lane] : -1;
  int32_t e1 = c1 < ke ? er[c1] : -1;
  bool k0 = e0 >= 0 && e0 < n_f;
  bool k1 = e1 >= 0 && e1 < n_f;
  s_id[lane] = k0 ? e0 : -1;
  s_id[c1] = k1 ? e1 : -1;
  __syncthreads();
  // gather: ke rows of kp / 4 int4 each (whole 128-B lines), all loads independent
  const int cpr = kp >> 2, lg = kp == 32 ? 3 : 4;  // int4 chunks per row (8 | 16)
  const int total = ke * cpr;
#pragma unroll 4
  for (int x = lane; x < total; x += 64) {
    const int c = x >> lg, part = x & (cpr - 1);
    const int32_t j = s_id[c];
    int4 v = make_int4(-1, -1, -1, -1);
    if (j >= 0) v = reinterpret_cast<const int4 *>(ff + (int64_t)j * kp)[part];
    s_rows[x] = v;
  }
  __syncthreads();
  // the greedy walk: serial over c, wave-uniform (the keep bits of all columns are two ballots)
  unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
  for (int c = 0; c < ke; ++c) {
    const bool kc = c < 64 ? (m0 >> c) & 1ull : (m1 >> (c - 64)) & 1ull;
    if (!kc) continue;                             // uniform: m0 / m1 are the same in every lane
    bool h0 = false, h1 = false;
    const int4 *fr = s_rows + c * cpr;
    for (int q = 0; q < cpr; ++q) {
      const int4 f = fr[q];                        // the same address in every lane: an LDS broadcast
      h0 |= (e0 == f.x) | (e0 == f.y) | (e0 == f.z) | (e0 == f.w);
      h1 |= (e1 == f.x) | (e1 == f.y) | (e1 == f.z) | (e1 == f.w);
    }
    // only the columns after c (c itself is never in its own list: the prep removed j from row j)
    k0 = k0 && !(h0 && lane > c);
    k1 = k1 && !(h1 && c1 > c);
    m0 = __ballot(k0);
    m1 = __ballot(k1);
  }
  const int32_t self = query_id ? query_id[row] : row0 + row;   // the query itself (faiss_knn.py:238-240), after the walk
  int32_t *orow = out + (int64_t)row * ldo;
  if (lane < ke) orow[lane] = (k0 && e0 != self) ? e0 : -1;
  if (c1 < ke) orow[c1] = (k1 && e1 != self) ? e1 : -1;
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_knn_desim_prep(const void *fI, int fI_is_int64, int64_t ldf, const float *fD, int64_t ldd, int n_f,
                                   int fI_end, float threshold, int32_t *out, int kp, cdml_stream_t stream) {
  CDML_REQUIRE(fI && fD && out, CDML_E_BADARG, "knn_desim_prep: null pointer");
  CDML_REQUIRE(n_f > 0 && fI_end > 0 && (fI_is_int64 == 0 || fI_is_int64 == 1), CDML_E_BADARG,
               "knn_desim_prep: bad size or id type (n_f %d, fI_end %d, fI_is_int64 %d)", n_f, fI_end, fI_is_int64);
  CDML_REQUIRE(kp == 32 || kp == 64, CDML_E_UNSUPPORTED, "knn_desim_prep: kp must be 32 or 64, got %d", kp);
  CDML_REQUIRE(fI_end <= kp, CDML_E_UNSUPPORTED, "knn_desim_prep: fI_end %d exceeds kp %d", fI_end, kp);
  CDML_REQUIRE(ldf >= fI_end && ldd >= fI_end, CDML_E_BADARG, "knn_desim_prep: row strides must be >= fI_end");
  CDML_REQUIRE(aligned16(out), CDML_E_ALIGN, "knn_desim_prep: out must be 16-B aligned");
  const int64_t n = (int64_t)n_f * kp;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (fI_is_int64)
    hipLaunchKernelGGL(k_desim_prep<int64_t>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const int64_t *>(fI), ldf,
                       fD, ldd, n_f, fI_end, threshold, out, kp);
  else
    hipLaunchKernelGGL(k_desim_prep<int32_t>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const int32_t *>(fI), ldf,
                       fD, ldd, n_f, fI_end, threshold, out, kp);
  return check_launch("knn_desim_prep");
}

extern "C" int cdml_knn_desim(const int32_t *eI, int64_t lde, int nq, int ke, const int32_t *query_id, int row0,
                              const int32_t *f_filtered, int kp, int n_f, int32_t *out, int64_t ldo, cdml_stream_t stream) {
  CDML_REQUIRE(eI && f_filtered && out, CDML_E_BADARG, "knn_desim: null pointer");
  CDML_REQUIRE(nq > 0 && ke > 0 && n_f > 0 && row0 >= 0, CDML_E_BADARG, "knn_desim: bad size (nq %d, ke %d, n_f %d, row0 %d)",
               nq, ke, n_f, row0);
  CDML_REQUIRE(ke <= kDesimMaxCols, CDML_E_UNSUPPORTED, "knn_desim: ke must be <= %d, got %d", kDesimMaxCols, ke);
  CDML_REQUIRE(kp == 32 || kp == 64, CDML_E_UNSUPPORTED, "knn_desim: kp must be 32 or 64, got %d", kp);
  CDML_REQUIRE(lde >= ke && ldo >= ke, CDML_E_BADARG, "knn_desim: row strides must be >= ke");
  CDML_REQUIRE(query_id || (int64_t)row0 + nq <= 0x7fffffff, CDML_E_BADARG, "knn_desim: row0 + nq exceeds the int32 id range");
  CDML_REQUIRE(aligned16(f_filtered), CDML_E_ALIGN, "knn_desim: f_filtered must be 16-B aligned");
  const size_t lds = (size_t)ke * kp * sizeof(int32_t);      // <= 32 KB
  hipLaunchKernelGGL(k_knn_desim, dim3(nq), dim3(64), lds, (hipStream_t)stream, eI, lde, nq, ke, query_id, row0, f_filtered,
                     kp, n_f, out, ldo);
  return check_launch("knn_desim");
}

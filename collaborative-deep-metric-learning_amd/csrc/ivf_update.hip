// In-place updates of the IVF index (include/cdml_ivf_update.h): the lists of an index that gained a
// chunk of rows or lost some are written as NEW arrays by one output-driven launch; a second launch finds ids in the lists.
//
//   k_ivf_lists_move  a block owns `rows_per_block` consecutive destination rows (256 for rows of up to 128 B, fewer for longer
//                     rows: about 32 KiB of payload a block).  Two block-uniform binary searches in new_start bracket the
//                     lists of the block's first and last row; a lane per row then finds its own list inside the bracket
//                     (0 or 1 steps unless the block spans many short lists), resolves its source -- a kept old row, through
//                     old_pos when there is one, or a chunk row through add_order -- stores the row's id and r_sq and leaves
//                     the source address in LDS.  After the one barrier all 256 lanes copy the block's payload as one run of
//                     16-byte (or 8-byte) pieces, four loads in flight a lane: consecutive lanes store consecutive
//                     destination bytes whatever the row length is, and read consecutive source bytes wherever consecutive
//                     destination rows have consecutive sources (always inside the kept part of a list when old_pos is
//                     null).  No atomics; every destination byte is stored once; sources are clamped into their arrays.
//   k_ivf_locate      one thread per query id: assign -> list, a binary search among the list's ascending ids.
#include "common.h"
#include "../../include/cdml_ivf_update.h"

namespace cdml {
namespace {

typedef uint32_t v16_t __attribute__((ext_vector_type(4)));
typedef uint32_t v8_t __attribute__((ext_vector_type(2)));

constexpr int kMoveThreads = 256;
constexpr int kMoveInFlight = 4;
constexpr int64_t kMoveBlockBytes = 32768;

struct MoveArgs {
  const char *old_rows;
  int64_t old_ld;
  const int32_t *old_ids;
  const float *old_r_sq;
  int64_t n_old;
  const int32_t *old_pos;
  int64_t n_kept;
  const char *add_rows;
  int64_t add_ld;
  const float *add_r_sq;
  int64_t n_chunk;
  const int32_t *add_order;
  int64_t n_add;
  int32_t id0;
  const int32_t *kept_start, *add_start, *new_start;
  int nlist;
  int pieces;                  // per row
  char *new_rows;
  int64_t new_ld;
  int32_t *new_ids;
  float *new_r_sq;
  int64_t n_new;
  int rows_per_block;
};

// the last c in [lo, hi] with start[c] <= o (start[lo] <= o is the caller's invariant)
__device__ __forceinline__ int list_of(const int32_t *start, int64_t o, int lo, int hi) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)start[mid] <= o)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int64_t clamp_index(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

template <typename V>
__global__ void __launch_bounds__(kMoveThreads) k_ivf_lists_move(const MoveArgs a) {
  __shared__ const char *sSrc[kMoveThreads];
  const int t = threadIdx.x, R = a.rows_per_block;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int64_t left = a.n_new - r0;
  const int nr = left < R ? (int)left : R;     // >= 1: the grid is ceil(n_new / R)
  const int c_lo = list_of(a.new_start, r0, 0, a.nlist - 1);
  const int c_hi = list_of(a.new_start, r0 + nr - 1, c_lo, a.nlist - 1);
  if (t < nr) {
    const int64_t o = r0 + t;
    const int c = list_of(a.new_start, o, c_lo, c_hi);
    const int64_t off = o - a.new_start[c];
    const int64_t k0 = a.kept_start[c], kept_c = (int64_t)a.kept_start[c + 1] - k0;
    const char *src = nullptr;
    int32_t id = -1;
    float rs = 0.f;
    if (off < kept_c) {
      int64_t p = k0 + off;
      if (a.old_pos) p = a.n_kept > 0 ? (int64_t)a.old_pos[clamp_index(p, a.n_kept)] : -1;
      if (a.n_old > 0 && p >= 0) {
        p = clamp_index(p, a.n_old);
        src = a.old_rows + p * a.old_ld;
        id = a.old_ids[p];
        rs = a.old_r_sq[p];
      }
    } else if (a.n_add > 0 && a.n_chunk > 0) {
      const int64_t j = clamp_index(a.add_order[clamp_index(a.add_start[c] + (off - kept_c), a.n_add)], a.n_chunk);
      src = a.add_rows + j * a.add_ld;
      id = a.id0 + (int32_t)j;
      rs = a.add_r_sq[j];
    }
    sSrc[t] = src;
    a.new_ids[o] = id;
    a.new_r_sq[o] = rs;
  }
  __syncthreads();
  const uint32_t P = (uint32_t)a.pieces, total = (uint32_t)nr * P;
  char *dst0 = a.new_rows + r0 * a.new_ld;
  for (uint32_t base = t; base < total; base += kMoveThreads * kMoveInFlight) {
    V v[kMoveInFlight];
    uint32_t row[kMoveInFlight], pc[kMoveInFlight];
#pragma unroll
    for (int u = 0; u < kMoveInFlight; ++u) {
      const uint32_t i = base + kMoveThreads * u;
      v[u] = V(0);
      if (i < total) {
        row[u] = i / P;
        pc[u] = i - row[u] * P;
        const char *s = sSrc[row[u]];
        if (s) v[u] = *reinterpret_cast<const V *>(s + (size_t)pc[u] * sizeof(V));
      }
    }
#pragma unroll
    for (int u = 0; u < kMoveInFlight; ++u) {
      const uint32_t i = base + kMoveThreads * u;
      if (i < total) *reinterpret_cast<V *>(dst0 + (int64_t)row[u] * a.new_ld + (size_t)pc[u] * sizeof(V)) = v[u];
    }
  }
}

__global__ void __launch_bounds__(256)
k_ivf_locate(const int64_t *__restrict__ q_ids, int64_t nq, const int64_t *__restrict__ assign, int64_t n_rows,
             const int32_t *__restrict__ ids, int64_t n_listed, const int32_t *__restrict__ list_start, int nlist,
             int32_t *__restrict__ pos) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int64_t id = q_ids[q];
  int32_t found = -1;
  if (id >= 0 && id < n_rows) {
    const int64_t c = assign[id];
    if (c >= 0 && c < nlist) {
      int64_t lo = list_start[c], hi = list_start[c + 1];      // [lo, hi), clamped into the lists
      lo = lo < 0 ? 0 : lo;
      hi = hi > n_listed ? n_listed : hi;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t v = ids[mid];
        if (v < id)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < n_listed && lo < (int64_t)list_start[c + 1] && (int64_t)ids[lo] == id) found = (int32_t)lo;
    }
  }
  pos[q] = found;
}

constexpr int64_t kMaxRows = 0x7fffffff;

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_ivf_lists_move(const void *old_rows, int64_t old_ld, const int32_t *old_ids, const float *old_r_sq,
                                   int64_t n_old, const int32_t *old_pos, int64_t n_kept, const void *add_rows, int64_t add_ld,
                                   const float *add_r_sq, int64_t n_chunk, const int32_t *add_order, int64_t n_add, int32_t id0,
                                   const int32_t *kept_start, const int32_t *add_start, const int32_t *new_start, int nlist,
                                   int64_t row_bytes, void *new_rows, int64_t new_ld, int32_t *new_ids, float *new_r_sq,
                                   int64_t n_new, cdml_stream_t stream) {
  CDML_REQUIRE(kept_start && add_start && new_start && new_rows && new_ids && new_r_sq, CDML_E_BADARG,
               "ivf_lists_move: null pointer (the start tables and the new arrays)");
  CDML_REQUIRE(n_new > 0 && nlist > 0, CDML_E_BADARG, "ivf_lists_move: n_new and nlist must be positive");
  CDML_REQUIRE(n_old >= 0 && n_kept >= 0 && n_chunk >= 0 && n_add >= 0 && id0 >= 0, CDML_E_BADARG,
               "ivf_lists_move: n_old, n_kept, n_chunk, n_add and id0 must not be negative");
  CDML_REQUIRE(n_new <= kMaxRows && n_old <= kMaxRows && n_chunk <= kMaxRows && (int64_t)id0 + n_chunk <= kMaxRows,
               CDML_E_UNSUPPORTED, "ivf_lists_move: too large: positions and ids are int32 (n_new, n_old, id0 + n_chunk <= 2^31 - 1)");
  CDML_REQUIRE(n_kept + n_add == n_new && n_add <= n_chunk && (old_pos ? n_kept <= kMaxRows : n_kept <= n_old), CDML_E_BADARG,
               "ivf_lists_move: sizes disagree: n_kept + n_add == n_new, n_add <= n_chunk, n_kept <= n_old without old_pos");
  CDML_REQUIRE(n_old == 0 || (old_rows && old_ids && old_r_sq), CDML_E_BADARG, "ivf_lists_move: null pointer (old arrays with n_old > 0)");
  CDML_REQUIRE(n_kept == 0 || n_old > 0, CDML_E_BADARG, "ivf_lists_move: sizes disagree: n_kept > 0 with n_old = 0");
  CDML_REQUIRE(n_chunk == 0 || (add_rows && add_r_sq), CDML_E_BADARG, "ivf_lists_move: null pointer (chunk arrays with n_chunk > 0)");
  CDML_REQUIRE(n_add == 0 || add_order, CDML_E_BADARG, "ivf_lists_move: null pointer (add_order with n_add > 0)");
  CDML_REQUIRE(row_bytes > 0 && row_bytes % 8 == 0 && row_bytes <= (1 << 20), CDML_E_BADARG,
               "ivf_lists_move: row_bytes must be a positive multiple of 8 (at most 2^20), got %lld", (long long)row_bytes);
  CDML_REQUIRE(new_ld >= row_bytes && new_ld % 8 == 0 && (n_old == 0 || (old_ld >= row_bytes && old_ld % 8 == 0)) &&
                   (n_chunk == 0 || (add_ld >= row_bytes && add_ld % 8 == 0)),
               CDML_E_BADARG, "ivf_lists_move: every stride must be a multiple of 8 and >= row_bytes = %lld", (long long)row_bytes);
  CDML_REQUIRE(aligned16(new_rows) && aligned16(old_rows) && aligned16(add_rows), CDML_E_ALIGN,
               "ivf_lists_move: the payload bases must be 16-B aligned");
  const bool wide = row_bytes % 16 == 0 && new_ld % 16 == 0 && (n_old == 0 || old_ld % 16 == 0) && (n_chunk == 0 || add_ld % 16 == 0);
  int R = kMoveThreads;
  while (R > 8 && R * row_bytes > kMoveBlockBytes) R >>= 1;
  MoveArgs a;
  a.old_rows = (const char *)old_rows, a.old_ld = old_ld, a.old_ids = old_ids, a.old_r_sq = old_r_sq, a.n_old = n_old;
  a.old_pos = old_pos, a.n_kept = n_kept;
  a.add_rows = (const char *)add_rows, a.add_ld = add_ld, a.add_r_sq = add_r_sq, a.n_chunk = n_chunk;
  a.add_order = add_order, a.n_add = n_add, a.id0 = id0;
  a.kept_start = kept_start, a.add_start = add_start, a.new_start = new_start, a.nlist = nlist;
  a.pieces = (int)(row_bytes / (wide ? 16 : 8));
  a.new_rows = (char *)new_rows, a.new_ld = new_ld, a.new_ids = new_ids, a.new_r_sq = new_r_sq, a.n_new = n_new;
  a.rows_per_block = R;
  const dim3 grid((unsigned)((n_new + R - 1) / R));
  hipStream_t st = (hipStream_t)stream;
  if (wide)
    hipLaunchKernelGGL(k_ivf_lists_move<v16_t>, grid, dim3(kMoveThreads), 0, st, a);
  else
    hipLaunchKernelGGL(k_ivf_lists_move<v8_t>, grid, dim3(kMoveThreads), 0, st, a);
  return check_launch("ivf_lists_move");
}

extern "C" int cdml_ivf_locate(const int64_t *q_ids, int64_t nq, const int64_t *assign, int64_t n_rows, const int32_t *ids,
                               int64_t n_listed, const int32_t *list_start, int nlist, int32_t *pos, cdml_stream_t stream) {
  CDML_REQUIRE(q_ids && assign && list_start && pos, CDML_E_BADARG, "ivf_locate: null pointer");
  CDML_REQUIRE(nq > 0 && n_rows > 0 && nlist > 0, CDML_E_BADARG, "ivf_locate: nq, n_rows and nlist must be positive");
  CDML_REQUIRE(n_listed >= 0 && n_listed <= n_rows, CDML_E_BADARG, "ivf_locate: n_listed must be in [0, n_rows]");
  CDML_REQUIRE(n_listed == 0 || ids, CDML_E_BADARG, "ivf_locate: null pointer (ids with n_listed > 0)");
  CDML_REQUIRE(nq <= kMaxRows && n_rows <= kMaxRows, CDML_E_UNSUPPORTED, "ivf_locate: too large: nq and n_rows <= 2^31 - 1");
  hipLaunchKernelGGL(k_ivf_locate, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q_ids, nq, assign,
                     n_rows, ids, n_listed, list_start, nlist, pos);
  return check_launch("ivf_locate");
}

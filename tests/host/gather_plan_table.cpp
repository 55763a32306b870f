// The argument checks and launch plans of the sampler + gather entry points (csrc/gather_plan.h) as a table: one line per
// entry point and case,
//     format entry case status "message" rpt grid nch ki
// -- valid baselines (the headline shape, every NCH bucket edge, every mode, n_steps 1 and 4, with and without x_ki) and
// every single-fault variation of a baseline, one per clause of a check.  Host program: includes only csrc/gather_plan.h,
// no HIP; pointers are placeholder addresses that nothing dereferences.  tests/test_gather_plan_host.py compiles it and
// compares its output with tests/data/gather_plan_table.txt, which was made from the library BEFORE the checks were
// gathered in the header (`--args` prints every case's arguments instead: what that library was called with).
#include "../../collaborative-deep-metric-learning_amd/csrc/gather_plan.h"
#include <functional>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

static char g_msg[512];
int cdml::fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}

using namespace cdml;

static bool g_args = false;
template <typename T> static T *at(uintptr_t a) { return reinterpret_cast<T *>(a); }
static unsigned long long u(const void *p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }
static int up(int v, int m) { return (v + m - 1) / m * m; }

// what each C entry point hands to the plan: cdml_<name> checks under `who` with the format's rules
struct Entry {
  const char *name, *fmt_name, *who;
  const GatherFormat *fmt;
  bool fused, listed, ki_entry, ki_optional, row0;
};
static const Entry kEntries[] = {
    {"sample_gather", "f32", "sample_gather", &kGatherF32, true, false, false, false, false},
    {"sample_gather_f16", "f16", "sample_gather_f16", &kGatherF16, true, false, false, false, false},
    {"sample_gather_x3", "x3", "sample_gather_x3", &kGatherX3, true, false, false, false, false},
    {"sample_gather_x3k", "x3", "sample_gather_x3", &kGatherX3, true, false, true, false, false},
    {"sample_gather_h2", "h2", "sample_gather_h2", &kGatherH2, true, false, false, false, false},
    {"sample_gather_listed", "f32", "sample_gather", &kGatherF32, true, true, false, false, false},
    {"sample_gather_listed_x3", "x3", "sample_gather_x3", &kGatherX3, true, true, false, true, false},
    {"sample_gather_listed_f16", "f16", "sample_gather_f16", &kGatherF16, true, true, false, false, false},
    {"gather_rows", "f32", "gather_rows", &kGatherF32, false, false, false, false, true},
    {"gather_rows_x3", "x3", "gather_rows_x3", &kGatherX3, false, false, false, false, false},
    {"gather_rows_f16", "f16", "gather_rows_f16", &kGatherF16, false, false, false, false, true},
};

static void result(const Entry &e, const std::string &cs, int rc, const GatherPlan &p) {
  if (rc) printf("%s %s %s %d \"%s\" - - - -\n", e.fmt_name, e.name, cs.c_str(), rc, g_msg);
  else printf("%s %s %s 0 \"\" %d %d %d %d\n", e.fmt_name, e.name, cs.c_str(), p.rpt, p.grid, p.nch, (int)p.ki);
}

static void emit(const Entry &e, const std::string &cs, SampleGatherArgs a, const ListedArgs &l) {
  a.ki_entry = e.ki_entry;
  a.listed = e.listed ? &l : nullptr;
  if (!e.ki_entry && !e.ki_optional) a.x_ki = nullptr, a.ki_step_stride = 0;      // (the entry point has no such parameters)
  if (g_args) {
    printf("%s %s %d %llu %lld %llu %llu %llu %d %lld %lld %llu %lld %lld %d %llu %llu %llu %lld %d %lld %lld %llu %llu %lld %llu %lld %d %llu %llu %lld\n",
           e.name, cs.c_str(), a.mode, u(a.pairs), (long long)a.n_pairs, (unsigned long long)a.seed, (unsigned long long)a.step,
           u(a.step_dev), a.batch, (long long)a.slot0, (long long)a.batch_global, u(a.table), (long long)a.n_rows,
           (long long)a.row_stride, a.F, u(a.idx_out), u(a.shift_out), u(a.x_out), (long long)a.out_stride, a.n_steps,
           (long long)a.x_step_stride, (long long)a.idx_step_stride, u(a.oob_flag), u(a.x_ki), (long long)a.ki_step_stride,
           u(l.lists), (long long)l.ldl, l.L, (unsigned long long)l.hard_thresh, u(l.kind_out), (long long)l.kind_step_stride);
    return;
  }
  GatherPlan p{};
  g_msg[0] = 0;
  result(e, cs, plan_sample_gather(e.who, *e.fmt, a, p), p);
}

static void emit_rows(const Entry &e, const std::string &cs, GatherRowsArgs a) {
  if (!e.row0) a.row0 = 0;
  if (g_args) {
    printf("%s %s %llu %lld %lld %lld %llu %d %d %llu %lld\n", e.name, cs.c_str(), u(a.table), (long long)a.row0,
           (long long)a.n_rows, (long long)a.row_stride, u(a.idx), a.n_idx, a.F, u(a.x_out), (long long)a.out_stride);
    return;
  }
  GatherPlan p{};
  g_msg[0] = 0;
  result(e, cs, plan_gather_rows(e.who, *e.fmt, a, p), p);
}

// a valid fused call: strides with slack (twice the batch's need), so that one changed argument trips one check
static SampleGatherArgs fused_base(const Entry &e, int mode, int F, int batch, int n_steps, bool ki, ListedArgs &l) {
  const GatherFormat &f = *e.fmt;
  const int plane = up(F, 256), rpt = mode == 1 ? 2 : 3;
  const int64_t rows = (int64_t)batch * rpt, out_stride = (int64_t)plane * f.planes;
  SampleGatherArgs a{};
  a.mode = mode;
  a.pairs = at<const int32_t>(0x10000), a.n_pairs = 1 << 22, a.seed = 1234, a.step = 7, a.step_dev = nullptr;
  a.batch = batch, a.slot0 = 0, a.batch_global = batch;
  a.table = at<const void>(0x20000), a.n_rows = 1 << 20, a.row_stride = plane, a.F = F;
  a.idx_out = at<int32_t>(0x30000), a.shift_out = e.listed ? nullptr : at<int32_t>(0x40000);
  a.x_out = at<void>(0x50000), a.out_stride = out_stride;
  a.n_steps = n_steps;
  a.x_step_stride = n_steps > 1 ? 2 * rows * out_stride : 0, a.idx_step_stride = n_steps > 1 ? 2 * rows : 0;
  a.oob_flag = at<int32_t>(0x60000);
  a.x_ki = ki ? at<void>(0x70000) : nullptr, a.ki_step_stride = (ki && n_steps > 1) ? 2 * 3 * rows * plane : 0;
  l = ListedArgs{at<const int32_t>(0x80000), 32, 24, 1ull << 31, at<int32_t>(0x90000), n_steps > 1 ? 2 * batch : 0};
  return a;
}

static GatherRowsArgs rows_base(const Entry &e, int F, int n_idx) {
  const int plane = up(F, 256);
  return GatherRowsArgs{at<const void>(0x20000), 64, 1 << 20, plane, at<const int32_t>(0x30000), n_idx, F, at<void>(0x50000),
                        (int64_t)plane * e.fmt->planes};
}

using Fault = std::function<void(SampleGatherArgs &, ListedArgs &)>;
using RowsFault = std::function<void(GatherRowsArgs &)>;

// F at every edge of a bucket list -- the largest F a bucket's registers hold (64 lanes x NCH chunks) and one chunk more --
// and the largest F of the format.  fp32 table, buckets 2 6 8: 512 516 1536 1540 2048; fp16 table, 1 3 8: 512 520 1536 1544 4096
static void bucket_edges(const GatherFormat &f, const NchBuckets &b, std::vector<int> &F) {
  auto add = [&F](int v) {
    for (int have : F)
      if (have == v) return;
    F.push_back(v);
  };
  for (int i = 0; i + 1 < b.n; ++i) add(64 * f.per_chunk * b.v[i]), add(64 * f.per_chunk * b.v[i] + f.per_chunk);
  add(f.max_f);
}

static void fused_cases(const Entry &e) {
  const GatherFormat &f = *e.fmt;
  std::vector<int> edges = {1500};                                               // the headline F, then the format's own edges
  bucket_edges(f, f.fused, edges);
  if (f.per_chunk == 4) bucket_edges(f, kGatherF32.fused, edges);                // (the plane formats also at the fp32 rows' 2 | 6 edge)
  const bool with_ki = e.ki_entry || e.ki_optional;
  ListedArgs l{};
  char cs[96];
  // ---- valid baselines ----
  for (int mode = e.listed ? 2 : 0; mode <= (e.listed ? 2 : 1); ++mode)
    for (int F : edges)
      for (int n_steps = 1; n_steps <= 4; n_steps += 3)
        for (int ki = e.ki_entry ? 1 : 0; ki <= (with_ki ? 1 : 0); ++ki) {
          const int batch = F == 1500 ? 16384 : 256;
          snprintf(cs, sizeof cs, "ok_mode%d_F%d_steps%d_ki%d", mode, F, n_steps, ki);
          emit(e, cs, fused_base(e, mode, F, batch, n_steps, ki, l), l);
        }
  {  // the smallest launches, the batches either side of the grid's cap (fp32: 2 048 blocks of 8 rows), what may be absent
    const int m = e.listed ? 2 : 0;
    SampleGatherArgs a = fused_base(e, m, 96, 1, 1, false, l);
    if (!e.ki_entry) emit(e, "ok_batch1", a, l);
    a = fused_base(e, m, 1500, 8, 2, with_ki, l);
    emit(e, "ok_batch8", a, l);
    a.oob_flag = nullptr, a.step_dev = at<const uint64_t>(0xA0000);
    emit(e, "ok_no_oob_flag_step_dev", a, l);
    a = fused_base(e, m, 1500, 8, 2, with_ki, l);
    a.x_out = at<void>(0x50008);
    emit(e, "x_out_8B_aligned", a, l);                                           // enough for the plane formats only
    if (!e.ki_entry) {
      emit(e, "ok_batch2730", fused_base(e, m, 1500, 2730, 2, false, l), l);
      emit(e, "ok_batch2731", fused_base(e, m, 1500, 2731, 2, false, l), l);
    }
  }
  // ---- single faults of the headline baseline: four steps, x_ki where the entry takes one ----
  std::vector<std::pair<const char *, Fault>> faults = {
      {"null_pairs", [](SampleGatherArgs &a, ListedArgs &) { a.pairs = nullptr; }},
      {"null_table", [](SampleGatherArgs &a, ListedArgs &) { a.table = nullptr; }},
      {"null_idx_out", [](SampleGatherArgs &a, ListedArgs &) { a.idx_out = nullptr; }},
      {"null_x_out", [](SampleGatherArgs &a, ListedArgs &) { a.x_out = nullptr; }},
      {"n_pairs_0", [](SampleGatherArgs &a, ListedArgs &) { a.n_pairs = 0; }},
      {"slot0_negative", [](SampleGatherArgs &a, ListedArgs &) { a.slot0 = -1; }},
      {"n_steps_0", [](SampleGatherArgs &a, ListedArgs &) { a.n_steps = 0; }},
      {"n_steps_65", [](SampleGatherArgs &a, ListedArgs &) { a.n_steps = 65; }},
      {"x_step_stride_small", [](SampleGatherArgs &a, ListedArgs &) { a.x_step_stride = a.x_step_stride / 2 - 8; }},
      {"x_step_stride_exact", [](SampleGatherArgs &a, ListedArgs &) { a.x_step_stride /= 2; }},
      {"x_step_stride_plus1", [](SampleGatherArgs &a, ListedArgs &) { a.x_step_stride += 1; }},
      {"x_step_stride_plus4", [](SampleGatherArgs &a, ListedArgs &) { a.x_step_stride += 4; }},
      {"idx_step_stride_small", [](SampleGatherArgs &a, ListedArgs &) { a.idx_step_stride = a.idx_step_stride / 2 - 1; }},
      {"row_stride_small", [](SampleGatherArgs &a, ListedArgs &) { a.row_stride = 1496; }},
      {"row_stride_plus1", [](SampleGatherArgs &a, ListedArgs &) { a.row_stride += 1; }},
      {"row_stride_plus4", [](SampleGatherArgs &a, ListedArgs &) { a.row_stride += 4; }},
      {"out_stride_small", [&f](SampleGatherArgs &a, ListedArgs &) { a.out_stride = 1496 * f.planes; }},
      {"out_stride_plus1", [](SampleGatherArgs &a, ListedArgs &) { a.out_stride += 1; }},
      {"out_plane_plus1", [&f](SampleGatherArgs &a, ListedArgs &) { a.out_stride += f.planes; }},
      {"out_plane_plus4", [&f](SampleGatherArgs &a, ListedArgs &) { a.out_stride += 4 * f.planes; }},
      {"table_4B_aligned", [](SampleGatherArgs &a, ListedArgs &) { a.table = at<const void>(0x20004); }},
      {"table_8B_aligned", [](SampleGatherArgs &a, ListedArgs &) { a.table = at<const void>(0x20008); }},
      {"x_out_4B_aligned", [](SampleGatherArgs &a, ListedArgs &) { a.x_out = at<void>(0x50004); }},
      {"F_0", [](SampleGatherArgs &a, ListedArgs &) { a.F = 0; }},
      {"F_negative", [](SampleGatherArgs &a, ListedArgs &) { a.F = -4; }},
      {"F_max_plus1", [&f](SampleGatherArgs &a, ListedArgs &) { a.F = f.max_f + 1; }},
      {"n_rows_2", [](SampleGatherArgs &a, ListedArgs &) { a.n_rows = 2; }},
      {"n_rows_2p31", [](SampleGatherArgs &a, ListedArgs &) { a.n_rows = 1ll << 31; }},
      {"batch_0", [](SampleGatherArgs &a, ListedArgs &) { a.batch = 0; }},
      {"batch_global_short", [](SampleGatherArgs &a, ListedArgs &) { a.batch_global = a.batch - 1; }},
      {"slot0_past_batch_global", [](SampleGatherArgs &a, ListedArgs &) { a.slot0 = 1; }},
      {"mode_minus1", [](SampleGatherArgs &a, ListedArgs &) { a.mode = -1; }},
      {"mode_2", [](SampleGatherArgs &a, ListedArgs &) { a.mode = 2; }},
      {"mode_3", [](SampleGatherArgs &a, ListedArgs &) { a.mode = 3; }},
  };
  for (auto &ft : faults) {
    if (e.listed && !strncmp(ft.first, "mode_", 5)) continue;                     // (the listed entry points take no mode)
    SampleGatherArgs a = fused_base(e, e.listed ? 2 : 0, 1500, 16384, 4, with_ki, l);
    ft.second(a, l);
    emit(e, ft.first, a, l);
  }
  if (!e.listed) {                                                               // mode 1's own
    SampleGatherArgs a = fused_base(e, 1, 1500, 16384, 4, with_ki, l);
    a.shift_out = nullptr;
    emit(e, "mode1_null_shift_out", a, l);
    a = fused_base(e, 1, 1500, 16384, 4, with_ki, l);
    a.batch = a.batch_global = 1;
    emit(e, "mode1_batch_1", a, l);
    a = fused_base(e, 0, 1500, 16384, 4, with_ki, l);
    a.shift_out = nullptr;
    emit(e, "mode0_null_shift_out", a, l);
  }
  if (with_ki) {                                                                 // the interleave rule
    std::vector<std::pair<const char *, Fault>> ki = {
        {"ki_null_x_ki", [](SampleGatherArgs &a, ListedArgs &) { a.x_ki = nullptr; }},
        {"ki_rows_not_8", [](SampleGatherArgs &a, ListedArgs &) { a.batch = a.batch_global = 9; }},
        {"ki_plane_not_256", [](SampleGatherArgs &a, ListedArgs &) { a.out_stride = 3 * 1540; }},
        {"ki_x_ki_8B_aligned", [](SampleGatherArgs &a, ListedArgs &) { a.x_ki = at<void>(0x70008); }},
        {"ki_step_stride_small", [](SampleGatherArgs &a, ListedArgs &) { a.ki_step_stride = a.ki_step_stride / 2 - 8; }},
        {"ki_step_stride_exact", [](SampleGatherArgs &a, ListedArgs &) { a.ki_step_stride /= 2; }},
        {"ki_plane_past_nch6", [](SampleGatherArgs &a, ListedArgs &) { a.F = 512, a.out_stride = 3 * 1792; }},
        {"ki_plane_at_nch6", [](SampleGatherArgs &a, ListedArgs &) { a.F = 512, a.out_stride = 3 * 1536; }},
        {"ki_plane_past_nch8", [](SampleGatherArgs &a, ListedArgs &) { a.F = 1540, a.row_stride = 2048, a.out_stride = 3 * 2304; }},
    };
    for (int mode = e.listed ? 2 : 0; mode <= (e.listed ? 2 : 1); ++mode)
      for (auto &ft : ki) {
        SampleGatherArgs a = fused_base(e, mode, 1500, 16384, 4, true, l);
        a.x_step_stride *= 2;                                                    // (room for the wider planes)
        ft.second(a, l);
        snprintf(cs, sizeof cs, "%s_mode%d", ft.first, mode);
        emit(e, cs, a, l);
      }
  }
  if (e.listed) {
    std::vector<std::pair<const char *, Fault>> lf = {
        {"listed_null_lists", [](SampleGatherArgs &, ListedArgs &l) { l.lists = nullptr; }},
        {"listed_L_0", [](SampleGatherArgs &, ListedArgs &l) { l.L = 0; }},
        {"listed_L_1025", [](SampleGatherArgs &, ListedArgs &l) { l.L = 1025, l.ldl = 1025; }},
        {"listed_L_1024", [](SampleGatherArgs &, ListedArgs &l) { l.L = 1024, l.ldl = 1024; }},
        {"listed_ldl_short", [](SampleGatherArgs &, ListedArgs &l) { l.ldl = l.L - 1; }},
        {"listed_thresh_past_2p32", [](SampleGatherArgs &, ListedArgs &l) { l.hard_thresh = (1ull << 32) + 1; }},
        {"listed_thresh_2p32", [](SampleGatherArgs &, ListedArgs &l) { l.hard_thresh = 1ull << 32; }},
        {"listed_kind_stride_short", [](SampleGatherArgs &a, ListedArgs &l) { l.kind_step_stride = a.batch - 1; }},
        {"listed_kind_stride_exact", [](SampleGatherArgs &a, ListedArgs &l) { l.kind_step_stride = a.batch; }},
        {"listed_no_kind_out", [](SampleGatherArgs &, ListedArgs &l) { l.kind_out = nullptr, l.kind_step_stride = 0; }},
    };
    for (auto &ft : lf) {
      SampleGatherArgs a = fused_base(e, 2, 1500, 16384, 4, with_ki, l);
      ft.second(a, l);
      emit(e, ft.first, a, l);
    }
  }
}

static void rows_cases(const Entry &e) {
  const GatherFormat &f = *e.fmt;
  char cs[96];
  std::vector<int> edges = {64, 1500};
  bucket_edges(f, f.rows, edges);                                                // fp32: buckets 2 4 6 8; fp16 table: 1 3 8
  for (int F : edges) {
    snprintf(cs, sizeof cs, "ok_F%d", F);
    emit_rows(e, cs, rows_base(e, F, 49152));
  }
  const int counts[] = {1, 4, 5, 24, 8192, 8193, 1000000};
  for (int n : counts) {
    snprintf(cs, sizeof cs, "ok_n_idx%d", n);
    emit_rows(e, cs, rows_base(e, 1500, n));
  }
  std::vector<std::pair<const char *, RowsFault>> faults = {
      {"null_table", [](GatherRowsArgs &a) { a.table = nullptr; }},
      {"null_idx", [](GatherRowsArgs &a) { a.idx = nullptr; }},
      {"null_x_out", [](GatherRowsArgs &a) { a.x_out = nullptr; }},
      {"n_rows_0", [](GatherRowsArgs &a) { a.n_rows = 0; }},
      {"n_idx_0", [](GatherRowsArgs &a) { a.n_idx = 0; }},
      {"row0_negative", [](GatherRowsArgs &a) { a.row0 = -1; }},
      {"F_0", [](GatherRowsArgs &a) { a.F = 0; }},
      {"F_max_plus1", [&f](GatherRowsArgs &a) { a.F = f.max_f + 1; }},
      {"row_stride_small", [](GatherRowsArgs &a) { a.row_stride = 1496; }},
      {"row_stride_plus1", [](GatherRowsArgs &a) { a.row_stride += 1; }},
      {"row_stride_plus4", [](GatherRowsArgs &a) { a.row_stride += 4; }},
      {"out_stride_small", [&f](GatherRowsArgs &a) { a.out_stride = 1496 * f.planes; }},
      {"out_stride_plus1", [](GatherRowsArgs &a) { a.out_stride += 1; }},
      {"out_plane_plus1", [&f](GatherRowsArgs &a) { a.out_stride += f.planes; }},
      {"out_plane_plus4", [&f](GatherRowsArgs &a) { a.out_stride += 4 * f.planes; }},
      {"table_8B_aligned", [](GatherRowsArgs &a) { a.table = at<const void>(0x20008); }},
      {"x_out_4B_aligned", [](GatherRowsArgs &a) { a.x_out = at<void>(0x50004); }},
      {"x_out_8B_aligned", [](GatherRowsArgs &a) { a.x_out = at<void>(0x50008); }},
  };
  for (auto &ft : faults) {
    GatherRowsArgs a = rows_base(e, 1500, 49152);
    ft.second(a);
    emit_rows(e, ft.first, a);
  }
}

int main(int argc, char **argv) {
  g_args = argc > 1 && !strcmp(argv[1], "--args");
  for (const Entry &e : kEntries) {
    if (e.fused) fused_cases(e);
    else rows_cases(e);
  }
  return 0;
}

// The K-split plans of the plane GEMMs and the plain-bf16 k-strided product as a table: one line per shape and form,
//     form M N K products ktiles period per splits need workspace
// (`workspace` = what the form's workspace query answers for the shape), checked line by line for the properties the
// entries rely on.  Host program: includes only csrc/gemm_plan.h, no HIP.  tests/test_gemm_plan_host.py compiles it,
// compares its output with tests/data/gemm_plan_table.txt and the workspace column with the built library.
#include "../../collaborative-deep-metric-learning_amd/csrc/gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>

using namespace cdml;

#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    if (!(cond)) {                                                                                               \
      fprintf(stderr, "%s:%d: %s fails at M=%d N=%d K=%d products=%d\n", __FILE__, __LINE__, #cond, M, N, K, products); \
      exit(1);                                                                                                   \
    }                                                                                                            \
  } while (0)

static bool same(const KSplitPlan &a, const KSplitPlan &b) {
  return a.ktiles == b.ktiles && a.period == b.period && a.per == b.per && a.splits == b.splits && a.slabs == b.slabs &&
         a.slab_bytes == b.slab_bytes && a.cs_rows == b.cs_rows && a.cs_bytes == b.cs_bytes && a.need == b.need;
}

static size_t f16x2_workspace(int tn, int M, int N, int K) {      // cdml_gemm_f16x2_workspace
  const size_t a = x3_workspace_bytes(tn, M, N, K, 6), b = x3_workspace_bytes(tn, M, N, K, 3);
  return a > b ? a : b;
}

static void row(const char *form, int M, int N, int K, int products, const KSplitPlan &p, size_t workspace) {
  CHECK(p.per % p.period == 0);
  CHECK((int64_t)(p.splits - 1) * p.per < p.ktiles && p.ktiles <= (int64_t)p.splits * p.per);      // no split is empty
  CHECK(p.need <= workspace);
  printf("%s %d %d %d %d %d %d %d %d %zu %zu\n", form, M, N, K, products, p.ktiles, p.period, p.per, p.splits, p.need, workspace);
}

int main() {
  const int Ms[] = {256, 512, 3072, 8192, 16384, 24576, 49152}, Ns[] = {256, 512, 1536, 5120};
  const int Ks[] = {128, 256, 640, 1280, 1536, 3072, 5120, 8192, 24576};
  const int pins[] = {60, 120, 0};                                 // cdml_x3_slab_steps: 0 = by row-tile class
  for (int N : Ns)
    for (int K : Ks)
      for (int f16 = 0; f16 < 2; ++f16)
        for (int products = 3; products <= 6; products += 3) {
          if (f16 && products != 3) continue;
          // ---- k-contiguous form ----
          if (K % 64 == 0 && products * (K / 64) % 2 == 0) {
            KSplitPlan of_class[2] = {};
            bool seen[2] = {false, false};
            for (int M : Ms) {
              const size_t ws = f16 ? f16x2_workspace(0, M, N, K) : x3_workspace_bytes(0, M, N, K, products);
              for (int pin : pins)
                for (int colsum = 0; colsum < 2; ++colsum)
                  for (int have = 0; have < 2; ++have)
                    for (int planes = 0; planes < 2; ++planes)
                      CHECK(x3_plan_nt(M, N, K, products, f16, planes, colsum, pin, 6, have).need <= ws);
              const KSplitPlan p = x3_plan_nt(M, N, K, products, f16, false, false, 0, 6, true);
              row(f16 ? "nt_f16" : "nt", M, N, K, products, p, ws);
              // the partition depends on K and on the row-tile class alone
              int s120 = products * (K / 64) * (f16 ? 2 : 1) / 120;
              s120 = s120 < 1 ? 1 : (s120 > 16 ? 16 : s120);
              const int c = (M + 255) / 256 * s120 <= 64 ? 0 : 1;
              if (seen[c]) CHECK(p.per == of_class[c].per && p.splits == of_class[c].splits);
              of_class[c] = p; seen[c] = true;
            }
          }
          // ---- k-strided form ----
          if (K % 128 == 0)
            for (int M : Ms) {
              const size_t ws = f16 ? f16x2_workspace(1, M, N, K) : x3_workspace_bytes(1, M, N, K, products);
              for (int kmajor = 0; kmajor < 2; ++kmajor)
                for (int bias = 0; bias < 2; ++bias)
                  for (int colsum = 0; colsum < 2; ++colsum)
                    CHECK(x3_plan_tn(M, N, K, products, x3_tn_period(products, kmajor, f16), bias, colsum).need <= ws);
              const KSplitPlan p = x3_plan_tn(M, N, K, products, x3_tn_period(products, true, f16), false, true);
              row(f16 ? "tn_f16" : "tn", M, N, K, products, p, ws);
              if (!f16 && products == 6) {      // cdml_gemm_bf16x3_tnk / _tn_kb: six products, K-major -- the row-major form's plan
                const KSplitPlan k = x3_plan_tn(M, N, K, 6, x3_tn_period(6, true, false), false, true);
                CHECK(same(p, k));
              }
            }
        }
  // ---- plain bf16, k-strided (cdml_gemm_bf16_tn): every requested split is launched, so only the period is checked ----
  const int products = 1;
  for (int N : Ns)
    for (int K : Ks)
      if (K % 128 == 0)
        for (int M : Ms) {
          const KSplitPlan p = bf16_tn_plan(M, N, K, true);
          const size_t ws = p.need;                                 // cdml_gemm_bf16_tn_workspace
          CHECK(p.per % p.period == 0 && p.ktiles <= (int64_t)p.splits * p.per && bf16_tn_plan(M, N, K, false).need <= ws);
          printf("bf16_tn %d %d %d %d %d %d %d %d %zu %zu\n", M, N, K, products, p.ktiles, p.period, p.per, p.splits, p.need, ws);
        }
  return 0;
}

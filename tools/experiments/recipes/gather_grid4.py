# A/B: the persistent gather kernels on 4 blocks per CU instead of 8
EDITS = [("gather_plan.h", "const int64_t cap = (int64_t)kPlanNumCU * 8;", "const int64_t cap = (int64_t)kPlanNumCU * 4;")]

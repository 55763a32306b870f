// The argument checks' vocabulary: the status codes, the per-thread error message and CDML_REQUIRE.  No HIP -- what the
// HIP-free plan headers (gather_plan.h) and common.h share.
#pragma once
#include "../../include/cdml.h"

namespace cdml {

// ---- per-thread error message ------------------------------------------------
char *err_buf();
int fail(int code, const char *fmt, ...);

#define CDML_REQUIRE(cond, code, ...)                  \
  do {                                                 \
    if (!(cond)) return ::cdml::fail((code), __VA_ARGS__); \
  } while (0)

}  // namespace cdml

// Error reporting of every translation unit of the library: fail() formats the message behind tfk_last_error() and returns
// the (non-zero) code, CHK passes a failed step's code on, HIPCHK turns a HIP error into one.  The thread-local message
// itself lives in engine.hip, behind tfk::set_error.  Nothing here needs a HIP header: HIPCHK is a macro, and only a unit
// that includes <hip/hip_runtime.h> can use it.
#pragma once
#include <stdarg.h>
#include <stdio.h>

namespace tfk {

int set_error(int code, const char* msg);  // engine.hip; returns code

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return set_error(code ? code : -1, buf);
}

}  // namespace tfk

#define CHK(expr)             \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != 0) return rc_; \
  } while (0)
#define HIPCHK(expr)                                                                                        \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess)                                                                                   \
      return tfk::fail((int)e_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// csrc/pxr_match.hip as host code over the stand-in runtime of matrix/hip/hip_runtime.h (see there).
#include <cstdarg>
#include <cstdio>

#include "matrix/hip/hip_runtime.h"
uint3e threadIdx, blockIdx, blockDim;
EmuBlock emu_block;
#include "pxr_internal.h"
static thread_local char g_err[512];
namespace pxr {
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace pxr
extern "C" const char* emu_last_error() { return g_err; }
extern "C" pxr_ctx* emu_ctx() { return new pxr_ctx(); }
#include "pxr_match.hip"

// Test infrastructure: the prologue of every <stage>_on_host.cpp.  It brings in the stand-in runtime of hip/hip_runtime.h (see
// there) and pxr_internal.h, defines the runtime's globals and what a csrc/*.hip file expects of the library around it
// (pxr::set_error), and exports what tests/lanes.py needs of every emulation: emu_last_error, emu_ctx and emu_ctx_free.  A stage is
// this header, its .hip file and, where it has one, a main for the sanitized stand-alone build.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "hip/hip_runtime.h"
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
extern "C" void emu_ctx_free(pxr_ctx* ctx) {       // the workspace is all that the emulated entry points hang on a context
  free(ctx->d_workspace);
  delete ctx;
}

// csrc/pxr_match.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
#include "on_host.h"
#include "pxr_match.hip"

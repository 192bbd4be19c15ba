// tests/cpp/caller.h for the caller programs that hold device memory of their own and are built with hipcc: the check of a HIP runtime
// call.  A failing call ends the enclosing function with status 3 after a message on stderr.
#pragma once
#include <hip/hip_runtime_api.h>
#include "caller.h"

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 3; } } while (0)

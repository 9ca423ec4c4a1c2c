// torch's semantics on inf and NaN for the training kernels (DESIGN section
// 27): torch.clamp, torch.maximum, torch.amax and torch.relu keep a NaN, while
// fmaxf returns the operand that is not one. Training under a GradScaler needs
// the NaN: an overflow must stay non-finite until the optimizer finds it and
// skips the step.
//
// An object that includes this header is built with -fhonor-nans (Makefile):
// under the library's -fno-honor-nans the tests of a NaN below fold to false.
#pragma once
#include <hip/hip_runtime.h>

// max(a, b) that is NaN when either is; on any other pair it is fmaxf(a, b),
// the same instruction and the same bits as before
__device__ __forceinline__ float pm_max_nan(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return fmaxf(a, b);
}

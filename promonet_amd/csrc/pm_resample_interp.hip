// The interpolated-sinc resampler of the C ABI (include/promonet_hip.h):
// pm_resample_interp and its tile query. Kernel: pm_resample_interp.h. Every
// argument is checked before the first HIP call, so the checks answer on a
// machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_resample_interp.h"

static_assert(RI_P == PM_RESAMPLE_INTERP_STEPS &&
              RI_N + 1 == PM_RESAMPLE_INTERP_TABLE,
              "the kernel walks the table the header describes");

extern "C" int pm_resample_interp_tile(int orig, int new_) {
    if (orig < 1 || new_ < 1)
        return pm_fail(PM_EINVAL, "orig and new must be at least 1");
    if (orig >= RI_RATE_MAX || new_ >= RI_RATE_MAX)
        return pm_fail(PM_EINVAL, "rates %d -> %d: a rate must be below %d",
                       orig, new_, RI_RATE_MAX);
    if (pm_ri_segment(orig, new_) == 0)
        return pm_fail(PM_EINVAL, "resampling ratio %d / %d: the input "
                       "segment of %d outputs does not fit %d floats of LDS",
                       new_, orig, RI_TILE, RI_LDS_FLOATS);
    return RI_TILE;
}

extern "C" int pm_resample_interp(
    const float* x, const int* lengths, const int* orig, const int* new_,
    const float* win, const float* delta, float* out, int rows, int n_in,
    long long x_stride, int n_out, long long out_stride, void* stream) {
    if (rows < 0 || n_in < 0 || n_out < 0)
        return pm_fail(PM_EINVAL, "negative size");
    if (!x || !orig || !new_ || !win || !delta || !out)
        return pm_fail(PM_EINVAL, "null argument");
    if (x_stride < n_in || out_stride < n_out)
        return pm_fail(PM_EINVAL, "a row stride is below its row's length");
    if (rows == 0 || n_out == 0) return PM_OK;
    ResampleInterpArgs a;
    a.x = x; a.lengths = lengths; a.orig = orig; a.new_ = new_;
    a.win = win; a.delta = delta; a.out = out;
    a.x_stride = x_stride; a.out_stride = out_stride;
    a.n_in = n_in; a.n_out = n_out;
    a.tiles = (int)(((long long)n_out + RI_TILE - 1) / RI_TILE);
    if ((long long)a.tiles * rows > PM_MAX_GRID)
        return pm_fail(PM_EINVAL, "too many workgroups (%d per row x %d rows)",
                       a.tiles, rows);
    hipLaunchKernelGGL(pm_resample_interp_kernel, dim3(a.tiles * rows),
                       dim3(RI_THREADS), 0, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// The LPC-feature stage of the C ABI (include/promonet_hip.h). Kernel:
// pm_lpc.h. Every argument is checked before the first HIP call, so the
// checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_lpc.h"

namespace {

// workgroups of LPC_THREADS a launch takes: 2^32 - 1 threads in all
const long long MAX_GRID = 0xffffffffll / LPC_THREADS;

}  // namespace

extern "C" int pm_harmonics_lpc(const float* audio, const int* lengths,
                                const float* window, const float* table,
                                float* features, float* coefficients, int rows,
                                long long stride, int samples, int frames,
                                int order, void* stream) {
    if (rows < 0 || samples < 0 || frames < 0)
        return pm_fail(PM_EINVAL, "negative size");
    if (order < 1 || order > LPC_MAX_ORDER)
        return pm_fail(PM_EINVAL, "order %d: the kernel takes orders 1 to %d",
                       order, LPC_MAX_ORDER);
    if (stride < samples)
        return pm_fail(PM_EINVAL, "the row stride is below the row's length");
    const long long total = (long long)rows * frames;
    if ((total + LPC_WAVES - 1) / LPC_WAVES > MAX_GRID)
        return pm_fail(PM_EINVAL, "too many frames");
    if (total == 0) return PM_OK;
    if (!audio || !window || !table || !features)
        return pm_fail(PM_EINVAL, "null argument");
    if (!pm_aligned16(window) || !pm_aligned16(table))
        return pm_fail(PM_EINVAL, "the window and the table must be 16-byte "
                       "aligned");
    LpcArgs a;
    a.x = audio; a.lengths = lengths; a.window = window; a.table = table;
    a.out = features; a.coefficients = coefficients; a.stride = stride;
    a.total = total; a.n = samples; a.T = frames; a.order = order;
    hipLaunchKernelGGL(hm_lpc_kernel,
                       dim3((unsigned)((total + LPC_WAVES - 1) / LPC_WAVES)),
                       dim3(LPC_THREADS), 0, (hipStream_t)stream, a);
    const hipError_t status = hipGetLastError();
    if (status != hipSuccess)
        return pm_fail(PM_EHIP, "hm_lpc_kernel launch failed: %s",
                       hipGetErrorString(status));
    return PM_OK;
}

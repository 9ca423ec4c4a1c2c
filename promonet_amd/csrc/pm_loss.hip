// The training-side losses of the C ABI (include/promonet_hip.h): the
// spectral-convergence loss in its three stages and the signal loss. Kernels:
// pm_loss.h, on the transform of pm_stockham.h: centred, so every plan is
// made with a margin of fft_size / 2. Every argument is checked before the
// first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_loss.h"

namespace {

// the gradient spectrum (only with_gradient) | the groups' partial sums
struct ScForwardLayout { float *gradient, *partials; size_t total; };
ScForwardLayout sc_forward_layout(int batch, const ScPlan& p,
                                  int with_gradient, void* base) {
    const size_t gradient = (size_t)batch * (p.M + 1) * p.frames * 2;
    PmCarve c(base);
    return {with_gradient ? c.take<float>(gradient) : nullptr,
            c.take<float>((size_t)batch * p.groups * 2), c.used};
}

}  // namespace

extern "C" size_t pm_sc_forward_workspace_bytes(int batch, int samples,
                                                int fft_size, int hop_size,
                                                int with_gradient) {
    ScPlan p;
    if (sc_make_plan(batch, samples, fft_size, hop_size, fft_size / 2, &p))
        return 0;
    return sc_forward_layout(batch, p, with_gradient, nullptr).total;
}

extern "C" size_t pm_sc_adjoint_workspace_bytes(int batch, int samples,
                                                int fft_size, int hop_size) {
    ScPlan p;
    if (sc_make_plan(batch, samples, fft_size, hop_size, fft_size / 2, &p))
        return 0;
    return pm_align256((size_t)batch * p.frames * p.N * sizeof(float));
}

extern "C" int pm_sc_stft(const float* x, const float* window,
                          const float* twiddle, const float* upstream,
                          float* s, float* gradient, int batch, int samples,
                          int fft_size, int hop_size, void* stream) {
    ScForwardArgs a;
    if (const char* why = sc_make_plan(batch, samples, fft_size, hop_size,
                                       fft_size / 2, &a.p))
        return pm_fail(PM_EINVAL, "pm_sc_stft: %s", why);
    if (!x || !window || !twiddle || (!s && !gradient))
        return pm_fail(PM_EINVAL, "null argument");
    a.x = x; a.y = nullptr; a.window = window; a.twiddle = twiddle;
    a.upstream = upstream; a.s = s; a.G = gradient; a.partials = nullptr;
    const size_t lds = 2 * (size_t)a.p.fpg * a.p.M * sizeof(float2);
    hipLaunchKernelGGL(sc_forward_kernel<false>, dim3(batch * a.p.groups),
                       dim3(SC_THREADS), lds, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_sc_forward(const float* x, const float* y,
                             const float* window, const float* twiddle,
                             float* sums, int batch, int samples,
                             int fft_size, int hop_size, int with_gradient,
                             void* workspace, size_t workspace_bytes,
                             void* stream) {
    ScForwardArgs a;
    if (const char* why = sc_make_plan(batch, samples, fft_size, hop_size,
                                       fft_size / 2, &a.p))
        return pm_fail(PM_EINVAL, "pm_sc_forward: %s", why);
    if (!x || !y || !window || !twiddle || !sums || !workspace)
        return pm_fail(PM_EINVAL, "null argument");
    const ScForwardLayout l =
        sc_forward_layout(batch, a.p, with_gradient, workspace);
    if (workspace_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    a.x = x; a.y = y; a.window = window; a.twiddle = twiddle;
    a.upstream = nullptr; a.s = nullptr;
    a.G = l.gradient;
    a.partials = l.partials;
    const size_t lds = 4 * (size_t)a.p.fpg * a.p.M * sizeof(float2);
    const int groups = batch * a.p.groups;
    hipLaunchKernelGGL(sc_forward_kernel<true>, dim3(groups),
                       dim3(SC_THREADS), lds, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sc_sums_kernel, dim3(1), dim3(SC_THREADS), 0,
                       (hipStream_t)stream, (const float*)a.partials,
                       (long long)groups, sums);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

hipError_t pm_sc_adjoint_launch(const ScPlan& p, int batch, const float* G,
                                const float* window, const float* twiddle,
                                const float* scale, float* grad_x,
                                int accumulate, float* frames, hipStream_t s) {
    ScAdjointArgs a;
    a.G = G; a.window = window; a.twiddle = twiddle; a.frames_out = frames;
    a.p = p;
    const size_t lds = 2 * (size_t)p.fpg * p.M * sizeof(float2);
    hipLaunchKernelGGL(sc_adjoint_frames_kernel, dim3(batch * p.groups),
                       dim3(SC_THREADS), lds, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    ScOverlapArgs o;
    o.frames_in = frames; o.scale = scale; o.grad_x = grad_x;
    o.N = p.N; o.pad = p.pad; o.hop = p.hop; o.frames = p.frames;
    o.T = p.T; o.accumulate = accumulate;
    o.total = (long long)batch * p.T;
    hipLaunchKernelGGL(sc_overlap_kernel,
                       dim3((o.total + SC_THREADS - 1) / SC_THREADS),
                       dim3(SC_THREADS), 0, s, o);
    return hipGetLastError();
}

extern "C" int pm_sc_adjoint(const float* gradient, const float* window,
                             const float* twiddle, const float* scale,
                             float* grad_x, int batch, int samples,
                             int fft_size, int hop_size, int accumulate,
                             void* workspace, size_t workspace_bytes,
                             void* stream) {
    ScPlan p;
    if (const char* why = sc_make_plan(batch, samples, fft_size, hop_size,
                                       fft_size / 2, &p))
        return pm_fail(PM_EINVAL, "pm_sc_adjoint: %s", why);
    if (!gradient || !window || !twiddle || !scale || !grad_x || !workspace)
        return pm_fail(PM_EINVAL, "null argument");
    if (workspace_bytes < pm_sc_adjoint_workspace_bytes(
            batch, samples, fft_size, hop_size))
        return pm_fail(PM_ENOMEM, "workspace too small");
    PM_HIP_TRY(pm_sc_adjoint_launch(p, batch, gradient, window, twiddle, scale,
                                    grad_x, accumulate, (float*)workspace,
                                    (hipStream_t)stream));
    return PM_OK;
}

extern "C" size_t pm_signal_loss_workspace_bytes(int rows) {
    if (rows < 1) return 0;
    return pm_align256((size_t)rows * 4 * sizeof(float));
}

namespace {
const char* check_signal(int rows, int samples) {
    if (rows < 1 || samples < 1) return "rows and samples must be at least 1";
    if (((long long)rows * samples + SC_THREADS - 1) / SC_THREADS > PM_MAX_GRID)
        return "too many samples for one launch";
    return nullptr;
}
}  // namespace

extern "C" int pm_signal_loss(const float* y_true, const float* y_pred,
                              float* out, int rows, int samples,
                              void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (const char* why = check_signal(rows, samples))
        return pm_fail(PM_EINVAL, "pm_signal_loss: %s", why);
    if (!y_true || !y_pred || !out || !workspace)
        return pm_fail(PM_EINVAL, "null argument");
    if (workspace_bytes < pm_signal_loss_workspace_bytes(rows))
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipLaunchKernelGGL(sc_signal_rows_kernel, dim3(rows), dim3(SC_THREADS), 0,
                       (hipStream_t)stream, y_true, y_pred, (float*)workspace,
                       samples);
    PM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sc_signal_mean_kernel, dim3(1), dim3(SC_THREADS), 0,
                       (hipStream_t)stream, (const float*)workspace, rows,
                       out);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_signal_loss_backward(const float* y_true,
                                       const float* y_pred,
                                       const float* grad_out, float* grad,
                                       int rows, int samples,
                                       const void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (const char* why = check_signal(rows, samples))
        return pm_fail(PM_EINVAL, "pm_signal_loss_backward: %s", why);
    if (!y_true || !y_pred || !grad_out || !grad || !workspace)
        return pm_fail(PM_EINVAL, "null argument");
    if (workspace_bytes < pm_signal_loss_workspace_bytes(rows))
        return pm_fail(PM_ENOMEM, "workspace too small");
    const long long total = (long long)rows * samples;
    hipLaunchKernelGGL(sc_signal_backward_kernel,
                       dim3((total + SC_THREADS - 1) / SC_THREADS),
                       dim3(SC_THREADS), 0, (hipStream_t)stream, y_true,
                       y_pred, (const float*)workspace, grad_out, grad, rows,
                       samples);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

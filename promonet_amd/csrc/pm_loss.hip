// The training-side losses of the C ABI (include/promonet_hip.h): the
// spectral-convergence loss in its three stages and the signal loss. Kernels:
// pm_loss.h. Every argument is checked before the first HIP call, so the
// checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_loss.h"

namespace {

const int MAX_SAMPLES = 1 << 30;

// The radix plan of a size and the split of a row's frames over workgroups:
// 5 first where N = 5 2^a, then 4s, then one 2 where a power of 4 does not
// finish. Returns NULL, or what is wrong with the sizes.
const char* make_plan(int batch, int samples, int fft_size, int hop_size,
                      ScPlan* p) {
    if (batch < 1) return "batch must be at least 1";
    if (fft_size < 64 || fft_size > 2560)
        return "fft_size must be between 64 and 2560";
    int rest = fft_size;
    if (rest % 5 == 0) rest /= 5;
    if (rest & (rest - 1)) return "fft_size must be 2^a or 5 * 2^a";
    if (hop_size < 1 || hop_size > fft_size)
        return "hop_size must be between 1 and fft_size";
    if (samples <= fft_size / 2)
        return "the row must be longer than fft_size / 2 (reflect padding)";
    if (samples > MAX_SAMPLES) return "the row must not exceed 2^30 samples";
    p->N = fft_size;
    p->M = fft_size / 2;
    p->hop = hop_size;
    p->T = samples;
    p->frames = 1 + samples / hop_size;
    p->fpg = SC_MAX_POINTS / p->M;
    if (p->fpg > p->frames) p->fpg = p->frames;
    p->groups = (p->frames + p->fpg - 1) / p->fpg;
    p->stages = 0;
    int m = p->M;
    if (m % 5 == 0) { p->radix[p->stages++] = 5; m /= 5; }
    while (m % 4 == 0) { p->radix[p->stages++] = 4; m /= 4; }
    if (m == 2) p->radix[p->stages++] = 2;
    if ((long long)batch * p->groups > PM_MAX_GRID ||
        ((long long)batch * samples + SC_THREADS - 1) / SC_THREADS >
            PM_MAX_GRID)
        return "too many frames or samples for one launch";
    return nullptr;
}

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
    if (make_plan(batch, samples, fft_size, hop_size, &p)) return 0;
    return sc_forward_layout(batch, p, with_gradient, nullptr).total;
}

extern "C" size_t pm_sc_adjoint_workspace_bytes(int batch, int samples,
                                                int fft_size, int hop_size) {
    ScPlan p;
    if (make_plan(batch, samples, fft_size, hop_size, &p)) return 0;
    return pm_align256((size_t)batch * p.frames * p.N * sizeof(float));
}

extern "C" int pm_sc_stft(const float* x, const float* window,
                          const float* twiddle, const float* upstream,
                          float* s, float* gradient, int batch, int samples,
                          int fft_size, int hop_size, void* stream) {
    ScForwardArgs a;
    if (const char* why = make_plan(batch, samples, fft_size, hop_size, &a.p))
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
    if (const char* why = make_plan(batch, samples, fft_size, hop_size, &a.p))
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

extern "C" int pm_sc_adjoint(const float* gradient, const float* window,
                             const float* twiddle, const float* scale,
                             float* grad_x, int batch, int samples,
                             int fft_size, int hop_size, int accumulate,
                             void* workspace, size_t workspace_bytes,
                             void* stream) {
    ScAdjointArgs a;
    if (const char* why = make_plan(batch, samples, fft_size, hop_size, &a.p))
        return pm_fail(PM_EINVAL, "pm_sc_adjoint: %s", why);
    if (!gradient || !window || !twiddle || !scale || !grad_x || !workspace)
        return pm_fail(PM_EINVAL, "null argument");
    if (workspace_bytes < pm_sc_adjoint_workspace_bytes(
            batch, samples, fft_size, hop_size))
        return pm_fail(PM_ENOMEM, "workspace too small");
    a.G = gradient; a.window = window; a.twiddle = twiddle;
    a.frames_out = (float*)workspace;
    const size_t lds = 2 * (size_t)a.p.fpg * a.p.M * sizeof(float2);
    hipLaunchKernelGGL(sc_adjoint_frames_kernel, dim3(batch * a.p.groups),
                       dim3(SC_THREADS), lds, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    ScOverlapArgs o;
    o.frames_in = (const float*)workspace; o.scale = scale; o.grad_x = grad_x;
    o.N = a.p.N; o.M = a.p.M; o.hop = a.p.hop; o.frames = a.p.frames;
    o.T = samples; o.accumulate = accumulate;
    o.total = (long long)batch * samples;
    hipLaunchKernelGGL(sc_overlap_kernel,
                       dim3((o.total + SC_THREADS - 1) / SC_THREADS),
                       dim3(SC_THREADS), 0, (hipStream_t)stream, o);
    PM_HIP_TRY(hipGetLastError());
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

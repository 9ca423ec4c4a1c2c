// The discriminator spectrograms of the C ABI (include/promonet_hip.h):
// pm_disc_spec_forward and pm_disc_spec_backward. Kernels: pm_disc_spec.h, on
// the transform of pm_stockham.h; the adjoint is pm_loss.hip's, through
// pm_sc_adjoint_launch. Every argument is checked before the first HIP call,
// so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_disc_spec.h"
#include "pm_host.h"

namespace {

long long elements_of(int batch, const ScPlan& p) {
    return (long long)batch * (p.M + 1) * p.frames;
}

// The plan of pm_stockham.h with the margin the caller names, then what only
// these entries check. Returns NULL, or what is wrong with the sizes.
const char* check_sizes(int mode, int batch, int samples, int fft_size,
                        int hop_size, int win_length, int pad, ScPlan* p) {
    if (const char* why =
            sc_make_plan(batch, samples, fft_size, hop_size, pad, p))
        return why;
    if (mode != PM_DISC_SPEC_R && mode != PM_DISC_SPEC_CMB &&
        mode != PM_DISC_SPEC_DB)
        return "mode must be PM_DISC_SPEC_R, _CMB or _DB";
    if (win_length < 1 || win_length > fft_size)
        return "win_length must be between 1 and fft_size";
    // (the launches over the elements)
    if ((elements_of(batch, *p) + SC_THREADS - 1) / SC_THREADS > PM_MAX_GRID)
        return "too many frames or samples for one launch";
    return nullptr;
}

// the workgroups of ds_floor_sums_kernel: a function of the sizes alone
int sum_groups(long long elements) {
    const long long want = (elements + 8 * SC_THREADS - 1) / (8 * SC_THREADS);
    return (int)(want < DS_SUM_GROUPS ? want : DS_SUM_GROUPS);
}

// forward (DB only): the workgroups' maxima
struct DsForwardLayout { float* partials; size_t total; };
DsForwardLayout forward_layout(int mode, int batch, const ScPlan& p,
                               void* base) {
    PmCarve c(base);
    return {mode == PM_DISC_SPEC_DB
                ? c.take<float>((size_t)batch * p.groups) : nullptr,
            c.used};
}

// backward: G | the time-domain frames | (DB) the partial sums | the share
struct DsBackwardLayout {
    float *gradient, *frames; double* partials; float* share; size_t total;
};
DsBackwardLayout backward_layout(int mode, int batch, const ScPlan& p,
                                 void* base) {
    const bool db = mode == PM_DISC_SPEC_DB;
    PmCarve c(base);
    return {c.take<float>((size_t)elements_of(batch, p) * 2),
            c.take<float>((size_t)batch * p.frames * p.N),
            db ? c.take<double>(2 * (size_t)sum_groups(elements_of(batch, p)))
               : nullptr,
            db ? c.take<float>(1) : nullptr, c.used};
}

template <bool GRAD>
void launch_transform(int mode, const DsArgs& a, int batch, hipStream_t s) {
    const size_t lds = 2 * (size_t)a.p.fpg * a.p.M * sizeof(float2);
    const dim3 grid(batch * a.p.groups), block(SC_THREADS);
    if (mode == PM_DISC_SPEC_R)
        hipLaunchKernelGGL((ds_transform_kernel<DS_R, GRAD>), grid, block,
                           lds, s, a);
    else if (mode == PM_DISC_SPEC_CMB)
        hipLaunchKernelGGL((ds_transform_kernel<DS_CMB, GRAD>), grid, block,
                           lds, s, a);
    else
        hipLaunchKernelGGL((ds_transform_kernel<DS_DB, GRAD>), grid, block,
                           lds, s, a);
}

}  // namespace

extern "C" size_t pm_disc_spec_workspace_bytes(int mode, int batch,
                                               int samples, int fft_size,
                                               int hop_size, int win_length,
                                               int pad, int backward) {
    ScPlan p;
    if (check_sizes(mode, batch, samples, fft_size, hop_size, win_length, pad,
                    &p))
        return 0;
    // (never 0 for sizes within the limits: 0 says that they are not)
    const size_t bytes = backward
        ? backward_layout(mode, batch, p, nullptr).total
        : forward_layout(mode, batch, p, nullptr).total;
    return bytes ? bytes : 256;
}

extern "C" int pm_disc_spec_forward(int mode, const float* x,
                                    const float* window, const float* twiddle,
                                    float* out, float* stats, int batch,
                                    int samples, int fft_size, int hop_size,
                                    int win_length, int pad, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    DsArgs a = {};
    if (const char* why = check_sizes(mode, batch, samples, fft_size,
                                      hop_size, win_length, pad, &a.p))
        return pm_fail(PM_EINVAL, "pm_disc_spec_forward: %s", why);
    const bool db = mode == PM_DISC_SPEC_DB;
    if (!x || !window || !twiddle || !out || (db && (!stats || !workspace)))
        return pm_fail(PM_EINVAL, "null argument");
    const DsForwardLayout l = forward_layout(mode, batch, a.p, workspace);
    if (db && workspace_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    a.x = x; a.window = window; a.twiddle = twiddle; a.out = out;
    a.partials = l.partials;
    launch_transform<false>(mode, a, batch, s);
    PM_HIP_TRY(hipGetLastError());
    if (db) {
        hipLaunchKernelGGL(ds_floor_kernel, dim3(1), dim3(SC_THREADS), 0, s,
                           (const float*)l.partials,
                           (long long)batch * a.p.groups, stats);
        PM_HIP_TRY(hipGetLastError());
        const long long total = elements_of(batch, a.p);
        hipLaunchKernelGGL(ds_apply_floor_kernel,
                           dim3((total + SC_THREADS - 1) / SC_THREADS),
                           dim3(SC_THREADS), 0, s, out, total,
                           (const float*)stats);
        PM_HIP_TRY(hipGetLastError());
    }
    return PM_OK;
}

extern "C" int pm_disc_spec_backward(int mode, const float* x,
                                     const float* window,
                                     const float* twiddle,
                                     const float* upstream,
                                     const float* saved_out,
                                     const float* stats, const float* scale,
                                     float* grad_x, int accumulate, int batch,
                                     int samples, int fft_size, int hop_size,
                                     int win_length, int pad, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    DsArgs a = {};
    if (const char* why = check_sizes(mode, batch, samples, fft_size,
                                      hop_size, win_length, pad, &a.p))
        return pm_fail(PM_EINVAL, "pm_disc_spec_backward: %s", why);
    const bool db = mode == PM_DISC_SPEC_DB;
    if (!x || !window || !twiddle || !upstream || !grad_x || !workspace ||
        (db && (!saved_out || !stats)))
        return pm_fail(PM_EINVAL, "null argument");
    const DsBackwardLayout l = backward_layout(mode, batch, a.p, workspace);
    if (workspace_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (db) {
        const long long total = elements_of(batch, a.p);
        const int groups = sum_groups(total);
        hipLaunchKernelGGL(ds_floor_sums_kernel, dim3(groups),
                           dim3(SC_THREADS), 0, s, saved_out, upstream, total,
                           stats, l.partials);
        PM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ds_share_kernel, dim3(1), dim3(SC_THREADS), 0, s,
                           (const double*)l.partials, groups, l.share);
        PM_HIP_TRY(hipGetLastError());
    }
    a.x = x; a.window = window; a.twiddle = twiddle; a.upstream = upstream;
    a.saved = saved_out; a.stats = stats; a.share = l.share;
    a.G = l.gradient;
    launch_transform<true>(mode, a, batch, s);
    PM_HIP_TRY(hipGetLastError());
    PM_HIP_TRY(pm_sc_adjoint_launch(a.p, batch, l.gradient, window, twiddle,
                                    scale, grad_x, accumulate, l.frames, s));
    return PM_OK;
}

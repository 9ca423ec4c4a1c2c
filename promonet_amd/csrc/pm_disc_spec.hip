// The discriminator spectrograms of the C ABI (include/promonet_hip.h):
// pm_disc_spec_forward and pm_disc_spec_backward. Kernels: pm_disc_spec.h, on
// the FFT core and the adjoint of pm_loss.h. Every argument is checked before
// the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"

// pm_loss.h also defines kernels that are no templates, and pm_loss.o has
// them already: here they are this file's own.
namespace {
#include "pm_disc_spec.h"

const int MAX_SAMPLES = 1 << 30;

// The plan of pm_loss.hip's make_plan with the margin as a parameter and the
// non-centred frame count. Returns NULL, or what is wrong with the sizes.
const char* make_plan(int mode, int batch, int samples, int fft_size,
                      int hop_size, int win_length, int pad, ScPlan* p) {
    if (mode != PM_DISC_SPEC_R && mode != PM_DISC_SPEC_CMB &&
        mode != PM_DISC_SPEC_DB)
        return "mode must be PM_DISC_SPEC_R, _CMB or _DB";
    if (batch < 1) return "batch must be at least 1";
    if (fft_size < 64 || fft_size > 2560)
        return "fft_size must be between 64 and 2560";
    int rest = fft_size;
    if (rest % 5 == 0) rest /= 5;
    if (rest & (rest - 1)) return "fft_size must be 2^a or 5 * 2^a";
    if (hop_size < 1 || hop_size > fft_size)
        return "hop_size must be between 1 and fft_size";
    if (win_length < 1 || win_length > fft_size)
        return "win_length must be between 1 and fft_size";
    if (pad < 0 || pad > fft_size) return "pad must be between 0 and fft_size";
    if (samples > MAX_SAMPLES) return "the row must not exceed 2^30 samples";
    if (samples <= pad)
        return "the row must be longer than pad (reflect padding)";
    if (samples + 2 * pad < fft_size)
        return "the padded row is shorter than one frame";
    p->N = fft_size;
    p->M = fft_size / 2;
    p->hop = hop_size;
    p->T = samples;
    p->frames = 1 + (samples + 2 * pad - fft_size) / hop_size;
    p->fpg = SC_MAX_POINTS / p->M;
    if (p->fpg > p->frames) p->fpg = p->frames;
    p->groups = (p->frames + p->fpg - 1) / p->fpg;
    p->stages = 0;
    int m = p->M;
    if (m % 5 == 0) { p->radix[p->stages++] = 5; m /= 5; }
    while (m % 4 == 0) { p->radix[p->stages++] = 4; m /= 4; }
    if (m == 2) p->radix[p->stages++] = 2;
    const long long elements = (long long)batch * (p->M + 1) * p->frames;
    if ((long long)batch * p->groups > PM_MAX_GRID ||
        ((long long)batch * samples + SC_THREADS - 1) / SC_THREADS >
            PM_MAX_GRID ||
        (elements + SC_THREADS - 1) / SC_THREADS > PM_MAX_GRID)
        return "too many frames or samples for one launch";
    return nullptr;
}

long long elements_of(int batch, const ScPlan& p) {
    return (long long)batch * (p.M + 1) * p.frames;
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
    if (make_plan(mode, batch, samples, fft_size, hop_size, win_length, pad,
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
    if (const char* why = make_plan(mode, batch, samples, fft_size, hop_size,
                                    win_length, pad, &a.p))
        return pm_fail(PM_EINVAL, "pm_disc_spec_forward: %s", why);
    const bool db = mode == PM_DISC_SPEC_DB;
    if (!x || !window || !twiddle || !out || (db && (!stats || !workspace)))
        return pm_fail(PM_EINVAL, "null argument");
    const DsForwardLayout l = forward_layout(mode, batch, a.p, workspace);
    if (db && workspace_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    a.x = x; a.window = window; a.twiddle = twiddle; a.out = out;
    a.partials = l.partials; a.pad = pad;
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
    if (const char* why = make_plan(mode, batch, samples, fft_size, hop_size,
                                    win_length, pad, &a.p))
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
    a.G = l.gradient; a.pad = pad;
    launch_transform<true>(mode, a, batch, s);
    PM_HIP_TRY(hipGetLastError());
    ScAdjointArgs f;
    f.G = l.gradient; f.window = window; f.twiddle = twiddle;
    f.frames_out = l.frames; f.p = a.p;
    const size_t lds = 2 * (size_t)a.p.fpg * a.p.M * sizeof(float2);
    hipLaunchKernelGGL(sc_adjoint_frames_kernel, dim3(batch * a.p.groups),
                       dim3(SC_THREADS), lds, s, f);
    PM_HIP_TRY(hipGetLastError());
    DsOverlapArgs o;
    o.frames_in = l.frames; o.scale = scale; o.grad_x = grad_x;
    o.N = a.p.N; o.pad = pad; o.hop = a.p.hop; o.frames = a.p.frames;
    o.T = samples; o.accumulate = accumulate;
    o.total = (long long)batch * samples;
    hipLaunchKernelGGL(ds_overlap_kernel,
                       dim3((o.total + SC_THREADS - 1) / SC_THREADS),
                       dim3(SC_THREADS), 0, s, o);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// The FARGAN discriminator's conv stacks of the C ABI (include/promonet_hip.h):
// pm_fdisc_conv_forward / _backward, pm_fdisc_weight_norm_forward / _backward
// and pm_fdisc_workspace_bytes. Kernels: pm_fdisc.h. Every argument is checked
// before the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_fdisc.h"
#include "pm_host.h"

namespace {

// Returns NULL, or what is wrong with the sizes of a layer.
const char* check_layer(int batch, int channels, int out_channels, int bins,
                        int frames, int dilation, int activation) {
    if (channels != 1 && channels != 16)
        return "channels must be 1 or 16";
    if (out_channels != 1 && out_channels != 16)
        return "out_channels must be 1 or 16";
    if (channels == 1 && out_channels == 1)
        return "no layer of the stack has one channel on both sides";
    if (dilation != 1 && dilation != 2 && dilation != 4 && dilation != 8 &&
        dilation != 16)
        return "dilation must be 1, 2, 4, 8 or 16";
    if (batch < 1 || bins < 1 || frames < 1)
        return "batch, bins and frames must be at least 1";
    if (activation != FD_NONE && activation != FD_RELU &&
        activation != FD_SIGMOID)
        return "activation must be PM_FDISC_NONE, _RELU or _SIGMOID";
    // (the kernels count pixels in 32 bits; the widest launch, four threads a
    // pixel, then has 2^25 workgroups)
    const long long pixels = (long long)batch * bins * frames;
    if (pixels > PM_MAX_GRID)
        return "too many pixels for one launch";
    return nullptr;
}

// The partials of gW and gb and the pixels of each
PmSplit split_of(long long pixels) {
    return pm_pixel_split(pixels, FD_GW_CHUNK, FD_GW_MAX_PARTS);
}

int partial_floats(int channels, int out_channels) {
    return out_channels * (channels + 2) * 9 + out_channels;
}

// backward: the partials
struct FdLayout { float* parts; size_t total; };
FdLayout backward_layout(long long pixels, int channels, int out_channels,
                         void* base) {
    PmCarve c(base);
    return {c.take<float>((size_t)split_of(pixels).parts *
                          partial_floats(channels, out_channels)),
            c.used};
}

const char* check_norm(int out_channels, int fan) {
    if (out_channels < 1 || out_channels > 65535)
        return "out_channels must be between 1 and 65535";
    if (fan < 1 || fan > (1 << 20))
        return "fan must be between 1 and 2^20";
    return nullptr;
}

}  // namespace

extern "C" size_t pm_fdisc_workspace_bytes(int batch, int channels,
                                           int out_channels, int bins,
                                           int frames) {
    if (check_layer(batch, channels, out_channels, bins, frames, 1, FD_NONE))
        return 0;
    return backward_layout((long long)batch * bins * frames, channels,
                           out_channels, nullptr).total;
}

extern "C" int pm_fdisc_conv_forward(const float* x, const float* weight,
                                     const float* bias, const float* table,
                                     float* y, int batch, int channels,
                                     int out_channels, int bins, int frames,
                                     int dilation, int activation,
                                     void* stream) {
    if (const char* why = check_layer(batch, channels, out_channels, bins,
                                      frames, dilation, activation))
        return pm_fail(PM_EINVAL, "pm_fdisc_conv_forward: %s", why);
    if (!x || !weight || !bias || !table || !y)
        return pm_fail(PM_EINVAL, "pm_fdisc_conv_forward: null argument");
    FdArgs a = {};
    a.x = x; a.w = weight; a.bias = bias; a.table = table; a.out = y;
    a.B = batch; a.F = bins; a.T = frames; a.d = dilation; a.act = activation;
    a.P = (long long)batch * bins * frames;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(FD_THREADS);
    const dim3 tiles(pm_groups(a.P, FD_CONV_PIXELS));
    if (out_channels == 1)
        hipLaunchKernelGGL(fd_conv_o1_kernel,
                           dim3(pm_groups(a.P, FD_THREADS)), block, 0, s, a);
    else if (channels == 16)
        hipLaunchKernelGGL((fd_conv16_kernel<16, false>), tiles, block, 0, s,
                           a);
    else
        hipLaunchKernelGGL((fd_conv16_kernel<1, false>), tiles, block, 0, s,
                           a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_fdisc_conv_backward(
    const float* upstream, const float* y, const float* x,
    const float* weight, const float* table, float* grad_x,
    float* grad_weight, float* grad_bias, int batch, int channels,
    int out_channels, int bins, int frames, int dilation, int activation,
    void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* why = check_layer(batch, channels, out_channels, bins,
                                      frames, dilation, activation))
        return pm_fail(PM_EINVAL, "pm_fdisc_conv_backward: %s", why);
    const long long pixels = (long long)batch * bins * frames;
    const FdLayout l =
        backward_layout(pixels, channels, out_channels, workspace);
    if (const int code = pm_check_backward(
            "pm_fdisc_conv_backward", upstream && y && x && weight && table,
            grad_weight, grad_bias, workspace, workspace_bytes, l.total))
        return code;
    FdArgs a = {};
    a.x = x; a.w = weight; a.table = table; a.g = upstream; a.y = y;
    a.B = batch; a.F = bins; a.T = frames; a.d = dilation; a.act = activation;
    a.P = pixels;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(FD_THREADS);
    if (grad_x) {
        a.out = grad_x;
        if (out_channels == 1)
            hipLaunchKernelGGL(fd_gx_o1_kernel,
                               dim3(pm_groups(a.P * 4, FD_THREADS)), block, 0,
                               s, a);
        else if (channels == 1)
            hipLaunchKernelGGL(fd_gx_c1_kernel,
                               dim3(pm_groups(a.P, FD_THREADS)), block, 0, s,
                               a);
        else
            hipLaunchKernelGGL((fd_conv16_kernel<16, true>),
                               dim3(pm_groups(a.P, FD_CONV_PIXELS)), block, 0,
                               s, a);
        PM_HIP_TRY(hipGetLastError());
    }
    if (grad_weight) {      // (and grad_bias: pm_check_backward)
        const PmSplit split = split_of(a.P);
        a.parts = l.parts;
        a.span = split.each;
        const dim3 grid(split.parts);
        if (out_channels == 1)
            hipLaunchKernelGGL((fd_gw_kernel<16, 1>), grid, block, 0, s, a);
        else if (channels == 16)
            hipLaunchKernelGGL((fd_gw_kernel<16, 16>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((fd_gw_kernel<1, 16>), grid, block, 0, s, a);
        PM_HIP_TRY(hipGetLastError());
        PM_HIP_TRY(dl_reduce(l.parts, split.parts,
                             partial_floats(channels, out_channels),
                             out_channels, grad_weight, grad_bias, s));
    }
    return PM_OK;
}

extern "C" int pm_fdisc_weight_norm_forward(const float* g, const float* v,
                                            float* w, int out_channels,
                                            int fan, void* stream) {
    if (const char* why = check_norm(out_channels, fan))
        return pm_fail(PM_EINVAL, "pm_fdisc_weight_norm_forward: %s", why);
    if (!g || !v || !w)
        return pm_fail(PM_EINVAL,
                       "pm_fdisc_weight_norm_forward: null argument");
    hipLaunchKernelGGL(fd_weight_norm_kernel, dim3(out_channels), dim3(64), 0,
                       (hipStream_t)stream, g, v, w, fan);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_fdisc_weight_norm_backward(const float* grad_w,
                                             const float* g, const float* v,
                                             float* grad_g, float* grad_v,
                                             int out_channels, int fan,
                                             void* stream) {
    if (const char* why = check_norm(out_channels, fan))
        return pm_fail(PM_EINVAL, "pm_fdisc_weight_norm_backward: %s", why);
    if (!grad_w || !g || !v || !grad_g || !grad_v)
        return pm_fail(PM_EINVAL,
                       "pm_fdisc_weight_norm_backward: null argument");
    hipLaunchKernelGGL(fd_weight_norm_backward_kernel, dim3(out_channels),
                       dim3(64), 0, (hipStream_t)stream, grad_w, g, v, grad_g,
                       grad_v, fan);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

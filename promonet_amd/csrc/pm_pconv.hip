// The conv stack of DiscriminatorP of the C ABI (include/promonet_hip.h):
// pm_pconv_forward / _backward, pm_pconv_fold_forward / _backward and their
// workspace queries. Kernels: pm_pconv.h. Every argument is checked before
// the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_pconv.h"

namespace {

struct Sizes {
    int B, C, O, H, P, K, S, Ho;
    int T, pad;                 // the first layer: samples, reflected samples
    long long in_pixels, out_pixels;
    bool first() const { return C == 1; }
    bool post() const { return O == 1; }
    long long partial_floats() const { return (long long)O * C * K + O; }
};

const char* check_period(int batch, int period) {
    if (batch < 1) return "batch must be at least 1";
    if (period < 1 || period > 64) return "period must be 1 ... 64";
    return nullptr;
}

// Returns NULL and fills `z`, or what is wrong with the sizes of a layer.
const char* check_layer(int batch, int channels, int out_channels, int height,
                        int period, int kernel, int stride, Sizes* z) {
    static const int forms[6][4] = {
        {1, 32, 5, 3}, {32, 128, 5, 3}, {128, 512, 5, 3}, {512, 1024, 5, 3},
        {1024, 1024, 5, 1}, {1024, 1, 3, 1}};
    bool form = false;
    for (const int* f : forms)
        form = form || (channels == f[0] && out_channels == f[1] &&
                        kernel == f[2] && stride == f[3]);
    if (!form)
        return "(channels, out_channels, kernel, stride) must be (1, 32, 5, "
               "3), (32, 128, 5, 3), (128, 512, 5, 3), (512, 1024, 5, 3), "
               "(1024, 1024, 5, 1) or (1024, 1, 3, 1)";
    if (const char* why = check_period(batch, period)) return why;
    if (height < 1) return "height must be at least 1";
    const int out_height = (height - 1) / stride + 1;
    const long long in_pixels = (long long)batch * height * period;
    const long long out_pixels = (long long)batch * out_height * period;
    // (the kernels count pixels in 32 bits)
    if (in_pixels > PM_MAX_GRID || out_pixels > PM_MAX_GRID)
        return "more than 2^31 - 1 input or output pixels";
    *z = {batch, channels, out_channels, height, period, kernel, stride,
          out_height, (int)(in_pixels / batch), 0, in_pixels, out_pixels};
    return nullptr;
}

// The first layer on the audio: the folded map is (B, (T + pad) / P, P)
const char* check_fold(int batch, int samples, int period, Sizes* z) {
    if (const char* why = check_period(batch, period)) return why;
    if (samples < 1) return "samples must be at least 1";
    const int pad = (period - samples % period) % period;
    if (samples <= pad)
        return "samples must be more than the reflected samples, (period - "
               "samples mod period) mod period";
    const int height = (int)(((long long)samples + pad) / period);
    const int out_height = (height - 1) / 3 + 1;
    const long long in_pixels = (long long)batch * height * period;
    const long long out_pixels = (long long)batch * out_height * period;
    if (in_pixels > PM_MAX_GRID || out_pixels > PM_MAX_GRID)
        return "more than 2^31 - 1 input or output pixels";
    *z = {batch, 1, 32, height, period, 5, 3, out_height, samples, pad,
          in_pixels, out_pixels};
    return nullptr;
}

// The partials of gW and gb and what each takes: K chunks of a tile (the
// general layers) or pixels (the edges). A function of the sizes alone.
PmChunkSplit split_of(const Sizes& z) {
    if (z.first() || z.post()) {
        const long long pixels = z.first() ? z.out_pixels : z.in_pixels;
        long long each = pm_ceil_div(pixels, PC_EDGE_MAX_PARTS);
        const int least = z.first() ? PC_FOLD_CHUNK : PC_POST_CHUNK;
        if (each < least) each = least;
        return {(int)pm_ceil_div(pixels, each), (int)each, 0};
    }
    const int tiles = (z.O / 64) * (z.C / (z.C < 64 ? 32 : 64));
    return pm_chunk_split(z.out_pixels, PC_GW_PIX, tiles, PC_GW_WORKGROUPS,
                          PC_GW_MIN_CHUNKS);
}

// backward: the partials
PmPartsLayout backward_layout(const Sizes& z, void* base) {
    return pm_parts_layout(base, (size_t)split_of(z).parts,
                           (size_t)z.partial_floats());
}

PcArgs args_of(const Sizes& z, float slope) {
    PcArgs a = {};
    a.B = z.B; a.H = z.H; a.Ho = z.Ho; a.P = z.P; a.C = z.C; a.O = z.O;
    a.T = z.T; a.pad = z.pad; a.slope = slope;
    a.pixels = z.out_pixels;
    return a;
}

template <bool GX, int S, int MT>
int launch_gemm(PcArgs a, const Sizes& z, hipStream_t s) {
    constexpr int SLOTS = (GX && S == 3) ? 2 : 5;
    const int lds = SLOTS * (MT + PC_NT) * PC_PITCH * (int)sizeof(float);
    long long ntiles;
    if (GX && S == 3) {
        ntiles = 0;
        for (int r = 0; r < 3; ++r) {
            const long long rows = z.H > r ? (z.H - 1 - r) / 3 + 1 : 0;
            a.classes[r] = (int)pm_ceil_div((long long)z.B * rows * z.P, PC_NT);
            ntiles += a.classes[r];
        }
    } else {
        ntiles = pm_ceil_div(GX ? z.in_pixels : z.out_pixels, PC_NT);
    }
    const long long grid = ntiles * ((GX ? z.C : z.O) / MT);
    return pm_launch_dynamic(pc_gemm_kernel<GX, S, MT>, (unsigned)grid,
                             PC_THREADS, lds, s, a);
}

template <int S, int CT>
int launch_gw(PcArgs a, const Sizes& z, const PmChunkSplit& split,
              hipStream_t s) {
    const int lds =
        PC_GW_PIX * (64 + 16 + 5 * (CT + 16)) * (int)sizeof(float);
    a.chunks = split.chunks; a.per = split.each;
    const int tiles = (z.O / 64) * (z.C / CT);
    return pm_launch_dynamic(pc_gw_kernel<S, CT>,
                             (unsigned)(tiles * split.parts), PC_THREADS, lds,
                             s, a);
}

int forward(const char* entry, const Sizes& z, const float* x,
            const float* weight, const float* bias, float* y, float slope,
            void* stream) {
    if (const char* why = pm_check_slope(slope))
        return pm_fail(PM_EINVAL, "%s: %s", entry, why);
    if (!x || !weight || !bias || !y)
        return pm_fail(PM_EINVAL, "%s: null argument", entry);
    PcArgs a = args_of(z, slope);
    a.x = x; a.w = weight; a.bias = bias; a.out = y;
    hipStream_t s = (hipStream_t)stream;
    if (z.first())
        hipLaunchKernelGGL(pc_fold_conv_kernel,
                           dim3(pm_groups(a.pixels * 8, PC_THREADS)),
                           dim3(PC_THREADS), 0, s, a);
    else if (z.post())
        hipLaunchKernelGGL(pc_post_conv_kernel,
                           dim3((unsigned)pm_ceil_div(a.pixels, 4)),
                           dim3(PC_THREADS), 0, s, a);
    else
        return z.S == 3 ? launch_gemm<false, 3, 64>(a, z, s)
                        : launch_gemm<false, 1, 64>(a, z, s);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

int backward(const char* entry, const Sizes& z, const float* upstream,
             const float* y, const float* x, const float* weight,
             float* grad_x, float* grad_weight, float* grad_bias, float slope,
             void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* why = pm_check_slope(slope))
        return pm_fail(PM_EINVAL, "%s: %s", entry, why);
    const PmPartsLayout l = backward_layout(z, workspace);
    if (const int code = pm_check_backward(
            entry, upstream && y && x && weight, grad_weight, grad_bias,
            workspace, workspace_bytes, l.total))
        return code;
    PcArgs a = args_of(z, slope);
    a.x = x; a.w = weight; a.g = upstream; a.y = y;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(PC_THREADS);
    if (grad_x) {
        a.out = grad_x;
        if (z.first()) {
            const long long samples = (long long)z.B * z.T;
            hipLaunchKernelGGL(pc_fold_gx_kernel,
                               dim3(pm_groups(samples, PC_THREADS)), block, 0,
                               s, a);
            PM_HIP_TRY(hipGetLastError());
        } else if (z.post()) {
            hipLaunchKernelGGL(pc_post_gx_kernel,
                               dim3(pm_groups(a.pixels * 256, PC_THREADS)),
                               block, 0, s, a);
            PM_HIP_TRY(hipGetLastError());
        } else {
            const int code =
                z.S == 1 ? launch_gemm<true, 1, 64>(a, z, s)
                : z.C == 32 ? launch_gemm<true, 3, 32>(a, z, s)
                            : launch_gemm<true, 3, 64>(a, z, s);
            if (code != PM_OK) return code;
        }
    }
    if (grad_weight) {      // (and grad_bias: pm_check_backward)
        a.parts = l.parts;
        const PmChunkSplit split = split_of(z);
        if (z.first() || z.post()) {
            a.span = split.each;
            if (z.first())
                hipLaunchKernelGGL(pc_fold_gw_kernel, dim3(split.parts), block,
                                   0, s, a);
            else
                hipLaunchKernelGGL(pc_post_gw_kernel, dim3(split.parts), block,
                                   0, s, a);
            PM_HIP_TRY(hipGetLastError());
        } else {
            const int code =
                z.S == 1 ? launch_gw<1, 64>(a, z, split, s)
                : z.C == 32 ? launch_gw<3, 32>(a, z, split, s)
                            : launch_gw<3, 64>(a, z, split, s);
            if (code != PM_OK) return code;
        }
        PM_HIP_TRY(dl_reduce(l.parts, split.parts, z.partial_floats(), z.O,
                             grad_weight, grad_bias, s));
    }
    return PM_OK;
}

}  // namespace

extern "C" size_t pm_pconv_workspace_bytes(int batch, int channels,
                                           int out_channels, int height,
                                           int period, int kernel,
                                           int stride) {
    Sizes z;
    if (check_layer(batch, channels, out_channels, height, period, kernel,
                    stride, &z))
        return 0;
    return backward_layout(z, nullptr).total;
}

extern "C" int pm_pconv_forward(const float* x, const float* weight,
                                const float* bias, float* y, int batch,
                                int channels, int out_channels, int height,
                                int period, int kernel, int stride,
                                float slope, void* stream) {
    Sizes z;
    if (const char* why = check_layer(batch, channels, out_channels, height,
                                      period, kernel, stride, &z))
        return pm_fail(PM_EINVAL, "pm_pconv_forward: %s", why);
    return forward("pm_pconv_forward", z, x, weight, bias, y, slope, stream);
}

extern "C" int pm_pconv_backward(
    const float* upstream, const float* y, const float* x,
    const float* weight, float* grad_x, float* grad_weight, float* grad_bias,
    int batch, int channels, int out_channels, int height, int period,
    int kernel, int stride, float slope, void* workspace,
    size_t workspace_bytes, void* stream) {
    Sizes z;
    if (const char* why = check_layer(batch, channels, out_channels, height,
                                      period, kernel, stride, &z))
        return pm_fail(PM_EINVAL, "pm_pconv_backward: %s", why);
    return backward("pm_pconv_backward", z, upstream, y, x, weight, grad_x,
                    grad_weight, grad_bias, slope, workspace, workspace_bytes,
                    stream);
}

extern "C" size_t pm_pconv_fold_workspace_bytes(int batch, int samples,
                                                int period) {
    Sizes z;
    if (check_fold(batch, samples, period, &z)) return 0;
    return backward_layout(z, nullptr).total;
}

extern "C" int pm_pconv_fold_forward(const float* audio, const float* weight,
                                     const float* bias, float* y, int batch,
                                     int samples, int period, float slope,
                                     void* stream) {
    Sizes z;
    if (const char* why = check_fold(batch, samples, period, &z))
        return pm_fail(PM_EINVAL, "pm_pconv_fold_forward: %s", why);
    return forward("pm_pconv_fold_forward", z, audio, weight, bias, y, slope,
                   stream);
}

extern "C" int pm_pconv_fold_backward(
    const float* upstream, const float* y, const float* audio,
    const float* weight, float* grad_audio, float* grad_weight,
    float* grad_bias, int batch, int samples, int period, float slope,
    void* workspace, size_t workspace_bytes, void* stream) {
    Sizes z;
    if (const char* why = check_fold(batch, samples, period, &z))
        return pm_fail(PM_EINVAL, "pm_pconv_fold_backward: %s", why);
    return backward("pm_pconv_fold_backward", z, upstream, y, audio, weight,
                    grad_audio, grad_weight, grad_bias, slope, workspace,
                    workspace_bytes, stream);
}

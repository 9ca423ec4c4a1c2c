// One conv of the generator's MRF Block of the C ABI (include/promonet_hip.h):
// pm_gconv_forward / _backward and their workspace query. Kernels:
// pm_gconv.h. Every argument is checked before the first HIP call, so the
// checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_gconv.h"
#include "pm_host.h"

namespace {

struct Sizes {
    int B, C, T, K, D;
    long long pixels;
    long long partial_floats() const { return (long long)C * C * K + C; }
    int gw_rows() const { return C < 64 ? 32 : 64; }    // OT of gc_gw_kernel
};

// Returns NULL and fills `z`, or what is wrong with the sizes.
const char* check_layer(int batch, int channels, int frames, int kernel,
                        int dilation, Sizes* z) {
    if ((channels != 32 && channels != 64 && channels != 128 &&
         channels != 256) ||
        (kernel != 3 && kernel != 7 && kernel != 11) ||
        (dilation != 1 && dilation != 3 && dilation != 5))
        return "channels must be 32, 64, 128 or 256, kernel 3, 7 or 11 and "
               "dilation 1, 3 or 5";
    static_assert(GC_MAX_DILATION == 5, "the dilations of check_layer");
    if (batch < 1) return "batch must be at least 1";
    if (frames < 1) return "frames must be at least 1";
    const long long pixels = (long long)batch * frames;
    // (the kernels count pixels in 32 bits)
    if (pixels > PM_MAX_GRID) return "more than 2^31 - 1 pixels";
    *z = {batch, channels, frames, kernel, dilation, pixels};
    return nullptr;
}

// The partials of gW and gb and the K chunks each takes. A function of the
// sizes alone.
PmChunkSplit split_of(const Sizes& z) {
    const int tiles = (z.C / z.gw_rows()) * (z.C / GC_GW_CT);
    return pm_chunk_split(z.pixels, GC_GW_PIX, tiles, GC_GW_WORKGROUPS,
                          GC_GW_MIN_CHUNKS);
}

// backward: the partials
PmPartsLayout backward_layout(const Sizes& z, void* base) {
    return pm_parts_layout(base, (size_t)split_of(z).parts,
                           (size_t)z.partial_floats());
}

GcArgs args_of(const Sizes& z, float slope) {
    GcArgs a = {};
    a.T = z.T; a.C = z.C; a.d = z.D; a.slope = slope; a.pixels = z.pixels;
    return a;
}

template <bool GX, int K, int MT>
int launch_gemm(const GcArgs& a, hipStream_t s) {
    const int lds = gc_gemm_lds<K, MT>() * (int)sizeof(float);
    // (at most 2^25 pixel tiles x 4 row tiles)
    const long long grid = pm_ceil_div(a.pixels, GC_NT) * (a.C / MT);
    return pm_launch_dynamic(gc_gemm_kernel<GX, K, MT>, (unsigned)grid,
                             GC_THREADS, lds, s, a);
}

template <bool GX>
int launch_gemm_of(const GcArgs& a, const Sizes& z, hipStream_t s) {
    if (z.C == 32)
        return z.K == 3 ? launch_gemm<GX, 3, 32>(a, s)
            : z.K == 7 ? launch_gemm<GX, 7, 32>(a, s)
                       : launch_gemm<GX, 11, 32>(a, s);
    return z.K == 3 ? launch_gemm<GX, 3, 64>(a, s)
        : z.K == 7 ? launch_gemm<GX, 7, 64>(a, s)
                   : launch_gemm<GX, 11, 64>(a, s);
}

template <int K, int OT>
int launch_gw(GcArgs a, const PmChunkSplit& split, hipStream_t s) {
    const int lds = gc_gw_lds<K, OT>() * (int)sizeof(float);
    a.chunks = split.chunks; a.per = split.each;
    const int tiles = (a.C / OT) * (a.C / GC_GW_CT);
    return pm_launch_dynamic(gc_gw_kernel<K, OT>,
                             (unsigned)(tiles * split.parts), GC_THREADS, lds,
                             s, a);
}

int launch_gw_of(const GcArgs& a, const Sizes& z, const PmChunkSplit& split,
                 hipStream_t s) {
    if (z.C == 32)
        return z.K == 3 ? launch_gw<3, 32>(a, split, s)
            : z.K == 7 ? launch_gw<7, 32>(a, split, s)
                       : launch_gw<11, 32>(a, split, s);
    return z.K == 3 ? launch_gw<3, 64>(a, split, s)
        : z.K == 7 ? launch_gw<7, 64>(a, split, s)
                   : launch_gw<11, 64>(a, split, s);
}

}  // namespace

extern "C" size_t pm_gconv_workspace_bytes(int batch, int channels, int frames,
                                           int kernel, int dilation) {
    Sizes z;
    if (check_layer(batch, channels, frames, kernel, dilation, &z)) return 0;
    return backward_layout(z, nullptr).total;
}

extern "C" int pm_gconv_forward(const float* x, const float* weight,
                                const float* bias, const float* residual,
                                float* y, int batch, int channels, int frames,
                                int kernel, int dilation, float slope,
                                void* stream) {
    Sizes z;
    if (const char* why =
            check_layer(batch, channels, frames, kernel, dilation, &z))
        return pm_fail(PM_EINVAL, "pm_gconv_forward: %s", why);
    if (const char* why = pm_check_slope(slope))
        return pm_fail(PM_EINVAL, "pm_gconv_forward: %s", why);
    if (!x || !weight || !bias || !y)
        return pm_fail(PM_EINVAL, "pm_gconv_forward: null argument");
    GcArgs a = args_of(z, slope);
    a.x = x; a.w = weight; a.bias = bias; a.residual = residual; a.out = y;
    return launch_gemm_of<false>(a, z, (hipStream_t)stream);
}

extern "C" int pm_gconv_backward(
    const float* upstream, const float* x, const float* weight, float* grad_x,
    float* grad_weight, float* grad_bias, int batch, int channels, int frames,
    int kernel, int dilation, float slope, void* workspace,
    size_t workspace_bytes, void* stream) {
    Sizes z;
    if (const char* why =
            check_layer(batch, channels, frames, kernel, dilation, &z))
        return pm_fail(PM_EINVAL, "pm_gconv_backward: %s", why);
    if (const char* why = pm_check_slope(slope))
        return pm_fail(PM_EINVAL, "pm_gconv_backward: %s", why);
    const PmPartsLayout l = backward_layout(z, workspace);
    if (const int code = pm_check_backward(
            "pm_gconv_backward", upstream && x && weight, grad_weight,
            grad_bias, workspace, workspace_bytes, l.total))
        return code;
    GcArgs a = args_of(z, slope);
    a.x = x; a.w = weight; a.g = upstream;
    hipStream_t s = (hipStream_t)stream;
    if (grad_x) {
        a.out = grad_x;
        if (const int code = launch_gemm_of<true>(a, z, s)) return code;
    }
    if (grad_weight) {      // (and grad_bias: pm_check_backward)
        a.parts = l.parts;
        const PmChunkSplit split = split_of(z);
        if (const int code = launch_gw_of(a, z, split, s)) return code;
        PM_HIP_TRY(dl_reduce(l.parts, split.parts, z.partial_floats(), z.C,
                             grad_weight, grad_bias, s));
    }
    return PM_OK;
}

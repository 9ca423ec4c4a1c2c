// The conv stacks of DiscriminatorCMB and DiscriminatorR of the C ABI
// (include/promonet_hip.h): pm_dconv_forward / _backward and
// pm_dconv_workspace_bytes. Kernels: pm_dconv.h. Every argument is checked
// before the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_dconv.h"
#include "pm_host.h"

namespace {

struct Sizes {
    int B, C, O, H, W, KW, S, Wo;
    long long in_pixels, out_pixels;
    bool wide() const { return C == 32 && O == 32; }
    int partial_floats() const { return O * C * 3 * KW + O; }
};

// Returns NULL and fills `z`, or what is wrong with the sizes of a layer.
const char* check_layer(int batch, int channels, int out_channels, int height,
                        int width, int kernel_width, int stride, Sizes* z) {
    const bool form =
        (channels == 1 && out_channels == 32 && kernel_width == 9 &&
         stride == 1) ||
        (channels == 32 && out_channels == 32 && kernel_width == 9 &&
         stride == 2) ||
        (channels == 32 && out_channels == 32 && kernel_width == 3 &&
         stride == 1) ||
        (channels == 32 && out_channels == 1 && kernel_width == 3 &&
         stride == 1);
    if (!form)
        return "(channels, out_channels, kernel_width, stride) must be "
               "(1, 32, 9, 1), (32, 32, 9, 2), (32, 32, 3, 1) or (32, 1, 3, 1)";
    if (batch < 1 || height < 1 || width < 1)
        return "batch, height and width must be at least 1";
    const int out_width = (width - 1) / stride + 1;
    const long long in_pixels = (long long)batch * height * width;
    const long long out_pixels = (long long)batch * height * out_width;
    // (the kernels count pixels in 32 bits; the widest launch, eight threads
    // a pixel, then has 2^26 workgroups)
    if (in_pixels > PM_MAX_GRID || out_pixels > PM_MAX_GRID)
        return "more than 2^31 - 1 input or output pixels";
    *z = {batch, channels, out_channels, height, width, kernel_width, stride,
          out_width, in_pixels, out_pixels};
    return nullptr;
}

// The tiles of the 32 -> 32 kernels over a map `columns` wide
struct Tiles { int tiles, tiles_h, tiles_w; };
Tiles tiles_of(const Sizes& z, int columns, int tile_columns) {
    Tiles t;
    t.tiles_h = (int)pm_ceil_div(z.H, DC_ROWS);
    t.tiles_w = (int)pm_ceil_div(columns, tile_columns);
    t.tiles = z.B * t.tiles_h * t.tiles_w;
    return t;
}

// The partials of gW and gb, one a workgroup, and what each takes: tiles (32
// -> 32) or pixels, a multiple of 16 (the edges). A function of the sizes
// alone.
PmSplit split_of(const Sizes& z) {
    if (z.wide()) {
        const int tiles = tiles_of(z, z.Wo, DC_COLS).tiles;
        int want = (int)pm_ceil_div(tiles, DC_GW_MIN_TILES);
        if (want > DC_GW_MAX_PARTS) want = DC_GW_MAX_PARTS;
        const int each = (int)pm_ceil_div(tiles, want);
        return {(int)pm_ceil_div(tiles, each), each};
    }
    return pm_pixel_split(z.out_pixels, DC_EDGE_CHUNK, DC_EDGE_MAX_PARTS);
}

// backward: the partials
PmPartsLayout backward_layout(const Sizes& z, void* base) {
    return pm_parts_layout(base, (size_t)split_of(z).parts,
                           (size_t)z.partial_floats());
}

unsigned walked(int tiles) {
    const int cus = pm_device_cus() > 0 ? pm_device_cus() : 256;
    return (unsigned)(tiles < cus ? tiles : cus);
}

DcArgs args_of(const Sizes& z, float slope) {
    DcArgs a = {};
    a.B = z.B; a.H = z.H; a.W = z.W; a.Wo = z.Wo; a.slope = slope;
    a.P = z.out_pixels;
    return a;
}

void set_tiles(DcArgs& a, const Tiles& t) {
    a.tiles = t.tiles; a.tiles_h = t.tiles_h; a.tiles_w = t.tiles_w;
}

template <int KW, int S>
int launch_conv32(DcArgs a, const Sizes& z, hipStream_t s) {
    typedef Dc32<KW, S> D;
    const int lds =
        (D::WEIGHTS + (DC_ROWS + 2) * D::NP * DC_PITCH) * (int)sizeof(float);
    set_tiles(a, tiles_of(z, z.Wo, DC_COLS));
    return pm_launch_dynamic(dc_conv32_kernel<KW, S>, walked(a.tiles),
                             DC_THREADS, lds, s, a);
}

template <int KW, int S>
int launch_gx32(DcArgs a, const Sizes& z, hipStream_t s) {
    typedef Dc32<KW, S> D;
    const int lds =
        (D::WEIGHTS + (DC_ROWS + 2) * D::NG * DC_PITCH) * (int)sizeof(float);
    set_tiles(a, tiles_of(z, z.W, D::GX_COLS));
    return pm_launch_dynamic(dc_gx32_kernel<KW, S>, walked(a.tiles),
                             DC_THREADS, lds, s, a);
}

template <int KW, int S>
int launch_gw32(DcArgs a, const Sizes& z, hipStream_t s) {
    typedef Dc32<KW, S> D;
    const int lds = ((DC_ROWS + 2) * D::NP + DC_ROWS * DC_COLS) * DC_PITCH *
        (int)sizeof(float);
    set_tiles(a, tiles_of(z, z.Wo, DC_COLS));
    const PmSplit split = split_of(z);
    a.per = split.each;
    return pm_launch_dynamic(dc_gw32_kernel<KW, S>, (unsigned)split.parts,
                             DC_THREADS, lds, s, a);
}

}  // namespace

extern "C" size_t pm_dconv_workspace_bytes(int batch, int channels,
                                           int out_channels, int height,
                                           int width, int kernel_width,
                                           int stride) {
    Sizes z;
    if (check_layer(batch, channels, out_channels, height, width, kernel_width,
                    stride, &z))
        return 0;
    return backward_layout(z, nullptr).total;
}

extern "C" int pm_dconv_forward(const float* x, const float* weight,
                                const float* bias, float* y, int batch,
                                int channels, int out_channels, int height,
                                int width, int kernel_width, int stride,
                                float slope, void* stream) {
    Sizes z;
    if (const char* why = check_layer(batch, channels, out_channels, height,
                                      width, kernel_width, stride, &z))
        return pm_fail(PM_EINVAL, "pm_dconv_forward: %s", why);
    if (const char* why = pm_check_slope(slope))
        return pm_fail(PM_EINVAL, "pm_dconv_forward: %s", why);
    if (!x || !weight || !bias || !y)
        return pm_fail(PM_EINVAL, "pm_dconv_forward: null argument");
    DcArgs a = args_of(z, slope);
    a.x = x; a.w = weight; a.bias = bias; a.out = y;
    hipStream_t s = (hipStream_t)stream;
    if (z.wide())
        return z.KW == 9 ? launch_conv32<9, 2>(a, z, s)
                         : launch_conv32<3, 1>(a, z, s);
    if (z.O == 1)
        hipLaunchKernelGGL(dc_conv_o1_kernel,
                           dim3(pm_groups(a.P, DC_THREADS)), dim3(DC_THREADS),
                           0, s, a);
    else
        hipLaunchKernelGGL(dc_conv_c1_kernel,
                           dim3(pm_groups(a.P * 8, DC_THREADS)),
                           dim3(DC_THREADS), 0, s, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_dconv_backward(
    const float* upstream, const float* y, const float* x,
    const float* weight, float* grad_x, float* grad_weight, float* grad_bias,
    int batch, int channels, int out_channels, int height, int width,
    int kernel_width, int stride, float slope, void* workspace,
    size_t workspace_bytes, void* stream) {
    Sizes z;
    if (const char* why = check_layer(batch, channels, out_channels, height,
                                      width, kernel_width, stride, &z))
        return pm_fail(PM_EINVAL, "pm_dconv_backward: %s", why);
    if (const char* why = pm_check_slope(slope))
        return pm_fail(PM_EINVAL, "pm_dconv_backward: %s", why);
    const PmPartsLayout l = backward_layout(z, workspace);
    if (const int code = pm_check_backward(
            "pm_dconv_backward", upstream && y && x && weight, grad_weight,
            grad_bias, workspace, workspace_bytes, l.total))
        return code;
    DcArgs a = args_of(z, slope);
    a.x = x; a.w = weight; a.g = upstream; a.y = y;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(DC_THREADS);
    if (grad_x) {
        a.out = grad_x;
        if (z.wide()) {
            const int code = z.KW == 9 ? launch_gx32<9, 2>(a, z, s)
                                       : launch_gx32<3, 1>(a, z, s);
            if (code != PM_OK) return code;
        } else {
            if (z.O == 1)
                hipLaunchKernelGGL(dc_gx_o1_kernel,
                                   dim3(pm_groups(a.P * 8, DC_THREADS)), block,
                                   0, s, a);
            else
                hipLaunchKernelGGL(dc_gx_c1_kernel,
                                   dim3(pm_groups(a.P, DC_THREADS)), block, 0,
                                   s, a);
            PM_HIP_TRY(hipGetLastError());
        }
    }
    if (grad_weight) {      // (and grad_bias: pm_check_backward)
        a.parts = l.parts;
        const PmSplit split = split_of(z);
        if (z.wide()) {
            const int code = z.KW == 9 ? launch_gw32<9, 2>(a, z, s)
                                       : launch_gw32<3, 1>(a, z, s);
            if (code != PM_OK) return code;
        } else {
            a.span = split.each;
            if (z.O == 1)
                hipLaunchKernelGGL(dc_gw_edge_kernel<1>, dim3(split.parts),
                                   block, 0, s, a);
            else
                hipLaunchKernelGGL(dc_gw_edge_kernel<32>, dim3(split.parts),
                                   block, 0, s, a);
            PM_HIP_TRY(hipGetLastError());
        }
        PM_HIP_TRY(dl_reduce(l.parts, split.parts, z.partial_floats(), z.O,
                             grad_weight, grad_bias, s));
    }
    return PM_OK;
}

// The FARGAN discriminator's conv stacks of the C ABI (include/promonet_hip.h):
// pm_fdisc_conv_forward / _backward, pm_fdisc_layer_forward / _backward,
// pm_fdisc_weight_norm_forward / _backward and the two workspace queries.
// Kernels: pm_fdisc.h, pm_fdisc_strided.h. Every argument is checked
// before the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_fdisc.h"
#include "pm_fdisc_strided.h"
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
PmPartsLayout backward_layout(long long pixels, int channels, int out_channels,
                              void* base) {
    return pm_parts_layout(base, (size_t)split_of(pixels).parts,
                           (size_t)partial_floats(channels, out_channels));
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
    const PmPartsLayout l =
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

// ---------------------------------------------------------------------------
// pm_fdisc_layer_*: every layer of the six stacks (kernels: pm_fdisc_strided.h
// and, for the three forms of pm_fdisc_conv_* at stride 1, the entries above)
// ---------------------------------------------------------------------------
namespace {

enum FsKind { FS_REFUSED, FS_NARROW, FS_FIRST, FS_LAST, FS_GEMM };

// What computes (channels, out_channels, stride): the table of the reference
FsKind kind_of(int channels, int out_channels, int stride) {
    const int C = channels, O = out_channels;
    if (stride == 1 &&
        ((C == 1 && O == 16) || (C == 16 && O == 16) || (C == 16 && O == 1)))
        return FS_NARROW;
    if (stride == 2 && C == 1 && O == 16) return FS_FIRST;
    const bool wide = C == 16 || C == 32 || C == 64 || C == 128;
    if (wide && O == 2 * C) return FS_GEMM;
    if (stride == 1 && wide && C >= 32 && O == C) return FS_GEMM;
    if (stride == 1 && O == 1 && (C == 32 || C == 64 || C == 128 || C == 256))
        return FS_LAST;
    return FS_REFUSED;
}

int out_bins(int bins, int stride) { return (bins - 1) / stride + 1; }

const char* check_strided(int batch, int channels, int out_channels, int bins,
                          int frames, int stride, int activation) {
    if (stride != 1 && stride != 2) return "stride must be 1 or 2";
    if (kind_of(channels, out_channels, stride) == FS_REFUSED)
        return "no layer of the six stacks has these channels at this stride";
    if (batch < 1 || bins < 1 || frames < 1)
        return "batch, bins and frames must be at least 1";
    if (activation != FD_NONE && activation != FD_RELU &&
        activation != FD_SIGMOID)
        return "activation must be PM_FDISC_NONE, _RELU or _SIGMOID";
    // (the kernels count the pixels of either map in 32 bits)
    if ((long long)batch * bins * frames > PM_MAX_GRID)
        return "too many pixels for one launch";
    return nullptr;
}

// gW of the general layers: the tiles, and the split of their K chunks
int gemm_tiles(int channels, int out_channels) {
    const int cb = channels == 16 ? 1 : 2;
    return channels / (16 * cb) * (int)pm_ceil_div(out_channels, 64 / cb);
}
PmChunkSplit gemm_split(long long out_pixels, int tiles) {
    return pm_chunk_split(out_pixels, FS_GW_PIX, tiles, FS_GW_WORKGROUPS,
                          FS_GW_MIN_CHUNKS);
}

// the partials of the layer's gW | gb (the edge kernels: one a workgroup of
// the pixels they walk)
int strided_parts(FsKind kind, long long in_pixels, long long out_pixels,
                  int channels, int out_channels) {
    if (kind == FS_GEMM)
        return gemm_split(out_pixels,
                          gemm_tiles(channels, out_channels)).parts;
    return pm_pixel_split(kind == FS_FIRST ? out_pixels : in_pixels,
                          FS_EDGE_CHUNK, FS_EDGE_MAX_PARTS).parts;
}

PmPartsLayout strided_layout(FsKind kind, long long in_pixels,
                             long long out_pixels, int channels,
                             int out_channels, void* base) {
    return pm_parts_layout(
        base,
        (size_t)strided_parts(kind, in_pixels, out_pixels, channels,
                              out_channels),
        (size_t)partial_floats(channels, out_channels));
}

// `tiles` pixel tiles of every row tile: MT = 16, 32 or 64 rows
template <bool GX, int S>
void launch_gemm(const FsArgs& a, unsigned tiles, hipStream_t s) {
    const int M = GX ? a.C : a.O;
    const dim3 block(FD_THREADS);
    if constexpr (GX) {     // (16 rows: gx of the 16 -> 32 layers alone)
        if (M == 16) {
            hipLaunchKernelGGL((fs_gemm_kernel<true, S, 16>), dim3(tiles),
                               block, 0, s, a);
            return;
        }
    }
    if (M == 32)
        hipLaunchKernelGGL((fs_gemm_kernel<GX, S, 32>), dim3(tiles), block, 0,
                           s, a);
    else
        hipLaunchKernelGGL((fs_gemm_kernel<GX, S, 64>),
                           dim3(tiles * (M / 64)), block, 0, s, a);
}

template <int S>
void launch_gw(const FsArgs& a, int tiles, const PmChunkSplit& split,
               hipStream_t s) {
    const dim3 grid((unsigned)tiles * split.parts), block(FD_THREADS);
    if (a.C == 16)
        hipLaunchKernelGGL((fs_gw_kernel<S, 1>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((fs_gw_kernel<S, 2>), grid, block, 0, s, a);
}

}  // namespace

extern "C" size_t pm_fdisc_layer_workspace_bytes(int batch, int channels,
                                                 int out_channels, int bins,
                                                 int frames, int stride) {
    if (check_strided(batch, channels, out_channels, bins, frames, stride,
                      FD_NONE))
        return 0;
    const FsKind kind = kind_of(channels, out_channels, stride);
    if (kind == FS_NARROW)
        return pm_fdisc_workspace_bytes(batch, channels, out_channels, bins,
                                        frames);
    return strided_layout(
        kind, (long long)batch * bins * frames,
        (long long)batch * out_bins(bins, stride) * frames, channels,
        out_channels, nullptr).total;
}

extern "C" int pm_fdisc_layer_forward(const float* x, const float* weight,
                                      const float* bias, const float* table,
                                      float* y, int batch, int channels,
                                      int out_channels, int bins, int frames,
                                      int stride, int activation,
                                      void* stream) {
    if (const char* why = check_strided(batch, channels, out_channels, bins,
                                        frames, stride, activation))
        return pm_fail(PM_EINVAL, "pm_fdisc_layer_forward: %s", why);
    if (!x || !weight || !bias || !table || !y)
        return pm_fail(PM_EINVAL, "pm_fdisc_layer_forward: null argument");
    const FsKind kind = kind_of(channels, out_channels, stride);
    if (kind == FS_NARROW)
        return pm_fdisc_conv_forward(x, weight, bias, table, y, batch,
                                     channels, out_channels, bins, frames, 1,
                                     activation, stream);
    FsArgs a = {};
    a.x = x; a.w = weight; a.bias = bias; a.table = table; a.out = y;
    a.B = batch; a.F = bins; a.Fo = out_bins(bins, stride); a.T = frames;
    a.C = channels; a.O = out_channels; a.s = stride; a.act = activation;
    const long long out_pixels = (long long)batch * a.Fo * frames;
    a.pixels = out_pixels;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(FD_THREADS);
    if (kind == FS_FIRST) {
        hipLaunchKernelGGL(fs_first_conv_kernel,
                           dim3(pm_groups(out_pixels * 4, FD_THREADS)), block,
                           0, s, a);
    } else if (kind == FS_LAST) {
        hipLaunchKernelGGL(fs_last_conv_kernel,
                           dim3(pm_groups(out_pixels * 8, FD_THREADS)), block,
                           0, s, a);
    } else {
        const unsigned tiles = pm_groups(out_pixels, FS_NT);
        if (stride == 1) launch_gemm<false, 1>(a, tiles, s);
        else launch_gemm<false, 2>(a, tiles, s);
    }
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_fdisc_layer_backward(
    const float* upstream, const float* y, const float* x,
    const float* weight, const float* table, float* grad_x,
    float* grad_weight, float* grad_bias, int batch, int channels,
    int out_channels, int bins, int frames, int stride, int activation,
    void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* why = check_strided(batch, channels, out_channels, bins,
                                        frames, stride, activation))
        return pm_fail(PM_EINVAL, "pm_fdisc_layer_backward: %s", why);
    const FsKind kind = kind_of(channels, out_channels, stride);
    const long long in_pixels = (long long)batch * bins * frames;
    const long long out_pixels =
        (long long)batch * out_bins(bins, stride) * frames;
    const size_t needed = kind == FS_NARROW
        ? pm_fdisc_workspace_bytes(batch, channels, out_channels, bins, frames)
        : strided_layout(kind, in_pixels, out_pixels, channels, out_channels,
                         nullptr).total;
    if (const int code = pm_check_backward(
            "pm_fdisc_layer_backward", upstream && y && x && weight && table,
            grad_weight, grad_bias, workspace, workspace_bytes, needed))
        return code;
    if (kind == FS_NARROW)
        return pm_fdisc_conv_backward(upstream, y, x, weight, table, grad_x,
                                      grad_weight, grad_bias, batch, channels,
                                      out_channels, bins, frames, 1,
                                      activation, workspace, workspace_bytes,
                                      stream);
    const PmPartsLayout l = strided_layout(kind, in_pixels, out_pixels, channels,
                                      out_channels, workspace);
    FsArgs a = {};
    a.x = x; a.w = weight; a.table = table; a.g = upstream; a.y = y;
    a.B = batch; a.F = bins; a.Fo = out_bins(bins, stride); a.T = frames;
    a.C = channels; a.O = out_channels; a.s = stride; a.act = activation;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(FD_THREADS);
    if (grad_x) {
        a.out = grad_x;
        a.pixels = in_pixels;
        if (kind == FS_FIRST) {
            hipLaunchKernelGGL(fs_first_gx_kernel,
                               dim3(pm_groups(in_pixels, FD_THREADS)), block,
                               0, s, a);
        } else if (kind == FS_LAST) {
            hipLaunchKernelGGL(
                fs_last_gx_kernel,
                dim3(pm_groups(in_pixels * (channels / 4), FD_THREADS)), block,
                0, s, a);
        } else if (stride == 1) {
            launch_gemm<true, 1>(a, pm_groups(in_pixels, FS_NT), s);
        } else {
            // the even input rows, then the odd ones
            a.classes[0] = (int)pm_groups(
                (long long)batch * ((bins + 1) / 2) * frames, FS_NT);
            a.classes[1] = (int)pm_groups(
                (long long)batch * (bins / 2) * frames, FS_NT);
            launch_gemm<true, 2>(
                a, (unsigned)a.classes[0] + (unsigned)a.classes[1], s);
        }
        PM_HIP_TRY(hipGetLastError());
    }
    if (grad_weight) {      // (and grad_bias: pm_check_backward)
        a.parts = l.parts;
        int parts;
        if (kind == FS_GEMM) {
            const int tiles = gemm_tiles(channels, out_channels);
            const PmChunkSplit split = gemm_split(out_pixels, tiles);
            a.pixels = out_pixels;
            a.chunks = split.chunks;
            a.per = split.each;
            parts = split.parts;
            if (stride == 1) launch_gw<1>(a, tiles, split, s);
            else launch_gw<2>(a, tiles, split, s);
        } else {
            a.pixels = kind == FS_FIRST ? out_pixels : in_pixels;
            const PmSplit split =
                pm_pixel_split(a.pixels, FS_EDGE_CHUNK, FS_EDGE_MAX_PARTS);
            a.span = split.each;
            parts = split.parts;
            if (kind == FS_FIRST)
                hipLaunchKernelGGL(fs_first_gw_kernel, dim3(parts), block, 0,
                                   s, a);
            else
                hipLaunchKernelGGL(fs_last_gw_kernel, dim3(parts), block, 0, s,
                                   a);
        }
        PM_HIP_TRY(hipGetLastError());
        PM_HIP_TRY(dl_reduce(l.parts, parts,
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

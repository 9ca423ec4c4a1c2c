// The conv stacks of the FARGAN discriminator, DiscriminatorMagFree
// (promonet/model/discriminator.py:320-389), forward and backward: a layer is
//   y = act(conv3x3(cat(x, sin, cos)) + bias),
// stride 1, dilation (d, 1), "same" padding (d, 1), with the two channels of
// FrequencyPositionalEmbedding (:381-389), sin and cos of 2 pi f / F, never
// materialised: they come from a (F, 2) table and are zero outside the map as
// the conv's own padding makes them.
//
// MEMORY ORDER. A map of 16 channels is channels_last: logical (B, 16, F, T),
// in memory (B, F, T, 16), so the 16 channels of a pixel are one 64-byte run.
// A map of one channel (the decibel spectrogram, the logits) is (B, F, T)
// either way. A pixel is p = (b F + f) T + t; the kernels tile the flattened
// pixels, so T = 9 and T = 257 fill waves alike, and a tap is the pixel
// p + (kf - 1) d T + (kt - 1) where its (f, t) lies inside the map.
//
// ARITHMETIC. fp32 throughout. The layers with 16 output channels run on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums): the 16 output
// channels are the 16 rows of one tile, 16 pixels its columns, and K walks the
// taps: per tap 4 steps of 4 input channels, then 5 steps that hold the 18
// (tap, sin / cos) pairs. The first layer (1 + 2 channels) is 9 steps of
// (x, sin, cos, 0). The layer with one output channel and the input gradients
// of the two edge layers are plain VALU kernels.
//
// BACKWARD. gz = upstream * act'(y) from the saved output alone (relu: y > 0,
// sigmoid: y (1 - y)) is formed where it is read. gx is the forward conv on gz
// with the flipped, transposed weight of the first C channels. gW (O, C + 2,
// 3, 3) and gb (O) are sums over all pixels: a workgroup accumulates its
// pixels in MFMA tiles (K = pixels), its four waves are added in order, the
// partial goes to the workspace, and dl_reduce_kernel (pm_dlayer.h) adds the
// partials in a fixed order in double. Their count and the pixels of each are
// a function of the sizes alone: no float atomics, the same bits on every run.
//
// NON-FINITE VALUES. This header promises torch's semantics on inf and NaN
// (DESIGN section 27): relu(NaN) is NaN and passes its upstream gradient, a
// non-finite input or upstream reaches exactly the outputs that a tap links it
// to, and no other element changes a bit. The object is built with
// -fhonor-nans (Makefile), or the test of a NaN folds.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_dlayer.h"
#include "pm_nonfinite.h"

#define FD_NONE 0
#define FD_RELU 1
#define FD_SIGMOID 2

#define FD_THREADS 256          // every kernel but the weight norm's
#define FD_WAVE_TILES 8         // 16-pixel tiles a wave of the conv kernel
#define FD_CONV_PIXELS (FD_THREADS / 64 * FD_WAVE_TILES * 16)   // a workgroup
#define FD_GW_CHUNK 2048        // fewest pixels of a gW workgroup (but the last)
#define FD_GW_MAX_PARTS 768     // most partials of gW and gb: three a CU
static_assert(FD_THREADS == DL_THREADS, "the workgroup of pm_dlayer.h");

struct FdArgs {
    const float* x;         // (B, F, T, C)
    const float* w;         // (O, C + 2, 3, 3)
    const float* bias;      // (O)
    const float* table;     // (F, 2): sin, cos of 2 pi f / F
    const float* g;         // backward: upstream (B, F, T, O)
    const float* y;         // backward: the saved output (B, F, T, O)
    float* out;             // forward: y; backward: gx (B, F, T, C)
    float* parts;           // backward: (parts, O (C + 2) 9 + O)
    int B, F, T, d, act;
    long long P;            // B F T
    int span;               // backward: pixels of a gW workgroup, 16 n
};

// The taps of a pixel of the flattened map (DlPixel, h the frequency and w the
// frame): the frequency of tap `tap` (kf = tap / 3, kt = tap % 3), or -1
// outside, which the embedding table needs. SIGN = -1 mirrors the tap (the
// input gradient reads gz at p - offset). DlPixel::inside's test with the row
// kept, in the order that leaves fd_conv16_kernel's machine code as it was.
__device__ __forceinline__ int fd_tap_f(const DlPixel& px, int tap, int d,
                                        int F, int T, int sign = 1) {
    const int ff = px.h + sign * (tap / 3 - 1) * d;
    const int tt = px.w + sign * (tap % 3 - 1);
    return (ff >= 0 && ff < F && tt >= 0 && tt < T) ? ff : -1;
}
__device__ __forceinline__ long long fd_tap_offset(int tap, int d, int T) {
    return dl_offset((long long)(tap / 3 - 1) * d, tap % 3 - 1, T);
}

// (torch.relu keeps a NaN)
__device__ __forceinline__ float fd_activate(float v, int act) {
    if (act == FD_RELU) return pm_max_nan(v, 0.f);
    if (act == FD_SIGMOID) return 1.f / (1.f + expf(-v));
    return v;
}
// upstream * act'(y); relu as torch's threshold_backward: 0 where y <= 0, the
// upstream elsewhere, so a NaN output passes it, and a choice, not a product:
// an infinite upstream behind a closed gate gives 0
__device__ __forceinline__ float fd_gate(float g, float y, int act) {
    if (act == FD_RELU) return y <= 0.f ? 0.f : g;
    if (act == FD_SIGMOID) return g * (y * (1.f - y));
    return g;
}

// ---------------------------------------------------------------------------
// 16 output rows on the MFMA. D[i][pixel], lane l: column l & 15, A and B
// element k = l >> 4 of a step; D rows 4 (l >> 4) + r in register r.
//   GRAD = false: i = output channel, y = act(conv + bias), C = 16 or 1;
//   GRAD = true (C = 16): i = input channel, gx = conv of gz with W[o][i] at
//   the mirrored tap; no embedding, no bias, no activation.
// A step of a tap contracts the input channels {4 k + e}: lane k reads the
// float4 of channels 4 k .. 4 k + 3 of the tap's pixel once and step e takes
// its element e, so the weight of (row i, step e, lane k) is channel 4 k + e.
// ---------------------------------------------------------------------------
template <int C, bool GRAD>
__global__ __launch_bounds__(FD_THREADS) void fd_conv16_kernel(FdArgs a) {
    constexpr int CIN = C + 2, FAN = CIN * 9;
    const int lane = threadIdx.x & 63, col = lane & 15, k = lane >> 4;
    // the weights of this lane, in registers for every tile
    float wx[C == 16 ? 36 : 9];
    float we[C == 16 ? 5 : 1];
    if (C == 16) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                wx[tap * 4 + e] = GRAD
                    ? a.w[(4 * k + e) * FAN + col * 9 + (8 - tap)]
                    : a.w[col * FAN + (4 * k + e) * 9 + tap];
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int tap = 2 * s + (k >> 1);
            we[s] = (!GRAD && tap < 9)
                ? a.w[col * FAN + (16 + (k & 1)) * 9 + tap] : 0.f;
        }
    } else {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            wx[tap] = k < 3 ? a.w[col * FAN + k * 9 + tap] : 0.f;
        we[0] = 0.f;
    }
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    if (!GRAD)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[r] = a.bias[4 * k + r];

    const long long first = ((long long)blockIdx.x * (FD_THREADS / 64) +
                             (threadIdx.x >> 6)) * (FD_WAVE_TILES * 16);
    for (int tile = 0; tile < FD_WAVE_TILES; ++tile) {
        const long long p = first + tile * 16 + col;
        if (first + tile * 16 >= a.P) break;        // (the whole wave leaves)
        const bool live = p < a.P;
        const DlPixel px(live ? p : 0, a.F, a.T);
        dl_f4 acc = {0.f, 0.f, 0.f, 0.f};
        if (C == 16) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ff = fd_tap_f(px, tap, a.d, a.F, a.T);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live && ff >= 0) {
                    const long long at =
                        (p + fd_tap_offset(tap, a.d, a.T)) * 16 + 4 * k;
                    if (GRAD) {
                        const float4 g = *(const float4*)(a.g + at);
                        const float4 y = *(const float4*)(a.y + at);
                        v = make_float4(fd_gate(g.x, y.x, a.act),
                                        fd_gate(g.y, y.y, a.act),
                                        fd_gate(g.z, y.z, a.act),
                                        fd_gate(g.w, y.w, a.act));
                    } else {
                        v = *(const float4*)(a.x + at);
                    }
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    wx[tap * 4 + 0], v.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    wx[tap * 4 + 1], v.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    wx[tap * 4 + 2], v.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    wx[tap * 4 + 3], v.w, acc, 0, 0, 0);
            }
            if (!GRAD) {
                // the 18 (tap, sin / cos) pairs: lane k holds pair 4 s + k
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    const int tap = 2 * s + (k >> 1);
                    const int ff =
                        tap < 9 ? fd_tap_f(px, tap, a.d, a.F, a.T) : -1;
                    const float v = (live && ff >= 0)
                        ? a.table[2 * ff + (k & 1)] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        we[s], v, acc, 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ff = fd_tap_f(px, tap, a.d, a.F, a.T);
                float v = 0.f;
                if (live && ff >= 0 && k < 3)
                    v = k == 0 ? a.x[p + fd_tap_offset(tap, a.d, a.T)]
                               : a.table[2 * ff + (k - 1)];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    wx[tap], v, acc, 0, 0, 0);
            }
        }
        if (live) {
            float4 o;
            if (GRAD)
                o = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else
                o = make_float4(fd_activate(acc[0] + bias[0], a.act),
                                fd_activate(acc[1] + bias[1], a.act),
                                fd_activate(acc[2] + bias[2], a.act),
                                fd_activate(acc[3] + bias[3], a.act));
            *(float4*)(a.out + p * 16 + 4 * k) = o;
        }
    }
}

// ---------------------------------------------------------------------------
// The edge layers on the VALU. Weights are read at uniform addresses.
// ---------------------------------------------------------------------------
// 16 -> 1, forward: one pixel a thread
__global__ __launch_bounds__(FD_THREADS) void fd_conv_o1_kernel(FdArgs a) {
    const long long p = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const DlPixel px(p, a.F, a.T);
    float acc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int ff = fd_tap_f(px, tap, a.d, a.F, a.T);
        if (ff < 0) continue;
        const float4* v =
            (const float4*)(a.x + (p + fd_tap_offset(tap, a.d, a.T)) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 u = v[q];
            acc = fmaf(a.w[(4 * q + 0) * 9 + tap], u.x, acc);
            acc = fmaf(a.w[(4 * q + 1) * 9 + tap], u.y, acc);
            acc = fmaf(a.w[(4 * q + 2) * 9 + tap], u.z, acc);
            acc = fmaf(a.w[(4 * q + 3) * 9 + tap], u.w, acc);
        }
        acc = fmaf(a.w[16 * 9 + tap], a.table[2 * ff], acc);
        acc = fmaf(a.w[17 * 9 + tap], a.table[2 * ff + 1], acc);
    }
    a.out[p] = fd_activate(acc + a.bias[0], a.act);
}

// 16 -> 1, input gradient: four input channels of one pixel a thread
__global__ __launch_bounds__(FD_THREADS) void fd_gx_o1_kernel(FdArgs a) {
    const long long i = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= a.P * 4) return;
    const long long p = i >> 2;
    const int q = (int)(i & 3);
    const DlPixel px(p, a.F, a.T);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (fd_tap_f(px, tap, a.d, a.F, a.T, -1) < 0) continue;
        const long long at = p - fd_tap_offset(tap, a.d, a.T);
        const float gz = fd_gate(a.g[at], a.y[at], a.act);
        acc.x = fmaf(a.w[(4 * q + 0) * 9 + tap], gz, acc.x);
        acc.y = fmaf(a.w[(4 * q + 1) * 9 + tap], gz, acc.y);
        acc.z = fmaf(a.w[(4 * q + 2) * 9 + tap], gz, acc.z);
        acc.w = fmaf(a.w[(4 * q + 3) * 9 + tap], gz, acc.w);
    }
    *(float4*)(a.out + p * 16 + 4 * q) = acc;
}

// 1 -> 16, input gradient: one pixel a thread
__global__ __launch_bounds__(FD_THREADS) void fd_gx_c1_kernel(FdArgs a) {
    const long long p = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const DlPixel px(p, a.F, a.T);
    float acc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (fd_tap_f(px, tap, a.d, a.F, a.T, -1) < 0) continue;
        const long long at = (p - fd_tap_offset(tap, a.d, a.T)) * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 g = *(const float4*)(a.g + at + 4 * q);
            const float4 y = *(const float4*)(a.y + at + 4 * q);
            acc = fmaf(a.w[(4 * q + 0) * 27 + tap], fd_gate(g.x, y.x, a.act), acc);
            acc = fmaf(a.w[(4 * q + 1) * 27 + tap], fd_gate(g.y, y.y, a.act), acc);
            acc = fmaf(a.w[(4 * q + 2) * 27 + tap], fd_gate(g.z, y.z, a.act), acc);
            acc = fmaf(a.w[(4 * q + 3) * 27 + tap], fd_gate(g.w, y.w, a.act), acc);
        }
    }
    a.out[p] = acc;
}

// ---------------------------------------------------------------------------
// gW and gb: MFMA tiles with K = pixels, four pixels a step, lane l: pixel
// (l >> 4) of the step, row / column l & 15.
//   O = 16 (C = 16 or 1): A[o][pixel] = gz, B[pixel][column]: the columns are
//     the features of the pixel, NM tiles of 16:
//       C = 16: 9 tiles of the 16 channels at a tap, then the 18 (tap, sin /
//               cos) pairs and, column 162, one (gb);
//       C = 1:  (tap, x / sin / cos) = 27 columns, then one;
//   O = 1 (C = 16): a tile a tap, A[c][pixel] = x where the mirrored tap is
//     inside the map, B[pixel][any column] = gz at that tap; a tenth tile has
//     the rows sin, cos, one (gb at the centre tap) and the taps as columns.
// fd_slot: where tile m, row i, column j goes in (O, C + 2, 3, 3) | (O), or -1.
// ---------------------------------------------------------------------------
template <int C, int O> struct FdGw {
    static constexpr int FAN = (C + 2) * 9;
    static constexpr int N = O * FAN + O;           // floats of a partial
    static constexpr int NM = O == 1 ? 10 : (C == 16 ? 11 : 2);
    __device__ static __forceinline__ int slot(int m, int i, int j) {
        if (O == 1) {
            if (m < 9) return j == 0 ? i * 9 + m : -1;
            if (i < 2) return j < 9 ? (16 + i) * 9 + j : -1;
            return (i == 2 && j == 4) ? FAN : -1;
        }
        const int idx = 16 * m + j;
        if (C == 16) {
            if (m < 9) return i * FAN + j * 9 + m;
            const int e = idx - 144;
            if (e < 18) return i * FAN + (16 + (e & 1)) * 9 + (e >> 1);
            return e == 18 ? O * FAN + i : -1;
        }
        if (idx < 27) return i * FAN + (idx % 3) * 9 + idx / 3;
        return idx == 27 ? O * FAN + i : -1;
    }
};

template <int C, int O>
__global__ __launch_bounds__(FD_THREADS) void fd_gw_kernel(FdArgs a) {
    typedef FdGw<C, O> G;
    constexpr int NM = G::NM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, k = lane >> 4;
    dl_f4 acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) acc[m] = dl_f4{0.f, 0.f, 0.f, 0.f};

    const auto [begin, steps] = dl_gw_span(a.P, a.span, wave);
    DlPixel px(begin + k < a.P ? begin + k : 0, a.F, a.T);
    for (int step = 0; step < steps; ++step, px.advance(4, a.F, a.T)) {
        const long long p = begin + step * 4 + k;
        const bool live = p < a.P;
        if (O == 16) {
            float gz = 0.f;
            if (live) gz = fd_gate(a.g[p * 16 + j], a.y[p * 16 + j], a.act);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                float v = 0.f;
                if (C == 16 && m < 9) {
                    if (live && fd_tap_f(px, m, a.d, a.F, a.T) >= 0)
                        v = a.x[(p + fd_tap_offset(m, a.d, a.T)) * 16 + j];
                } else {
                    // (tap, which) of this column: which 0 = x (C = 1),
                    // 1 = sin, 2 = cos; 3 = one; -1 = nothing
                    int tap = 0, which = -1;
                    if (C == 16) {
                        const int e = 16 * m + j - 144;
                        tap = e >> 1;
                        which = e < 18 ? 1 + (e & 1) : (e == 18 ? 3 : -1);
                    } else {
                        const int idx = 16 * m + j;
                        tap = idx / 3;
                        which = idx < 27 ? idx % 3 : (idx == 27 ? 3 : -1);
                    }
                    if (live && which == 3) {
                        v = 1.f;
                    } else if (live && which >= 0) {
                        const int ff = fd_tap_f(px, tap, a.d, a.F, a.T);
                        if (ff >= 0)
                            v = which == 0
                                ? a.x[p + fd_tap_offset(tap, a.d, a.T)]
                                : a.table[2 * ff + which - 1];
                    }
                }
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    gz, v, acc[m], 0, 0, 0);
            }
        } else {
            float gz = 0.f;
            if (live && j < 9 && fd_tap_f(px, j, a.d, a.F, a.T, -1) >= 0) {
                const long long at = p - fd_tap_offset(j, a.d, a.T);
                gz = fd_gate(a.g[at], a.y[at], a.act);
            }
            const float xv = live ? a.x[p * 16 + j] : 0.f;
            float ev = 0.f;
            if (live && j < 3)
                ev = j == 2 ? 1.f : a.table[2 * px.h + j];
            // One tile a tap, every column the tap's gz: where the tap leaves
            // the map x is left out, not multiplied by the 0 that gz is
            // there, or an infinite x on a border pixel would make that
            // product a NaN. The same products in the same order as one
            // tile with the taps as its columns, to the bit.
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const bool in =
                    live && fd_tap_f(px, tap, a.d, a.F, a.T, -1) >= 0;
                acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    in ? xv : 0.f, __shfl(gz, (k << 4) | tap, 64), acc[tap],
                    0, 0, 0);
            }
            acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                ev, gz, acc[9], 0, 0, 0);
        }
    }
    dl_gw_store<G>(acc, a.parts);
}

// ---------------------------------------------------------------------------
// Weight norm over (C + 2, 3, 3) per output channel (torch._weight_norm, dim
// 0): w = g v / |v|. One wave an output channel, fixed-order sums.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float fd_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(64) void fd_weight_norm_kernel(
    const float* __restrict__ g, const float* __restrict__ v,
    float* __restrict__ w, int fan) {
    const float* row = v + (long long)blockIdx.x * fan;
    float sq = 0.f;
    for (int i = threadIdx.x; i < fan; i += 64) sq = fmaf(row[i], row[i], sq);
    const float scale = g[blockIdx.x] / sqrtf(fd_wave_sum(sq));
    for (int i = threadIdx.x; i < fan; i += 64)
        w[(long long)blockIdx.x * fan + i] = row[i] * scale;
}

// g_g = <gw, v> / |v|;  g_v = (g / |v|) (gw - v <gw, v> / |v|^2)
__global__ __launch_bounds__(64) void fd_weight_norm_backward_kernel(
    const float* __restrict__ gw, const float* __restrict__ g,
    const float* __restrict__ v, float* __restrict__ grad_g,
    float* __restrict__ grad_v, int fan) {
    const float* row = v + (long long)blockIdx.x * fan;
    const float* up = gw + (long long)blockIdx.x * fan;
    float sq = 0.f, dot = 0.f;
    for (int i = threadIdx.x; i < fan; i += 64) {
        sq = fmaf(row[i], row[i], sq);
        dot = fmaf(up[i], row[i], dot);
    }
    sq = fd_wave_sum(sq);
    dot = fd_wave_sum(dot);
    const float norm = sqrtf(sq);
    if (threadIdx.x == 0) grad_g[blockIdx.x] = dot / norm;
    const float scale = g[blockIdx.x] / norm, back = dot / sq;
    for (int i = threadIdx.x; i < fan; i += 64)
        grad_v[(long long)blockIdx.x * fan + i] =
            scale * (up[i] - row[i] * back);
}

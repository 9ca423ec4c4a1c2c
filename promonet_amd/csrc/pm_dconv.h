// The conv stacks of the complex multi-band and the multi-resolution
// discriminators, DiscriminatorCMB.band_convs / conv_post
// (promonet/model/discriminator.py:146-208) and DiscriminatorR.convs /
// conv_post (:96-127), forward and backward: a layer is
//   y = leaky(conv2d(x, W, b, stride (1, s), padding (1, (kw - 1) / 2)), slope)
// with x (B, C, H, W), W (O, C, 3, kw) and (C, O, kw, s) one of
//   (1, 32, 9, 1)   (32, 32, 9, 2)   (32, 32, 3, 1)   (32, 1, 3, 1).
// The output is Wo = (W - 1) / s + 1 wide and H high. slope 1 is no activation.
//
// MEMORY ORDER. A map of 32 channels is channels_last: logical (B, 32, H, W),
// in memory (B, H, W, 32), the 32 channels of a pixel one 128-byte run. A map
// of one channel is (B, H, W).
//
// ARITHMETIC. fp32 throughout; the 32 -> 32 layers run on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums).
//
// THE 32 -> 32 KERNELS work on tiles of DC_ROWS output rows x DC_COLS output
// columns of one batch row, one row a wave, walked by a grid of at most one
// workgroup a CU:
//   forward  the whole weight (3 kw 32 32 floats, 110 592 bytes at kw 9) is
//            staged in LDS once a workgroup, in the order the A operand is
//            read (one 16-byte read gives a lane four K steps). The DC_ROWS +
//            2 input rows x 15 s + kw input pixels that the tile reads are
//            staged in LDS too, DC_PITCH floats a pixel; the next tile's are
//            in flight in registers under the MFMAs of this one. The 32
//            output channels are two 16-row tiles that share every B operand,
//            16 MFMAs a tap from six 16-byte LDS reads; the K = 864 sum of a
//            tile is split by kernel row and channel half into six chains of
//            36 MFMAs, added pairwise at the end: twelve independent
//            accumulators a wave, and a third of the rounding error of one
//            chain of 216.
//   gx       gather form on gz = g (y > 0 ? 1 : slope), formed where it is
//            staged. At s = 2 a tile is DC_ROWS rows x 32 input pixels: the 16
//            even and the 16 odd pixels are two MFMA column sets that read the
//            SAME staged gz pixels (output column j + 2 - t for tap 2 t +
//            parity), the even ones under taps 0 2 4 6 8 and the odd ones
//            under 1 3 5 7, nothing scattered. The transposed weight is staged
//            whole and the sums are split as in the forward.
//   gW, gb   K = pixels. A = gz (o rows), B = x at the tap (c columns); wave
//            (m, n) of a workgroup owns the o tile m and the c tile n of all
//            3 kw taps: 27 accumulators, each MFMA of a step independent of
//            the other 26; gb is one more accumulator against a column of
//            ones. A workgroup walks `per` consecutive tiles and writes one
//            partial (O C 3 kw + O floats) to the workspace; dl_reduce_kernel
//            adds the partials in ascending order in double. Their count and
//            the tiles of each are a function of the sizes alone: no float
//            atomics, the same bits on every run.
// THE EDGE LAYERS (1 -> 32 with K = 27 and 32 -> 1) are plain VALU kernels
// over the flattened pixels, weights in LDS; their gW / gb are MFMA tiles with
// K = pixels over spans of the flattened pixels.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_dlayer.h"

#define DC_THREADS 256
#define DC_ROWS 4               // output rows of a tile: one a wave
#define DC_COLS 16              // output columns of a tile
#define DC_PITCH 36             // floats of a staged pixel: 32 channels + 4
#define DC_GW_MIN_TILES 4       // fewest tiles of a gW workgroup (but the last)
#define DC_GW_MAX_PARTS 256     // most partials of the 32 -> 32 gW: 28 MB
#define DC_EDGE_CHUNK 2048      // fewest pixels of an edge gW workgroup
#define DC_EDGE_MAX_PARTS 768   // most partials of an edge gW
static_assert(DC_THREADS == DL_THREADS, "the workgroup of pm_dlayer.h");

struct DcArgs {
    const float* x;         // (B, H, W, C)
    const float* w;         // (O, C, 3, kw)
    const float* bias;      // (O)
    const float* g;         // backward: upstream (B, H, Wo, O)
    const float* y;         // backward: the saved output (B, H, Wo, O)
    float* out;             // forward: y; backward: gx (B, H, W, C)
    float* parts;           // backward: (parts, O C 3 kw + O)
    int B, H, W, Wo;
    float slope;
    int tiles, tiles_h, tiles_w;    // the 32 -> 32 kernels
    int per;                // gW: tiles of a workgroup
    long long P;            // edge kernels: B H W pixels
    int span;               // edge gW: pixels of a workgroup, 16 n
};

// six partial sums in a fixed pairwise order
__device__ __forceinline__ dl_f4 dc_sum6(dl_f4 a, dl_f4 b, dl_f4 c, dl_f4 d,
                                         dl_f4 e, dl_f4 f) {
    return ((a + b) + (c + d)) + (e + f);
}

// ---------------------------------------------------------------------------
// 32 -> 32: what the three kernels share
// ---------------------------------------------------------------------------
template <int KW, int S> struct Dc32 {
    static constexpr int PAD = (KW - 1) / 2, TAPS = 3 * KW;
    static constexpr int WEIGHTS = TAPS * 1024;             // floats
    // input pixels a tile of the forward reads in a row, and its float4s
    static constexpr int NP = (DC_COLS - 1) * S + KW;
    static constexpr int XV = (DC_ROWS + 2) * NP * 8;
    static constexpr int XL = (XV + DC_THREADS - 1) / DC_THREADS;
    // gx: input columns of a tile, staged gz pixels of a row, their float4s
    static constexpr int GX_COLS = DC_COLS * S;
    static constexpr int NG = S == 2 ? DC_COLS + 4 : DC_COLS + KW - 1;
    static constexpr int GV = (DC_ROWS + 2) * NG * 8;
    static constexpr int GL = (GV + DC_THREADS - 1) / DC_THREADS;
    // gW: the gz pixels of a tile
    static constexpr int ZV = DC_ROWS * DC_COLS * 8;
    static constexpr int ZL = ZV / DC_THREADS;
};

struct DcTile {
    int b, h0, c0;
    __device__ __forceinline__ DcTile(int t, const DcArgs& a) {
        const int ct = t % a.tiles_w, rest = t / a.tiles_w;
        c0 = ct; h0 = (rest % a.tiles_h) * DC_ROWS; b = rest / a.tiles_h;
    }
};

// The weight to LDS in the order of the A operand: position
//   ((tap 2 + m) 2 + half) 256 + lane 4 + e,  lane = i + 16 k,
// holds W[row 16 m + i][contracted 16 half + 4 k + e][tap]; the rows are the
// output channels (forward) or, TRANS, the input channels (gx).
template <int KW, bool TRANS>
__device__ __forceinline__ void dc_stage_weight(const float* __restrict__ w,
                                                float* wl) {
    constexpr int TAPS = 3 * KW;
    for (int idx = threadIdx.x; idx < TAPS * 1024; idx += DC_THREADS) {
        const int tap = idx % TAPS, oc = idx / TAPS;
        const int o = oc >> 5, c = oc & 31;
        const int row = TRANS ? c : o, con = TRANS ? o : c;
        wl[((tap * 2 + (row >> 4)) * 2 + (con >> 4)) * 256 +
           ((row & 15) + 16 * ((con & 15) >> 2)) * 4 + (con & 3)] = w[idx];
    }
}

// The DC_ROWS + 2 input rows of a forward tile, to registers and on to LDS
template <int KW, int S>
__device__ __forceinline__ void dc_load_x(const DcArgs& a, int t, float4* r) {
    typedef Dc32<KW, S> D;
    if (t >= a.tiles) return;
    const DcTile tile(t, a);
#pragma unroll
    for (int u = 0; u < D::XL; ++u) {
        const int idx = threadIdx.x + u * DC_THREADS;
        const int q = idx & 7, pi = (idx >> 3) % D::NP, row = (idx >> 3) / D::NP;
        const int h = tile.h0 - 1 + row;
        const int w = tile.c0 * DC_COLS * S - D::PAD + pi;
        r[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < D::XV && h >= 0 && h < a.H && w >= 0 && w < a.W)
            r[u] = *(const float4*)(
                a.x + ((long long)(tile.b * a.H + h) * a.W + w) * 32 + 4 * q);
    }
}
template <int KW, int S>
__device__ __forceinline__ void dc_store_x(const float4* r, float* xl) {
    typedef Dc32<KW, S> D;
#pragma unroll
    for (int u = 0; u < D::XL; ++u) {
        const int idx = threadIdx.x + u * DC_THREADS;
        if (idx < D::XV)
            *(float4*)(xl + (idx >> 3) * DC_PITCH + 4 * (idx & 7)) = r[u];
    }
}

// ---------------------------------------------------------------------------
// 32 -> 32 forward. D[o][pixel]; lane l: column l & 15, K element k = l >> 4;
// a lane's two 16-byte reads of a pixel hold the channels 4 k ... 4 k + 3 and
// 16 + 4 k ..., so step e of half h contracts the channels {16 h + 4 k + e}.
// LDS: the weight, then the input rows.
// ---------------------------------------------------------------------------
template <int KW, int S>
__global__ __launch_bounds__(DC_THREADS) void dc_conv32_kernel(DcArgs a) {
    typedef Dc32<KW, S> D;
    extern __shared__ float dc_lds[];
    float* wl = dc_lds;
    float* xl = dc_lds + D::WEIGHTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, k = lane >> 4;
    dc_stage_weight<KW, false>(a.w, wl);
    float bias[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[m][r] = a.bias[16 * m + 4 * k + r];

    float4 regs[D::XL];
    dc_load_x<KW, S>(a, blockIdx.x, regs);
    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        __syncthreads();            // the tile before is read
        dc_store_x<KW, S>(regs, xl);
        __syncthreads();
        dc_load_x<KW, S>(a, t + gridDim.x, regs);
        const DcTile tile(t, a);
        const int h = tile.h0 + wave, wo = tile.c0 * DC_COLS + col;
        if (h >= a.H) continue;     // (the whole wave; it meets the barriers)
        // [kh][channel half][o tile]: twelve independent chains of 36 MFMAs,
        // added pairwise at the end: more in flight, and a shorter sum each
        dl_f4 acc[3][2][2];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc[kh][e >> 1][e & 1] = dl_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < KW; ++kw) {
                const float* px = xl +
                    ((wave + kh) * D::NP + col * S + kw) * DC_PITCH + 4 * k;
                const float4 b0 = *(const float4*)px;
                const float4 b1 = *(const float4*)(px + 16);
                const float* wa = wl + (kh * KW + kw) * 1024 + lane * 4;
                const float4 a00 = *(const float4*)wa;
                const float4 a01 = *(const float4*)(wa + 256);
                const float4 a10 = *(const float4*)(wa + 512);
                const float4 a11 = *(const float4*)(wa + 768);
                DL_MFMA4(acc[kh][0][0], a00, b0);
                DL_MFMA4(acc[kh][0][1], a10, b0);
                DL_MFMA4(acc[kh][1][0], a01, b1);
                DL_MFMA4(acc[kh][1][1], a11, b1);
            }
        }
        const dl_f4 acc0 = dc_sum6(acc[0][0][0], acc[0][1][0], acc[1][0][0],
                                   acc[1][1][0], acc[2][0][0], acc[2][1][0]);
        const dl_f4 acc1 = dc_sum6(acc[0][0][1], acc[0][1][1], acc[1][0][1],
                                   acc[1][1][1], acc[2][0][1], acc[2][1][1]);
        if (wo < a.Wo) {
            float* out = a.out +
                ((long long)(tile.b * a.H + h) * a.Wo + wo) * 32 + 4 * k;
            *(float4*)out = make_float4(
                dl_leaky(acc0[0] + bias[0][0], a.slope),
                dl_leaky(acc0[1] + bias[0][1], a.slope),
                dl_leaky(acc0[2] + bias[0][2], a.slope),
                dl_leaky(acc0[3] + bias[0][3], a.slope));
            *(float4*)(out + 16) = make_float4(
                dl_leaky(acc1[0] + bias[1][0], a.slope),
                dl_leaky(acc1[1] + bias[1][1], a.slope),
                dl_leaky(acc1[2] + bias[1][2], a.slope),
                dl_leaky(acc1[3] + bias[1][3], a.slope));
        }
    }
}

// ---------------------------------------------------------------------------
// 32 -> 32 input gradient, gather form. D[c][input pixel]. A tile is DC_ROWS
// input rows x 16 S input columns: column j of parity p is the input pixel
// w = S (j0 + j) + p, and its tap t (kw = S t + p at s = 2, kw = t at s = 1)
// reads gz at the output column j0 + j + 2 - t (s = 2) or w + PAD - t (s = 1):
// staged pixel j + 4 - t or j + KW - 1 - t of the NG staged ones.
// LDS: the transposed weight, then the gz rows h0 - 1 ... h0 + DC_ROWS.
// ---------------------------------------------------------------------------
template <int KW, int S>
__device__ __forceinline__ void dc_load_gz(const DcArgs& a, int t, float4* gr,
                                           float4* yr) {
    typedef Dc32<KW, S> D;
    if (t >= a.tiles) return;
    const DcTile tile(t, a);
#pragma unroll
    for (int u = 0; u < D::GL; ++u) {
        const int idx = threadIdx.x + u * DC_THREADS;
        const int q = idx & 7, pi = (idx >> 3) % D::NG, row = (idx >> 3) / D::NG;
        const int h = tile.h0 - 1 + row;
        const int wo = tile.c0 * DC_COLS - (S == 2 ? 2 : D::PAD) + pi;
        gr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < D::GV && h >= 0 && h < a.H && wo >= 0 && wo < a.Wo) {
            const long long at =
                ((long long)(tile.b * a.H + h) * a.Wo + wo) * 32 + 4 * q;
            gr[u] = *(const float4*)(a.g + at);
            yr[u] = *(const float4*)(a.y + at);
        }
    }
}

template <int KW, int S>
__global__ __launch_bounds__(DC_THREADS) void dc_gx32_kernel(DcArgs a) {
    typedef Dc32<KW, S> D;
    extern __shared__ float dc_lds[];
    float* wl = dc_lds;
    float* zl = dc_lds + D::WEIGHTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, k = lane >> 4;
    dc_stage_weight<KW, true>(a.w, wl);

    float4 gr[D::GL], yr[D::GL];
    dc_load_gz<KW, S>(a, blockIdx.x, gr, yr);
    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < D::GL; ++u) {
            const int idx = threadIdx.x + u * DC_THREADS;
            if (idx < D::GV)
                *(float4*)(zl + (idx >> 3) * DC_PITCH + 4 * (idx & 7)) =
                    dl_gate4(gr[u], yr[u], a.slope);
        }
        __syncthreads();
        dc_load_gz<KW, S>(a, t + gridDim.x, gr, yr);
        const DcTile tile(t, a);
        const int h = tile.h0 + wave;
        if (h >= a.H) continue;
        // [parity][kh][channel half][c tile], as in the forward
        dl_f4 part[S][3][2][2];
#pragma unroll
        for (int p = 0; p < S; ++p)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    part[p][kh][e >> 1][e & 1] = dl_f4{0.f, 0.f, 0.f, 0.f};
        constexpr int STEPS = S == 2 ? 5 : KW;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int t2 = 0; t2 < STEPS; ++t2) {
                const float* px = zl +
                    ((wave + 2 - kh) * D::NG + col +
                     (S == 2 ? 4 : KW - 1) - t2) * DC_PITCH + 4 * k;
                const float4 b0 = *(const float4*)px;
                const float4 b1 = *(const float4*)(px + 16);
#pragma unroll
                for (int p = 0; p < S; ++p) {
                    const int kw = S == 2 ? 2 * t2 + p : t2;
                    if (kw >= KW) continue;
                    const float* wa = wl + (kh * KW + kw) * 1024 + lane * 4;
                    const float4 a00 = *(const float4*)wa;
                    const float4 a01 = *(const float4*)(wa + 256);
                    const float4 a10 = *(const float4*)(wa + 512);
                    const float4 a11 = *(const float4*)(wa + 768);
                    DL_MFMA4(part[p][kh][0][0], a00, b0);
                    DL_MFMA4(part[p][kh][0][1], a10, b0);
                    DL_MFMA4(part[p][kh][1][0], a01, b1);
                    DL_MFMA4(part[p][kh][1][1], a11, b1);
                }
            }
        }
        dl_f4 acc[S][2];
#pragma unroll
        for (int p = 0; p < S; ++p)
#pragma unroll
            for (int m = 0; m < 2; ++m)
                acc[p][m] = dc_sum6(
                    part[p][0][0][m], part[p][0][1][m], part[p][1][0][m],
                    part[p][1][1][m], part[p][2][0][m], part[p][2][1][m]);
#pragma unroll
        for (int p = 0; p < S; ++p) {
            const int w = S * (tile.c0 * DC_COLS + col) + p;
            if (w >= a.W) continue;
            float* out = a.out +
                ((long long)(tile.b * a.H + h) * a.W + w) * 32 + 4 * k;
            *(float4*)out = make_float4(acc[p][0][0], acc[p][0][1],
                                        acc[p][0][2], acc[p][0][3]);
            *(float4*)(out + 16) = make_float4(acc[p][1][0], acc[p][1][1],
                                               acc[p][1][2], acc[p][1][3]);
        }
    }
}

// ---------------------------------------------------------------------------
// 32 -> 32 weight and bias gradients: see the head of this file. The tiles
// are the forward's. LDS: the x rows as in the forward, then gz (DC_ROWS,
// DC_COLS) pixels, zero outside the map.
// ---------------------------------------------------------------------------
template <int KW, int S>
__device__ __forceinline__ void dc_load_z(const DcArgs& a, int t, float4* gr,
                                          float4* yr) {
    typedef Dc32<KW, S> D;
    if (t >= a.tiles) return;
    const DcTile tile(t, a);
#pragma unroll
    for (int u = 0; u < D::ZL; ++u) {
        const int idx = threadIdx.x + u * DC_THREADS;
        const int q = idx & 7, pi = (idx >> 3) % DC_COLS;
        const int h = tile.h0 + (idx >> 3) / DC_COLS;
        const int wo = tile.c0 * DC_COLS + pi;
        gr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (h < a.H && wo < a.Wo) {
            const long long at =
                ((long long)(tile.b * a.H + h) * a.Wo + wo) * 32 + 4 * q;
            gr[u] = *(const float4*)(a.g + at);
            yr[u] = *(const float4*)(a.y + at);
        }
    }
}

template <int KW, int S>
__global__ __launch_bounds__(DC_THREADS) void dc_gw32_kernel(DcArgs a) {
    typedef Dc32<KW, S> D;
    constexpr int TAPS = D::TAPS;
    extern __shared__ float dc_lds[];
    float* xl = dc_lds;
    float* zl = dc_lds + (DC_ROWS + 2) * D::NP * DC_PITCH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, k = lane >> 4, m = wave >> 1, n = wave & 1;
    dl_f4 acc[TAPS], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) acc[tap] = dl_f4{0.f, 0.f, 0.f, 0.f};

    const int first = blockIdx.x * a.per;
    const int last = first + a.per < a.tiles ? first + a.per : a.tiles;
    float4 xr[D::XL], gr[D::ZL], yr[D::ZL];
    dc_load_x<KW, S>(a, first, xr);
    dc_load_z<KW, S>(a, first, gr, yr);
    for (int t = first; t < last; ++t) {
        __syncthreads();
        dc_store_x<KW, S>(xr, xl);
#pragma unroll
        for (int u = 0; u < D::ZL; ++u) {
            const int idx = threadIdx.x + u * DC_THREADS;
            *(float4*)(zl + (idx >> 3) * DC_PITCH + 4 * (idx & 7)) =
                dl_gate4(gr[u], yr[u], a.slope);
        }
        __syncthreads();
        if (t + 1 < last) {
            dc_load_x<KW, S>(a, t + 1, xr);
            dc_load_z<KW, S>(a, t + 1, gr, yr);
        }
        for (int step = 0; step < DC_ROWS * DC_COLS / 4; ++step) {
            const int row = step >> 2, pc = 4 * (step & 3) + k;
            const float gz = zl[(row * DC_COLS + pc) * DC_PITCH + 16 * m + j];
            const float* px =
                xl + (row * D::NP + pc * S) * DC_PITCH + 16 * n + j;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < KW; ++kw)
                    acc[kh * KW + kw] = DL_MFMA(
                        gz, px[(kh * D::NP + kw) * DC_PITCH],
                        acc[kh * KW + kw]);
            if (n == 0) accb = DL_MFMA(gz, 1.f, accb);
        }
    }
    // rows o = 16 m + 4 k + r, column c = 16 n + j: every float of the partial
    // is written by exactly one thread
    float* part = a.parts + (long long)blockIdx.x * (TAPS * 1024 + 32);
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part[((16 * m + 4 * k + r) * 32 + 16 * n + j) * TAPS + tap] =
                acc[tap][r];
    if (n == 0 && j == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part[TAPS * 1024 + 16 * m + 4 * k + r] = accb[r];
}

// ---------------------------------------------------------------------------
// The edge layers, stride 1: the output pixel p = (b H + h) W + w is the input
// pixel, and tap (kh, kw) is the tap (kh - 1, kw - PAD) of DlPixel.
// ---------------------------------------------------------------------------
// W (O, C, 3, KW) with O C = 32 to LDS as [tap][32]
template <int TAPS>
__device__ __forceinline__ void dc_stage_edge(const float* __restrict__ w,
                                              float* wl) {
    for (int idx = threadIdx.x; idx < TAPS * 32; idx += DC_THREADS)
        wl[(idx % TAPS) * 32 + idx / TAPS] = w[idx];
    __syncthreads();
}

// 1 -> 32 (kw 9), forward: four output channels of a pixel a thread
__global__ __launch_bounds__(DC_THREADS) void dc_conv_c1_kernel(DcArgs a) {
    __shared__ float wl[27 * 32];
    dc_stage_edge<27>(a.w, wl);
    const long long i = (long long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (i >= a.P * 8) return;
    const long long p = i >> 3;
    const int q = (int)(i & 7);
    const DlPixel px(p, a.H, a.W);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 9; ++kw) {
            if (!px.inside(kh - 1, kw - 4, a.H, a.W)) continue;
            const float v = a.x[p + dl_offset(kh - 1, kw - 4, a.W)];
            const float4 w = *(const float4*)(wl + (kh * 9 + kw) * 32 + 4 * q);
            acc.x = fmaf(w.x, v, acc.x);
            acc.y = fmaf(w.y, v, acc.y);
            acc.z = fmaf(w.z, v, acc.z);
            acc.w = fmaf(w.w, v, acc.w);
        }
    const float4 bias = *(const float4*)(a.bias + 4 * q);
    *(float4*)(a.out + p * 32 + 4 * q) = make_float4(
        dl_leaky(acc.x + bias.x, a.slope), dl_leaky(acc.y + bias.y, a.slope),
        dl_leaky(acc.z + bias.z, a.slope), dl_leaky(acc.w + bias.w, a.slope));
}

// 1 -> 32, input gradient: one pixel a thread
__global__ __launch_bounds__(DC_THREADS) void dc_gx_c1_kernel(DcArgs a) {
    __shared__ float wl[27 * 32];
    dc_stage_edge<27>(a.w, wl);
    const long long p = (long long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const DlPixel px(p, a.H, a.W);
    // (four chains of 216 terms, added pairwise: a shorter sum each)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 9; ++kw) {
            if (!px.inside(kh - 1, kw - 4, a.H, a.W, -1)) continue;
            const long long at = (p - dl_offset(kh - 1, kw - 4, a.W)) * 32;
            const float* w = wl + (kh * 9 + kw) * 32;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 gz = dl_gate4(*(const float4*)(a.g + at + 4 * q),
                                           *(const float4*)(a.y + at + 4 * q),
                                           a.slope);
                const float4 u = *(const float4*)(w + 4 * q);
                acc.x = fmaf(u.x, gz.x, acc.x);
                acc.y = fmaf(u.y, gz.y, acc.y);
                acc.z = fmaf(u.z, gz.z, acc.z);
                acc.w = fmaf(u.w, gz.w, acc.w);
            }
        }
    a.out[p] = (acc.x + acc.y) + (acc.z + acc.w);
}

// 32 -> 1 (kw 3), forward: one pixel a thread
__global__ __launch_bounds__(DC_THREADS) void dc_conv_o1_kernel(DcArgs a) {
    __shared__ float wl[9 * 32];
    dc_stage_edge<9>(a.w, wl);
    const long long p = (long long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const DlPixel px(p, a.H, a.W);
    // (four chains of 72 terms, added pairwise)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            if (!px.inside(kh - 1, kw - 1, a.H, a.W)) continue;
            const float* v = a.x + (p + dl_offset(kh - 1, kw - 1, a.W)) * 32;
            const float* w = wl + (kh * 3 + kw) * 32;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 u = *(const float4*)(v + 4 * q);
                const float4 c = *(const float4*)(w + 4 * q);
                acc.x = fmaf(c.x, u.x, acc.x);
                acc.y = fmaf(c.y, u.y, acc.y);
                acc.z = fmaf(c.z, u.z, acc.z);
                acc.w = fmaf(c.w, u.w, acc.w);
            }
        }
    a.out[p] = dl_leaky(
        ((acc.x + acc.y) + (acc.z + acc.w)) + a.bias[0], a.slope);
}

// 32 -> 1, input gradient: four input channels of a pixel a thread
__global__ __launch_bounds__(DC_THREADS) void dc_gx_o1_kernel(DcArgs a) {
    __shared__ float wl[9 * 32];
    dc_stage_edge<9>(a.w, wl);
    const long long i = (long long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (i >= a.P * 8) return;
    const long long p = i >> 3;
    const int q = (int)(i & 7);
    const DlPixel px(p, a.H, a.W);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            if (!px.inside(kh - 1, kw - 1, a.H, a.W, -1)) continue;
            const long long at = p - dl_offset(kh - 1, kw - 1, a.W);
            const float gz = dl_gate(a.g[at], a.y[at], a.slope);
            const float4 w = *(const float4*)(wl + (kh * 3 + kw) * 32 + 4 * q);
            acc.x = fmaf(w.x, gz, acc.x);
            acc.y = fmaf(w.y, gz, acc.y);
            acc.z = fmaf(w.z, gz, acc.z);
            acc.w = fmaf(w.w, gz, acc.w);
        }
    *(float4*)(a.out + p * 32 + 4 * q) = acc;
}

// ---------------------------------------------------------------------------
// gW and gb of the edge layers: MFMA tiles with K = pixels, four pixels a
// step, lane l: pixel l >> 4 of the step, row / column l & 15. A workgroup
// takes `span` flattened pixels, a wave a quarter.
//   1 -> 32: A[o][pixel] = gz (two row tiles), B[pixel][column]: column
//            < 27 is x at that tap, column 27 is one (gb): two column tiles;
//   32 -> 1: A[c][pixel] = x (two row tiles), B[pixel][tap] = gz at the
//            mirrored tap; a third tile has A = 1 in row 0: its column 4 (the
//            centre tap) is gb.
// ---------------------------------------------------------------------------
template <int O> struct DcEdgeGw {
    static constexpr int TAPS = O == 32 ? 27 : 9;
    static constexpr int N = 32 * TAPS + O;     // floats of a partial
    static constexpr int NM = O == 32 ? 4 : 3;
    __device__ static __forceinline__ int slot(int m, int i, int j) {
        if (O == 32) {
            const int o = 16 * (m >> 1) + i, idx = 16 * (m & 1) + j;
            if (idx < 27) return o * 27 + idx;
            return idx == 27 ? 32 * 27 + o : -1;
        }
        if (m < 2) return j < 9 ? (16 * m + i) * 9 + j : -1;
        return (i == 0 && j == 4) ? 32 * 9 : -1;
    }
};

template <int O>
__global__ __launch_bounds__(DC_THREADS) void dc_gw_edge_kernel(DcArgs a) {
    typedef DcEdgeGw<O> G;
    constexpr int NM = G::NM, PAD = O == 32 ? 4 : 1, KW = O == 32 ? 9 : 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, k = lane >> 4;
    dl_f4 acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) acc[m] = dl_f4{0.f, 0.f, 0.f, 0.f};
    const auto [begin, steps] = dl_gw_span(a.P, a.span, wave);
    DlPixel px(begin + k < a.P ? begin + k : 0, a.H, a.W);
    for (int step = 0; step < steps; ++step, px.advance(4, a.H, a.W)) {
        const long long p = begin + step * 4 + k;
        const bool live = p < a.P;
        if (O == 32) {
            float gz0 = 0.f, gz1 = 0.f;
            if (live) {
                gz0 = dl_gate(a.g[p * 32 + j], a.y[p * 32 + j], a.slope);
                gz1 = dl_gate(a.g[p * 32 + 16 + j], a.y[p * 32 + 16 + j],
                              a.slope);
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int idx = 16 * n + j;
                const int dh = idx / 9 - 1, dw = idx % 9 - PAD;
                float v = 0.f;
                if (live && idx == 27) v = 1.f;
                else if (live && idx < 27 && px.inside(dh, dw, a.H, a.W))
                    v = a.x[p + dl_offset(dh, dw, a.W)];
                acc[n] = DL_MFMA(gz0, v, acc[n]);
                acc[2 + n] = DL_MFMA(gz1, v, acc[2 + n]);
            }
        } else {
            const int dh = j / KW - 1, dw = j % KW - PAD;
            float gz = 0.f;
            if (live && j < 9 && px.inside(dh, dw, a.H, a.W, -1)) {
                const long long at = p - dl_offset(dh, dw, a.W);
                gz = dl_gate(a.g[at], a.y[at], a.slope);
            }
            const float x0 = live ? a.x[p * 32 + j] : 0.f;
            const float x1 = live ? a.x[p * 32 + 16 + j] : 0.f;
            acc[0] = DL_MFMA(x0, gz, acc[0]);
            acc[1] = DL_MFMA(x1, gz, acc[1]);
            acc[2] = DL_MFMA(j == 0 ? 1.f : 0.f, gz, acc[2]);
        }
    }
    dl_gw_store<G>(acc, a.parts);
}

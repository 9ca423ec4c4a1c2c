// One conv of the generator's MRF Block (promonet/model/hifigan.py:198-210),
// forward and backward, with its input activation and its residual add:
//   y = conv1d(leaky(x, slope), W, b, dilation d, padding (k - 1) d / 2) [+ r]
// with x, y, r (B, C, T), W (C, C, k), C in {32, 64, 128, 256}, k in {3, 7,
// 11}, d in {1, 3, 5}: 36 forms. slope 1 is no activation.
//
// MEMORY ORDER. channels_last: logical (B, C, T), in memory (B, T, C). A pixel
// is (b, t) flattened; tap j of the pixel p is the pixel p + (j - (k - 1) / 2)
// d where t + (j - (k - 1) / 2) d lies in [0, T), zero otherwise: a tile that
// crosses a batch row carries no tap across it.
//
// ARITHMETIC. fp32 throughout, on v_mfma_f32_16x16x4_f32 (DL_MFMA).
//
// THE KERNELS are implicit GEMMs over flattened pixels, as pc_gemm_kernel and
// pc_gw_kernel (pm_pconv.h) are; the weight chunk and the chains of the
// forward / gx kernel are the shared ones of pm_pixel_gemm.h:
//   forward  M = output channels, N = pixels, K = (tap, channel). A tile is
//            MT rows x GC_NT pixels, a wave 16 pixels of all rows. K runs in
//            chunks of GC_KC channels: the chunk of the weight (the k taps of
//            its channels are contiguous in W) is staged as [tap][row], and
//            the chunk of the tile's pixels ONCE, with the (k - 1) d / 2
//            pixels on either side that the taps reach, leaky applied as it
//            is staged: tap j of the tile's pixel n is the staged row n + j d.
//            A lane knows the t of its pixel and reads zero in place of a tap
//            outside its utterance. The next chunk is in flight in registers
//            under the MFMAs. The sum of an output is split by channel half
//            and chunk parity into four chains, added pairwise. The bias and
//            the residual are added in the epilogue.
//   gx       the same walk over the upstream gradient with the weight read
//            transposed and its taps mirrored (slot k - 1 - j), and
//            leaky'(x) of the saved input, x = 0 taking the slope, in the
//            epilogue.
//   gW, gb   K = pixels in chunks of GC_GW_PIX. A tile is OT output channels
//            x GC_GW_CT input channels x the k taps: A = upstream, B =
//            leaky(x) at the tap, zero outside the utterance; gb is one more
//            accumulator against a column of ones in the tiles of the first
//            input channels. The chunks are split over `parts` workgroups a
//            tile, each writing one partial (C C k + C floats) to the
//            workspace; dl_reduce_kernel adds them in ascending order in
//            double. Their count is a function of the sizes alone: no float
//            atomics, the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_pixel_gemm.h"

#define GC_THREADS 256
#define GC_NT 64                // pixels of a tile of the forward and of gx
#define GC_KC 32                // contracted channels of a K chunk
#define GC_PITCH 36             // floats of a staged row: GC_KC + 4
#define GC_MAX_DILATION 5       // the staged pixels are sized for it
#define GC_GW_PIX 32            // pixels of a K chunk of gW
#define GC_GW_CT 32             // input channels of a gW tile
#define GC_GW_MIN_CHUNKS 2      // fewest chunks of a gW partial (but the last)
#define GC_GW_WORKGROUPS 512    // gW: workgroups wanted, tiles x partials
static_assert(GC_THREADS == DL_THREADS, "the workgroup of pm_dlayer.h");

struct GcArgs {
    const float* x;         // (B, T, C): the input (forward, gW), the gate (gx)
    const float* w;         // (C, C, k)
    const float* bias;      // (C)
    const float* residual;  // forward: (B, T, C) or null
    const float* g;         // backward: upstream (B, T, C)
    float* out;             // forward: y; backward: gx
    float* parts;           // backward: (parts, C C k + C)
    int T, C, d;
    float slope;
    int chunks, per;        // gW: K chunks, and those of a partial
    long long pixels;       // B T
};

// the staged pixel rows of a tile at dilation d
template <int K> __host__ __device__ constexpr int gc_rows(int d) {
    return GC_NT + (K - 1) * d;
}
// floats of dynamic LDS of gc_gemm_kernel<., K, MT>
template <int K, int MT> constexpr int gc_gemm_lds() {
    return (K * MT + gc_rows<K>(GC_MAX_DILATION)) * GC_PITCH;
}

// ---------------------------------------------------------------------------
// The forward (GX false) and the input gradient (GX true): D[row][pixel].
// Lane l: pixel / row l & 15, K element k = l >> 4; a lane's two 16-byte reads
// of a staged row hold the chunk's channels 4 k ... and 16 + 4 k ....
// LDS: the weight [slot][MT rows][GC_PITCH], then the pixels [row][GC_PITCH],
// row r being the pixel (tile's first) - (K - 1) / 2 d + r. Slot s of the
// tile's pixel n is the staged row n + s d; it is the tap s of the forward and
// the tap K - 1 - s of gx.
// ---------------------------------------------------------------------------
template <bool GX, int K, int MT>
__global__ __launch_bounds__(GC_THREADS) void gc_gemm_kernel(GcArgs a) {
    constexpr int MM = MT / 16, HALF = (K - 1) / 2;
    constexpr int AV = pg_weight_vecs<K, MT, GC_KC>();
    constexpr int BV =
        (gc_rows<K>(GC_MAX_DILATION) * 8 + GC_THREADS - 1) / GC_THREADS;
    extern __shared__ float gc_lds[];
    float* wl = gc_lds;
    float* xl = gc_lds + K * MT * GC_PITCH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, k = lane >> 4;
    const float* src = GX ? a.g : a.x;
    const int mtiles = a.C / MT;
    const int m0 = ((int)blockIdx.x % mtiles) * MT;
    const long long first = (long long)((int)blockIdx.x / mtiles) * GC_NT;
    const int rows = gc_rows<K>(a.d);

    // the source pixel of each staged float4 of this thread, or -1
    int from[BV];
#pragma unroll
    for (int u = 0; u < BV; ++u) {
        const int row = (threadIdx.x + u * GC_THREADS) >> 3;
        const long long p = first - HALF * a.d + row;
        from[u] = (row < rows && p >= 0 && p < a.pixels) ? (int)p : -1;
    }

    float4 ar[AV], br[BV];
    auto load = [&](int ci) {
        const int c0 = ci * GC_KC;
        pg_weight_load<GX, K, MT, GC_KC>(ar, a.w, a.C, m0, c0);
#pragma unroll
        for (int u = 0; u < BV; ++u) {
            const int q = (threadIdx.x + u * GC_THREADS) & 7;
            br[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (from[u] >= 0)
                br[u] = *(const float4*)(
                    src + (long long)from[u] * a.C + c0 + 4 * q);
        }
    };
    auto store = [&]() {
        pg_weight_store<GX, K, MT, GC_KC, GC_PITCH>(
            ar, wl, [](int tap) { return GX ? K - 1 - tap : tap; });
#pragma unroll
        for (int u = 0; u < BV; ++u) {
            const int idx = threadIdx.x + u * GC_THREADS;
            if ((idx >> 3) >= rows) continue;
            float4 v = br[u];
            if (!GX) v = dl_leaky4(v, a.slope);
            *(float4*)(xl + (idx >> 3) * GC_PITCH + 4 * (idx & 7)) = v;
        }
    };

    // this lane's pixel and its t; beyond the last pixel every tap is outside
    const long long n = first + wave * 16 + col;
    const int t = n < a.pixels ? (int)((unsigned)n % (unsigned)a.T)
                               : -(1 << 30);

    PgChains<MM> acc;
    auto mma = [&](dl_f4 (&to)[MM][2]) {
#pragma unroll
        for (int slot = 0; slot < K; ++slot) {
            const float* px =
                xl + (wave * 16 + col + slot * a.d) * GC_PITCH + 4 * k;
            float4 b0 = *(const float4*)px;
            float4 b1 = *(const float4*)(px + 16);
            if ((unsigned)(t + (slot - HALF) * a.d) >= (unsigned)a.T) {
                b0 = make_float4(0.f, 0.f, 0.f, 0.f);
                b1 = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int m = 0; m < MM; ++m) {
                const float* wa =
                    wl + (slot * MT + 16 * m + col) * GC_PITCH + 4 * k;
                const float4 a0 = *(const float4*)wa;
                const float4 a1 = *(const float4*)(wa + 16);
                DL_MFMA4(to[m][0], a0, b0);
                DL_MFMA4(to[m][1], a1, b1);
            }
        }
    };

    const int chunks = a.C / GC_KC;
    load(0);
    for (int ci = 0; ci < chunks; ++ci) {
        __syncthreads();            // the chunk before is read
        store();
        __syncthreads();
        if (ci + 1 < chunks) load(ci + 1);
        acc.step(ci, mma);
    }

    if (n >= a.pixels) return;
    const long long at = n * a.C + m0 + 4 * k;
#pragma unroll
    for (int m = 0; m < MM; ++m) {
        const dl_f4 sum = acc.sum(m);
        float4 v = make_float4(sum[0], sum[1], sum[2], sum[3]);
        if (GX) {
            v = dl_gate4(v, *(const float4*)(a.x + at + 16 * m), a.slope);
        } else {
            const float4 bias = *(const float4*)(a.bias + m0 + 16 * m + 4 * k);
            v = make_float4(v.x + bias.x, v.y + bias.y, v.z + bias.z,
                            v.w + bias.w);
            if (a.residual) {
                const float4 r = *(const float4*)(a.residual + at + 16 * m);
                v = make_float4(v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w);
            }
        }
        *(float4*)(a.out + at + 16 * m) = v;
    }
}

// ---------------------------------------------------------------------------
// The weight and bias gradients: see the head of this file. Workgroup (tile,
// part): tile = o tile x c tile, the c tiles fastest. A wave takes 16 output
// channels; at OT = 32 the waves 2 and 3 take them again at the second half of
// the tile's input channels. Lane l: K element (pixel of the step) l >> 4, row
// o / column c l & 15.
// LDS: upstream [GC_GW_PIX][OT + 16], then leaky(x) [tap][GC_GW_PIX][GC_GW_CT
// + 16], zero where the tap or the pixel is outside.
// ---------------------------------------------------------------------------
template <int K, int OT> constexpr int gc_gw_lds() {
    return GC_GW_PIX * (OT + 16 + K * (GC_GW_CT + 16));
}

template <int K, int OT>
__global__ __launch_bounds__(GC_THREADS) void gc_gw_kernel(GcArgs a) {
    constexpr int CT = GC_GW_CT, HALF = (K - 1) / 2;
    constexpr int NN = (CT / 16) / (64 / OT), ZP = OT + 16, XP = CT + 16;
    constexpr int XV = K * GC_GW_PIX * (CT / 4) / GC_THREADS;
    constexpr int ZV = GC_GW_PIX * (OT / 4) / GC_THREADS;
    extern __shared__ float gc_lds[];
    float* zl = gc_lds;
    float* xl = gc_lds + GC_GW_PIX * ZP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, k = lane >> 4;
    const int wo = wave % (OT / 16), wc = wave / (OT / 16);
    const int ctiles = a.C / CT, tiles = ctiles * (a.C / OT);
    const int tile = (int)blockIdx.x % tiles, part = (int)blockIdx.x / tiles;
    const int c0 = (tile % ctiles) * CT, o0 = (tile / ctiles) * OT;
    const bool with_bias = c0 == 0 && wc == 0;

    dl_f4 acc[K][NN], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int n = 0; n < NN; ++n) acc[t][n] = dl_f4{0.f, 0.f, 0.f, 0.f};

    float4 gr[ZV], xr[XV];
    auto load = [&](int chunk) {
#pragma unroll
        for (int u = 0; u < ZV; ++u) {
            const int idx = threadIdx.x + u * GC_THREADS;
            const long long n =
                (long long)chunk * GC_GW_PIX + idx / (OT / 4);
            gr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < a.pixels)
                gr[u] = *(const float4*)(
                    a.g + n * a.C + o0 + 4 * (idx % (OT / 4)));
        }
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int idx = threadIdx.x + u * GC_THREADS;
            const int q = idx % (CT / 4), rest = idx / (CT / 4);
            const int pix = rest % GC_GW_PIX, tap = rest / GC_GW_PIX;
            const long long n = (long long)chunk * GC_GW_PIX + pix;
            xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < a.pixels) {
                const int off = (tap - HALF) * a.d;
                const int t = (int)((unsigned)n % (unsigned)a.T) + off;
                if (t >= 0 && t < a.T)
                    xr[u] = *(const float4*)(
                        a.x + (n + off) * a.C + c0 + 4 * q);
            }
        }
    };

    const int first = part * a.per;
    const int last = first + a.per < a.chunks ? first + a.per : a.chunks;
    if (first < last) load(first);
    for (int chunk = first; chunk < last; ++chunk) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < ZV; ++u) {
            const int idx = threadIdx.x + u * GC_THREADS;
            *(float4*)(zl + (idx / (OT / 4)) * ZP + 4 * (idx % (OT / 4))) =
                gr[u];
        }
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int idx = threadIdx.x + u * GC_THREADS;
            *(float4*)(xl + (idx / (CT / 4)) * XP + 4 * (idx % (CT / 4))) =
                make_float4(dl_leaky(xr[u].x, a.slope),
                            dl_leaky(xr[u].y, a.slope),
                            dl_leaky(xr[u].z, a.slope),
                            dl_leaky(xr[u].w, a.slope));
        }
        __syncthreads();
        if (chunk + 1 < last) load(chunk + 1);
#pragma unroll 2
        for (int step = 0; step < GC_GW_PIX / 4; ++step) {
            const float gz = zl[(4 * step + k) * ZP + 16 * wo + i];
#pragma unroll
            for (int t = 0; t < K; ++t)
#pragma unroll
                for (int n = 0; n < NN; ++n)
                    acc[t][n] = DL_MFMA(
                        gz,
                        xl[(t * GC_GW_PIX + 4 * step + k) * XP +
                           16 * (wc * NN + n) + i],
                        acc[t][n]);
            if (with_bias) accb = DL_MFMA(gz, 1.f, accb);
        }
    }
    // rows o = o0 + 16 wo + 4 k + r, column c = c0 + 16 (wc NN + n) + i: every
    // float of the partial is written by exactly one thread
    const long long weights = (long long)a.C * a.C * K;
    float* base = a.parts + (long long)part * (weights + a.C);
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int n = 0; n < NN; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                base[((long long)(o0 + 16 * wo + 4 * k + r) * a.C + c0 +
                      16 * (wc * NN + n) + i) * K + t] = acc[t][n][r];
    if (with_bias && i == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            base[weights + o0 + 16 * wo + 4 * k + r] = accb[r];
}

// The conv stack of the multi-period discriminator, DiscriminatorP
// (promonet/model/discriminator.py:57-93), forward and backward: a layer is
//   y = leaky(conv2d(x, W, b, stride (s, 1), padding ((k - 1) / 2, 0)), slope)
// with x (B, C, H, P), W (O, C, k, 1), P the period, and (C, O, k, s) one of
//   (1, 32, 5, 3)  (32, 128, 5, 3)  (128, 512, 5, 3)  (512, 1024, 5, 3)
//   (1024, 1024, 5, 1)  (1024, 1, 3, 1).
// The conv runs along H alone; the output is Ho = (H - 1) / s + 1 high and P
// wide. slope 1 is no activation.
//
// MEMORY ORDER. A map of 32 or more channels is channels_last: logical (B, C,
// H, P), in memory (B, H, P, C). The one-channel logits are (B, H, P), the
// audio is (B, T). A pixel is (b, h, w) flattened: tap t of the output pixel
// (b, ho, w) is the input pixel (b, s ho - pad + t, w), P pixels a row apart.
//
// ARITHMETIC. fp32 throughout; the general layers run on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums).
//
// THE GENERAL KERNELS (layers 2 to 5) are implicit GEMMs over flattened
// pixels, so that a tile is full whatever the period and the height; the
// weight chunk and the chains of the forward / gx kernel are the shared ones
// of pm_pixel_gemm.h:
//   forward  M = O, N = output pixels (b, ho, w), K = (tap, channel). A tile
//            is 64 rows x PC_NT pixels, a wave 16 pixels of all rows. K
//            runs in chunks of PC_KC channels: the chunk of the weight (all
//            five taps of a row are contiguous in W) and, per tap, the chunk
//            of the PC_NT input pixels are staged in LDS, PC_PITCH floats a
//            row; the next chunk is in flight in registers under the MFMAs.
//            Every pixel finds its own (b, ho, w), so a tile that crosses a
//            batch row carries no tap across it: a tap outside the map is a
//            zero row. The K = 160 ... 5120 sum of an output is split by
//            channel half and chunk parity into four chains, added pairwise:
//            sixteen independent accumulators a wave.
//   gx       the same kernel on gz = g (y > 0 ? 1 : slope), formed where it
//            is staged, with the rows the input channels and the weight read
//            transposed (32 rows at the 32 channels of the second layer). At
//            s = 1 the input row r reads tap t at the output
//            row r + 2 - t. At s = 3 the input rows are taken by residue
//            class, a tile being of one class: r = 3 j takes tap 2 at the
//            output row j; r = 3 j + 1 taps 0 and 3 at j + 1 and j; r = 3 j +
//            2 taps 1 and 4 at j + 1 and j. Nothing is scattered and every
//            input pixel is written once.
//   gW, gb   K = output pixels in chunks of PC_GW_PIX. A tile is 64 output
//            channels x 64 (32) input channels x the five taps, a wave 16
//            output channels: A = gz, B = x at the tap; gb is one more
//            accumulator against a column of ones in the tiles of the first
//            input channels. The chunks are split over `parts` workgroups a
//            tile, each writing one partial (O C 5 + O floats) to the
//            workspace; dl_reduce_kernel adds the partials in ascending order
//            in double. Their count is a function of the sizes alone: no
//            float atomics, the same bits on every run.
// THE EDGE LAYERS are plain VALU kernels. The first layer (1 -> 32) reads the
// audio in place of the folded map: the pixel (h, w) is the sample t = h P + w
// and, past the end, the sample 2 (T - 1) - t (the reference's right reflect
// pad); its gx is the gradient in the audio, with the adjoint of that pad in
// gather form. The last layer (1024 -> 1) is a 3072-term dot product a pixel,
// one wave a pixel.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_pixel_gemm.h"

#define PC_THREADS 256
#define PC_NT 64                // pixels of a tile of the forward and of gx
#define PC_KC 32                // contracted channels of a K chunk
#define PC_PITCH 36             // floats of a staged row: PC_KC + 4
#define PC_GW_PIX 32            // output pixels of a K chunk of gW
#define PC_GW_MIN_CHUNKS 2      // fewest chunks of a gW partial (but the last)
#define PC_GW_WORKGROUPS 512    // gW: workgroups wanted, tiles x partials
#define PC_FOLD_CHUNK 256       // fewest output pixels of a first-layer partial
#define PC_POST_CHUNK 16        // fewest pixels of a last-layer partial
#define PC_EDGE_MAX_PARTS 1024  // most partials of an edge layer
static_assert(PC_THREADS == DL_THREADS, "the workgroup of pm_dlayer.h");

struct PcArgs {
    const float* x;         // (B, H, P, C); the first layer: the audio (B, T)
    const float* w;         // (O, C, k, 1)
    const float* bias;      // (O)
    const float* g;         // backward: upstream (B, Ho, P, O)
    const float* y;         // backward: the saved output (B, Ho, P, O)
    float* out;             // forward: y; backward: gx
    float* parts;           // backward: (parts, O C k + O)
    int B, H, Ho, P, C, O;
    int T, pad;             // the first layer: samples, reflected samples
    float slope;
    int classes[3];         // gx at s = 3: pixel tiles of each residue class
    int chunks, per;        // gW: K chunks, and those of a partial
    long long pixels;       // edge kernels: B Ho P output pixels
    int span;               // edge gW: pixels of a workgroup
};

// ---------------------------------------------------------------------------
// The general forward (GX false) and input gradient (GX true): D[row][pixel].
// Lane l: pixel / row l & 15, K element k = l >> 4; a lane's two 16-byte reads
// of a staged row hold the chunk's channels 4 k ... and 16 + 4 k ..., so step
// e of half h contracts the channels {16 h + 4 k + e}.
// LDS: the weight [slot][MT rows][PC_PITCH], then the pixels [slot][PC_NT]
// [PC_PITCH]; a slot is a tap (at most two of them for gx at s = 3).
// ---------------------------------------------------------------------------
template <bool GX, int S, int MT>
__global__ __launch_bounds__(PC_THREADS) void pc_gemm_kernel(PcArgs a) {
    constexpr int SLOTS = (GX && S == 3) ? 2 : 5;
    constexpr int MM = MT / 16;
    constexpr int AV = pg_weight_vecs<5, MT, PC_KC>();
    constexpr int BV = SLOTS * PC_NT * 8 / PC_THREADS;
    extern __shared__ float pc_lds[];
    float* wl = pc_lds;
    float* xl = pc_lds + SLOTS * MT * PC_PITCH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, k = lane >> 4;
    // rows M, contracted channels KC of the source map `src`, its height
    const int M = GX ? a.C : a.O, KC = GX ? a.O : a.C;
    const int source_rows = GX ? a.Ho : a.H;
    const float* src = GX ? a.g : a.x;
    const int mtiles = M / MT;
    const int m0 = ((int)blockIdx.x % mtiles) * MT;
    int nt = (int)blockIdx.x / mtiles, cls = 0;
    if (GX && S == 3) {
        if (nt >= a.classes[0]) { nt -= a.classes[0]; cls = 1; }
        if (cls == 1 && nt >= a.classes[1]) { nt -= a.classes[1]; cls = 2; }
    }
    // the rows of the written map that this tile's pixels run over
    const int rows = GX ? (S == 3 ? (a.H > cls ? (a.H - 1 - cls) / 3 + 1 : 0)
                                  : a.H)
                        : a.Ho;
    const unsigned plane = (unsigned)rows * (unsigned)a.P;
    const long long total = (long long)a.B * plane;
    // the taps of the slots (gx at s = 3: one or two of the five)
    const int slots = (GX && S == 3) ? (cls ? 2 : 1) : 5;
    const int tap0 = (cls + 2) % 3, tap1 = cls + 2;

    // the source pixel of each staged float4 of this thread, or -1
    int from[BV];
#pragma unroll
    for (int u = 0; u < BV; ++u) {
        const int idx = threadIdx.x + u * PC_THREADS;
        const int pix = (idx >> 3) & (PC_NT - 1), slot = idx >> 9;
        const long long n = (long long)nt * PC_NT + pix;
        from[u] = -1;
        if (n < total && slot < slots) {
            const unsigned b = (unsigned)n / plane, rem = (unsigned)n % plane;
            const int j = (int)(rem / (unsigned)a.P);
            const int w = (int)(rem % (unsigned)a.P);
            int row;
            if (!GX) row = S * j - 2 + slot;
            else if (S == 1) row = j + 2 - slot;
            else row = slot == 0 ? j + (cls ? 1 : 0) : j;
            if (row >= 0 && row < source_rows)
                from[u] = (int)((b * (unsigned)source_rows + (unsigned)row) *
                                (unsigned)a.P) + w;
        }
    }

    float4 ar[AV], br[BV], yr[GX ? BV : 1];
    auto load = [&](int ci) {
        const int c0 = ci * PC_KC;
        pg_weight_load<GX, 5, MT, PC_KC>(ar, a.w, a.C, m0, c0);
#pragma unroll
        for (int u = 0; u < BV; ++u) {
            const int q = (threadIdx.x + u * PC_THREADS) & 7;
            br[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (GX) yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (from[u] >= 0) {
                const long long at = (long long)from[u] * KC + c0 + 4 * q;
                br[u] = *(const float4*)(src + at);
                if constexpr (GX) yr[u] = *(const float4*)(a.y + at);
            }
        }
    };
    auto store = [&]() {
        pg_weight_store<GX, 5, MT, PC_KC, PC_PITCH>(ar, wl, [&](int tap) {
            if (GX && S == 3)
                return tap == tap0 ? 0 : (cls && tap == tap1) ? 1 : -1;
            return tap;
        });
#pragma unroll
        for (int u = 0; u < BV; ++u) {
            const int idx = threadIdx.x + u * PC_THREADS;
            float4 v = br[u];
            if constexpr (GX) v = dl_gate4(br[u], yr[u], a.slope);
            *(float4*)(xl + (idx >> 3) * PC_PITCH + 4 * (idx & 7)) = v;
        }
    };

    PgChains<MM> acc;
    auto mma = [&](dl_f4 (&to)[MM][2]) {
#pragma unroll
        for (int slot = 0; slot < SLOTS; ++slot) {
            if (slot >= slots) break;
            const float* px =
                xl + (slot * PC_NT + wave * 16 + col) * PC_PITCH + 4 * k;
            const float4 b0 = *(const float4*)px;
            const float4 b1 = *(const float4*)(px + 16);
#pragma unroll
            for (int m = 0; m < MM; ++m) {
                const float* wa =
                    wl + (slot * MT + 16 * m + col) * PC_PITCH + 4 * k;
                const float4 a0 = *(const float4*)wa;
                const float4 a1 = *(const float4*)(wa + 16);
                DL_MFMA4(to[m][0], a0, b0);
                DL_MFMA4(to[m][1], a1, b1);
            }
        }
    };
    const int chunks = KC / PC_KC;
    load(0);
    for (int ci = 0; ci < chunks; ++ci) {
        __syncthreads();            // the chunk before is read
        store();
        __syncthreads();
        if (ci + 1 < chunks) load(ci + 1);
        acc.step(ci, mma);
    }

    const long long n = (long long)nt * PC_NT + wave * 16 + col;
    if (n >= total) return;
    long long pixel = n;
    if (GX && S == 3) {
        const unsigned b = (unsigned)n / plane, rem = (unsigned)n % plane;
        const unsigned j = rem / (unsigned)a.P, w = rem % (unsigned)a.P;
        pixel = ((long long)b * a.H + 3 * j + cls) * a.P + w;
    }
    float* out = a.out + pixel * M + m0 + 4 * k;
#pragma unroll
    for (int m = 0; m < MM; ++m) {
        const dl_f4 sum = acc.sum(m);
        if (GX) {
            *(float4*)(out + 16 * m) =
                make_float4(sum[0], sum[1], sum[2], sum[3]);
        } else {
            const float4 bias = *(const float4*)(a.bias + m0 + 16 * m + 4 * k);
            *(float4*)(out + 16 * m) = make_float4(
                dl_leaky(sum[0] + bias.x, a.slope),
                dl_leaky(sum[1] + bias.y, a.slope),
                dl_leaky(sum[2] + bias.z, a.slope),
                dl_leaky(sum[3] + bias.w, a.slope));
        }
    }
}

// ---------------------------------------------------------------------------
// The general weight and bias gradients: see the head of this file. Workgroup
// (tile, part): tile = o tile x c tile, the c tiles fastest. Lane l: K element
// (pixel of the step) l >> 4, row o / column c l & 15.
// LDS: gz [PC_GW_PIX][64 + 16], then x [tap][PC_GW_PIX][CT + 16], zero where
// the tap or the pixel is outside.
// ---------------------------------------------------------------------------
template <int S, int CT>
__global__ __launch_bounds__(PC_THREADS) void pc_gw_kernel(PcArgs a) {
    constexpr int NN = CT / 16, ZP = 64 + 16, XP = CT + 16;
    constexpr int XV = 5 * PC_GW_PIX * (CT / 4) / PC_THREADS;
    constexpr int ZV = PC_GW_PIX * 16 / PC_THREADS;
    extern __shared__ float pc_lds[];
    float* zl = pc_lds;
    float* xl = pc_lds + PC_GW_PIX * ZP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, k = lane >> 4;
    const int ctiles = a.C / CT, tiles = ctiles * (a.O / 64);
    const int tile = (int)blockIdx.x % tiles, part = (int)blockIdx.x / tiles;
    const int c0 = (tile % ctiles) * CT, o0 = (tile / ctiles) * 64;
    const bool with_bias = c0 == 0;
    const unsigned plane = (unsigned)a.Ho * (unsigned)a.P;

    dl_f4 acc[5][NN], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int n = 0; n < NN; ++n) acc[t][n] = dl_f4{0.f, 0.f, 0.f, 0.f};

    float4 gr[ZV], yr[ZV], xr[XV];
    auto load = [&](int chunk) {
#pragma unroll
        for (int u = 0; u < ZV; ++u) {
            const int idx = threadIdx.x + u * PC_THREADS;
            const long long n = (long long)chunk * PC_GW_PIX + (idx >> 4);
            gr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < a.pixels) {
                const long long at = n * a.O + o0 + 4 * (idx & 15);
                gr[u] = *(const float4*)(a.g + at);
                yr[u] = *(const float4*)(a.y + at);
            }
        }
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int idx = threadIdx.x + u * PC_THREADS;
            const int q = idx % (CT / 4), rest = idx / (CT / 4);
            const int pix = rest % PC_GW_PIX, tap = rest / PC_GW_PIX;
            const long long n = (long long)chunk * PC_GW_PIX + pix;
            xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < a.pixels) {
                const unsigned b = (unsigned)n / plane;
                const unsigned rem = (unsigned)n % plane;
                const int ho = (int)(rem / (unsigned)a.P);
                const int w = (int)(rem % (unsigned)a.P);
                const int row = S * ho - 2 + tap;
                if (row >= 0 && row < a.H)
                    xr[u] = *(const float4*)(
                        a.x + (((long long)b * a.H + row) * a.P + w) * a.C +
                        c0 + 4 * q);
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
            const int idx = threadIdx.x + u * PC_THREADS;
            *(float4*)(zl + (idx >> 4) * ZP + 4 * (idx & 15)) =
                dl_gate4(gr[u], yr[u], a.slope);
        }
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int idx = threadIdx.x + u * PC_THREADS;
            *(float4*)(xl + (idx / (CT / 4)) * XP + 4 * (idx % (CT / 4))) =
                xr[u];
        }
        __syncthreads();
        if (chunk + 1 < last) load(chunk + 1);
#pragma unroll 2
        for (int step = 0; step < PC_GW_PIX / 4; ++step) {
            const float gz = zl[(4 * step + k) * ZP + 16 * wave + i];
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int n = 0; n < NN; ++n)
                    acc[t][n] = DL_MFMA(
                        gz, xl[(t * PC_GW_PIX + 4 * step + k) * XP + 16 * n + i],
                        acc[t][n]);
            if (with_bias) accb = DL_MFMA(gz, 1.f, accb);
        }
    }
    // rows o = o0 + 16 wave + 4 k + r, column c = c0 + 16 n + i: every float
    // of the partial is written by exactly one thread
    float* base = a.parts + (long long)part * ((long long)a.O * a.C * 5 + a.O);
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int n = 0; n < NN; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                base[((long long)(o0 + 16 * wave + 4 * k + r) * a.C + c0 +
                      16 * n + i) * 5 + t] = acc[t][n][r];
    if (with_bias && i == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            base[(long long)a.O * a.C * 5 + o0 + 16 * wave + 4 * k + r] =
                accb[r];
}

// ---------------------------------------------------------------------------
// The first layer, 1 -> 32 at k 5, s 3, on the audio (B, T). The folded map
// is (B, H, P) with H = (T + pad) / P; its pixel (h, w) is the sample h P + w,
// reflected about T - 1 past the end. 32-bit pixel arithmetic: the host
// refuses more than 2^31 - 1 pixels. The batch row of a pixel (DlBatchPixel)
// finds the audio.
// ---------------------------------------------------------------------------

// the folded map at row h (zero outside), column w of the batch row `audio`
__device__ __forceinline__ float pc_folded(const float* __restrict__ audio,
                                           int h, int w, const PcArgs& a) {
    if (h < 0 || h >= a.H) return 0.f;
    int t = h * a.P + w;
    if (t >= a.T) t = 2 * (a.T - 1) - t;
    return audio[t];
}

// W (32, 1, 5, 1) to LDS as [tap][32]
__device__ __forceinline__ void pc_stage_first(const float* __restrict__ w,
                                               float* wl) {
    for (int idx = threadIdx.x; idx < 160; idx += PC_THREADS)
        wl[(idx % 5) * 32 + idx / 5] = w[idx];
    __syncthreads();
}

// forward: four output channels of a pixel a thread
__global__ __launch_bounds__(PC_THREADS) void pc_fold_conv_kernel(PcArgs a) {
    __shared__ float wl[160];
    pc_stage_first(a.w, wl);
    const long long idx = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (idx >= a.pixels * 8) return;
    const long long p = idx >> 3;
    const int q = (int)(idx & 7);
    const DlBatchPixel px(p, a.Ho, a.P);
    const float* audio = a.x + (long long)px.b * a.T;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const float v = pc_folded(audio, 3 * px.h - 2 + t, px.w, a);
        const float4 w = *(const float4*)(wl + t * 32 + 4 * q);
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

// The gradient of the folded map at the position pos = h P + w of a batch
// row: the taps t with 3 ho - 2 + t = h
__device__ __forceinline__ float pc_fold_gather(const PcArgs& a,
                                                const float* wl, int b,
                                                int pos) {
    const int h = pos / a.P, w = pos - h * a.P;
    // (four chains, added pairwise: a shorter sum each)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < 5; ++t) {
        const int num = h + 2 - t;
        if (num < 0 || num % 3 != 0 || num / 3 >= a.Ho) continue;
        const long long at =
            (((long long)b * a.Ho + num / 3) * a.P + w) * 32;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 gz = dl_gate4(*(const float4*)(a.g + at + 4 * q),
                                       *(const float4*)(a.y + at + 4 * q),
                                       a.slope);
            const float4 u = *(const float4*)(wl + t * 32 + 4 * q);
            acc.x = fmaf(u.x, gz.x, acc.x);
            acc.y = fmaf(u.y, gz.y, acc.y);
            acc.z = fmaf(u.z, gz.z, acc.z);
            acc.w = fmaf(u.w, gz.w, acc.w);
        }
    }
    return (acc.x + acc.y) + (acc.z + acc.w);
}

// the gradient in the audio, one sample a thread: the sample's own position
// and, for T - 1 - pad <= t <= T - 2, the position 2 (T - 1) - t that reflects
// onto it
__global__ __launch_bounds__(PC_THREADS) void pc_fold_gx_kernel(PcArgs a) {
    __shared__ float wl[160];
    pc_stage_first(a.w, wl);
    const long long idx = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (idx >= (long long)a.B * a.T) return;
    const int b = (int)(idx / a.T), t = (int)(idx % a.T);
    float sum = pc_fold_gather(a, wl, b, t);
    if (t >= a.T - 1 - a.pad && t <= a.T - 2)
        sum += pc_fold_gather(a, wl, b, 2 * (a.T - 1) - t);
    a.out[idx] = sum;
}

// gW (32, 1, 5, 1) and gb: a workgroup takes `span` output pixels, thread
// (slice = tid / 32, o = tid % 32) every eighth of them in ascending order;
// the eight slices are added in order. One partial of 160 + 32 floats.
__global__ __launch_bounds__(PC_THREADS) void pc_fold_gw_kernel(PcArgs a) {
    __shared__ float lds[8][6][32];
    const int o = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const long long begin = (long long)blockIdx.x * a.span;
    const long long end =
        begin + a.span < a.pixels ? begin + a.span : a.pixels;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long p = begin + slice; p < end; p += 8) {
        const DlBatchPixel px(p, a.Ho, a.P);
        const float* audio = a.x + (long long)px.b * a.T;
        const float gz = dl_gate(a.g[p * 32 + o], a.y[p * 32 + o], a.slope);
#pragma unroll
        for (int t = 0; t < 5; ++t)
            acc[t] = fmaf(gz, pc_folded(audio, 3 * px.h - 2 + t, px.w, a),
                          acc[t]);
        acc[5] += gz;
    }
#pragma unroll
    for (int t = 0; t < 6; ++t) lds[slice][t][o] = acc[t];
    __syncthreads();
    if (threadIdx.x >= 192) return;
    const int t = threadIdx.x >> 5;
    float sum = lds[0][t][o];
    for (int s = 1; s < 8; ++s) sum += lds[s][t][o];
    a.parts[(long long)blockIdx.x * 192 + (t < 5 ? o * 5 + t : 160 + o)] = sum;
}

// ---------------------------------------------------------------------------
// The last layer, 1024 -> 1 at k 3, s 1: W (1, 1024, 3, 1), the three taps of
// a channel in a run. Tap t of the pixel p is the pixel p + (t - 1) P where
// its row lies inside the map.
// ---------------------------------------------------------------------------

// forward: one pixel a wave, a lane 16 channels x 3 taps, the lanes added by
// a butterfly in a fixed order
__global__ __launch_bounds__(PC_THREADS) void pc_post_conv_kernel(PcArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * 4 + wave;
    if (p >= a.pixels) return;
    const DlBatchPixel px(p, a.H, a.P);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = 4 * (lane + 64 * u);
        float wv[12];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const float4 w = *(const float4*)(a.w + 3 * c + 4 * f);
            wv[4 * f] = w.x; wv[4 * f + 1] = w.y;
            wv[4 * f + 2] = w.z; wv[4 * f + 3] = w.w;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int h = px.h - 1 + t;
            if (h < 0 || h >= a.H) continue;
            const float4 v = *(const float4*)(
                a.x + (p + (long long)(t - 1) * a.P) * 1024 + c);
            acc.x = fmaf(wv[t], v.x, acc.x);
            acc.y = fmaf(wv[3 + t], v.y, acc.y);
            acc.z = fmaf(wv[6 + t], v.z, acc.z);
            acc.w = fmaf(wv[9 + t], v.w, acc.w);
        }
    }
    float sum = (acc.x + acc.y) + (acc.z + acc.w);
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) sum += __shfl_xor(sum, step, 64);
    if (lane == 0) a.out[p] = dl_leaky(sum + a.bias[0], a.slope);
}

// input gradient: four input channels of a pixel a thread
__global__ __launch_bounds__(PC_THREADS) void pc_post_gx_kernel(PcArgs a) {
    const long long idx = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (idx >= a.pixels * 256) return;
    const long long p = idx >> 8;
    const int c = 4 * (int)(idx & 255);
    const DlBatchPixel px(p, a.H, a.P);
    float wv[12];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const float4 w = *(const float4*)(a.w + 3 * c + 4 * f);
        wv[4 * f] = w.x; wv[4 * f + 1] = w.y;
        wv[4 * f + 2] = w.z; wv[4 * f + 3] = w.w;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int h = px.h + 1 - t;
        if (h < 0 || h >= a.H) continue;
        const long long at = p + (long long)(1 - t) * a.P;
        const float gz = dl_gate(a.g[at], a.y[at], a.slope);
        acc.x = fmaf(wv[t], gz, acc.x);
        acc.y = fmaf(wv[3 + t], gz, acc.y);
        acc.z = fmaf(wv[6 + t], gz, acc.z);
        acc.w = fmaf(wv[9 + t], gz, acc.w);
    }
    *(float4*)(a.out + p * 1024 + c) = acc;
}

// gW (1, 1024, 3, 1) and gb: a workgroup takes `span` pixels in ascending
// order, a thread four channels x three taps; thread 0 adds gb. One partial
// of 3072 + 1 floats.
__global__ __launch_bounds__(PC_THREADS) void pc_post_gw_kernel(PcArgs a) {
    const int c = 4 * threadIdx.x;
    const long long begin = (long long)blockIdx.x * a.span;
    const long long end =
        begin + a.span < a.pixels ? begin + a.span : a.pixels;
    float acc[4][3] = {};
    float accb = 0.f;
    for (long long p = begin; p < end; ++p) {
        const DlBatchPixel px(p, a.H, a.P);
        const float4 v = *(const float4*)(a.x + p * 1024 + c);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int h = px.h + 1 - t;
            if (h < 0 || h >= a.H) continue;
            const long long at = p + (long long)(1 - t) * a.P;
            const float gz = dl_gate(a.g[at], a.y[at], a.slope);
            acc[0][t] = fmaf(gz, v.x, acc[0][t]);
            acc[1][t] = fmaf(gz, v.y, acc[1][t]);
            acc[2][t] = fmaf(gz, v.z, acc[2][t]);
            acc[3][t] = fmaf(gz, v.w, acc[3][t]);
            if (t == 1) accb += gz;
        }
    }
    float* part = a.parts + (long long)blockIdx.x * 3073;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 3; ++t) part[(c + e) * 3 + t] = acc[e][t];
    if (threadIdx.x == 0) part[3072] = accb;
}

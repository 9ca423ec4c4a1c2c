// The strided, wider layers of the FARGAN discriminator's conv stacks: what
// DiscriminatorMagFree builds at n_fft 128 ... 2048 beside the forms of
// pm_fdisc.h. A layer is
//   y = act(conv2d(cat(x, sin, cos), W, b, stride (s, 1), padding (1, 1)))
// with x (B, C, F, T), W (O, C + 2, 3, 3), s in {1, 2}, the output
// Fo = (F - 1) / s + 1 bins high: output row fo reads the input rows
// s fo + kf - 1, zero outside [0, F) for the map and the embedding alike. The
// embedding is that of the INPUT: sin, cos of 2 pi f / F from the (F, 2) table,
// read at the tap's input row. (C, O, s) is one of
//   (1, 16, 2)
//   (16, 32, s) (32, 64, s) (64, 128, s) (128, 256, s)
//   (32, 32, 1) (64, 64, 1) (128, 128, 1)
//   (32, 1, 1) (64, 1, 1) (128, 1, 1) (256, 1, 1).
// Memory order and arithmetic are pm_fdisc.h's: channels_last maps, fp32, the
// general layers on v_mfma_f32_16x16x4_f32.
//
// THE GENERAL KERNEL (fs_gemm_kernel) is an implicit GEMM over flattened
// pixels, forward and gx alike, as pc_gemm_kernel (pm_pconv.h) is:
//   forward  rows = output channels in tiles of MT = 32 or 64, columns = FS_NT
//            output pixels (b, fo, t), a wave 16 pixels of all rows. K runs in
//            chunks of (one frequency tap, FS_KC channels, the three time
//            taps): the chunk of the weight and of the FS_NT pixels at each
//            time tap are staged in LDS, FS_PITCH floats a row, the next chunk
//            in flight in registers under the MFMAs. Every pixel finds its own
//            (b, fo, t): a tile that crosses a batch row or a frequency row
//            carries no tap across it. The sum is split by chunk parity and
//            row block: 2 MT / 16 independent accumulators a wave. The
//            embedding is six more K steps (tap, sin | cos) from the table.
//   gx       the same kernel on gz = g act'(y), formed where it is staged,
//            the rows the input channels, the weight read transposed and the
//            time tap mirrored. At s = 1 the input row f reads tap kf at the
//            output row f + 1 - kf. At s = 2 a tile is of one parity: an even
//            row 2 j has tap 1 alone (output row j), an odd row 2 j + 1 tap 0
//            (row j + 1, where it exists) and tap 2 (row j): one or two chunks
//            a channel block, none for a tap that does not reach the row.
//            Nothing is scattered, every input pixel is written once.
//   gW, gb   (fs_gw_kernel) K = output pixels in chunks of FS_GW_PIX. A tile
//            is 4 / CB blocks of 16 output channels x CB blocks of 16 input
//            channels x the nine taps, a wave one block pair: A = gz, B = x at
//            the tap. The waves of the first input channel block also hold
//            the 18 embedding pairs and a column of ones (gb). `parts`
//            workgroups a tile each write a partial (O (C + 2) 9 + O floats);
//            dl_reduce_kernel adds them in a fixed order in double. Their
//            count is a function of the sizes alone: no float atomics.
// THE EDGES are plain VALU kernels: the first layer (1 -> 16 at s = 2) with
// its gx and gW, and the last (C -> 1 at s = 1, C = 32 ... 256) likewise.
//
// NON-FINITE VALUES. This header promises torch's semantics on inf and NaN
// (DESIGN section 27), with pm_fdisc.h's activation and gate: a non-finite
// input or upstream reaches exactly the outputs that a tap links it to, and no
// other element changes a bit.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_fdisc.h"

#define FS_NT 64                // pixels of a tile of the forward and of gx
#define FS_KC 16                // contracted channels of a K chunk
#define FS_PITCH 20             // floats of a staged row: FS_KC + 4
#define FS_GW_PIX 16            // output pixels of a K chunk of gW
#define FS_GW_MIN_CHUNKS 2      // fewest chunks of a gW partial (but the last)
#define FS_GW_WORKGROUPS 512    // gW: workgroups wanted, tiles x partials
#define FS_EDGE_CHUNK 1024      // fewest pixels of an edge gW partial
#define FS_EDGE_MAX_PARTS 768   // most partials of an edge layer

struct FsArgs {
    const float* x;         // (B, F, T, C)
    const float* w;         // (O, C + 2, 3, 3)
    const float* bias;      // (O)
    const float* table;     // (F, 2): sin, cos of 2 pi f / F
    const float* g;         // backward: upstream (B, Fo, T, O)
    const float* y;         // backward: the saved output (B, Fo, T, O)
    float* out;             // forward: y; backward: gx
    float* parts;           // backward: (parts, O (C + 2) 9 + O)
    int B, F, Fo, T, C, O, s, act;
    int classes[2];         // gx at s = 2: pixel tiles of each parity
    int chunks, per;        // gW: K chunks, and those of a partial
    long long pixels;       // edge kernels: the pixels they walk
    int span;               // edge gW: pixels of a workgroup
};

// (A pixel of a flattened (B, rows, T) map is a DlBatchPixel: h its frequency
// row, w its frame.)
__device__ __forceinline__ float4 fs_gate4(float4 g, float4 y, int act) {
    return make_float4(fd_gate(g.x, y.x, act), fd_gate(g.y, y.y, act),
                       fd_gate(g.z, y.z, act), fd_gate(g.w, y.w, act));
}

// ---------------------------------------------------------------------------
// The general forward (GX false) and input gradient (GX true): D[row][pixel].
// Lane l: pixel / row l & 15, K element k = l >> 4; a lane's 16-byte read of a
// staged row holds the chunk's channels 4 k ..., so step e contracts the
// channels {4 k + e}.
// LDS: the weight [time tap][MT rows][FS_PITCH] and the pixels [time tap]
// [FS_NT][FS_PITCH]: 240 (MT + FS_NT) bytes, 30 720 at MT = 64.
// ---------------------------------------------------------------------------
template <bool GX, int S, int MT>
__global__ __launch_bounds__(FD_THREADS) void fs_gemm_kernel(FsArgs a) {
    constexpr int MM = MT / 16;
    constexpr int AV = MT * FS_KC * 3 / FD_THREADS;
    static_assert(AV * FD_THREADS == MT * FS_KC * 3, "whole loads a thread");
    static_assert(FS_NT * FS_KC / 4 == FD_THREADS, "a float4 a time tap");
    __shared__ __attribute__((aligned(16))) float wl[3 * MT * FS_PITCH];
    __shared__ __attribute__((aligned(16))) float xl[3 * FS_NT * FS_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, k = lane >> 4;
    // rows M, contracted channels KC of the source map `src`, its height
    const int M = GX ? a.C : a.O, KC = GX ? a.O : a.C;
    const int CIN = a.C + 2;
    const int source_rows = GX ? a.Fo : a.F;
    const float* src = GX ? a.g : a.x;
    const int mtiles = M / MT;
    const int m0 = ((int)blockIdx.x % mtiles) * MT;
    int nt = (int)blockIdx.x / mtiles, cls = 0;
    if (GX && S == 2 && nt >= a.classes[0]) { nt -= a.classes[0]; cls = 1; }
    // the rows of the written map that this tile's pixels run over
    const int rows = GX ? (S == 2 ? (a.F + 1 - cls) / 2 : a.F) : a.Fo;
    const long long total = (long long)a.B * rows * a.T;
    // the frequency taps of the slots (gx at s = 2: one or two of the three)
    const int slots = (GX && S == 2) ? 1 + cls : 3;
    auto tap_of = [&](int slot) {
        return (GX && S == 2) ? (cls ? 2 * slot : 1) : slot;
    };
    // the source row that the written row j reads at the slot
    auto row_of = [&](int slot, int j) {
        if (!GX) return S * j - 1 + slot;
        if (S == 1) return j + 1 - slot;
        return cls ? j + 1 - slot : j;
    };

    // the pixel whose chunk this thread stages, the same at every time tap
    const long long ns = (long long)nt * FS_NT + ((threadIdx.x >> 2) & 63);
    const bool staged = ns < total;
    const DlBatchPixel sp(staged ? ns : 0, rows, a.T);
    const int q = threadIdx.x & 3;
    const int cblocks = KC / FS_KC;

    float ar[AV];
    float4 br[3], yr[GX ? 3 : 1];
    auto load = [&](int ci) {
        const int slot = ci / cblocks, c0 = (ci % cblocks) * FS_KC;
        const int kf = tap_of(slot);
#pragma unroll
        for (int u = 0; u < AV; ++u) {
            const int idx = threadIdx.x + u * FD_THREADS;
            const int kt = idx % 3, pair = idx / 3;
            // (the three time taps of a (row, channel) are a run in W)
            const int row = GX ? pair % MT : pair / FS_KC;
            const int con = GX ? pair / MT : pair % FS_KC;
            const int o = GX ? c0 + con : m0 + row;
            const int c = GX ? m0 + row : c0 + con;
            ar[u] = a.w[((long long)o * CIN + c) * 9 + kf * 3 + kt];
        }
        const int row = row_of(slot, sp.h);
        const bool ok = staged && row >= 0 && row < source_rows;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int tt = sp.w + (GX ? 1 - u : u - 1);
            br[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (GX) yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && tt >= 0 && tt < a.T) {
                const long long at =
                    (((long long)sp.b * source_rows + row) * a.T + tt) * KC +
                    c0 + 4 * q;
                br[u] = *(const float4*)(src + at);
                if constexpr (GX) yr[u] = *(const float4*)(a.y + at);
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int u = 0; u < AV; ++u) {
            const int idx = threadIdx.x + u * FD_THREADS;
            const int kt = idx % 3, pair = idx / 3;
            const int row = GX ? pair % MT : pair / FS_KC;
            const int con = GX ? pair / MT : pair % FS_KC;
            wl[(kt * MT + row) * FS_PITCH + con] = ar[u];
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int idx = threadIdx.x + u * FD_THREADS;
            float4 v = br[u];
            if constexpr (GX) v = fs_gate4(br[u], yr[u], a.act);
            *(float4*)(xl + (idx >> 2) * FS_PITCH + 4 * (idx & 3)) = v;
        }
    };

    // [chunk parity][row block]
    dl_f4 acc[2][MM];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int m = 0; m < MM; ++m) acc[p][m] = dl_f4{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](dl_f4 (&to)[MM]) {
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const float4 b = *(const float4*)(
                xl + (kt * FS_NT + wave * 16 + col) * FS_PITCH + 4 * k);
#pragma unroll
            for (int m = 0; m < MM; ++m) {
                const float4 w = *(const float4*)(
                    wl + (kt * MT + 16 * m + col) * FS_PITCH + 4 * k);
                DL_MFMA4(to[m], w, b);
            }
        }
    };

    const int chunks = slots * cblocks;
    load(0);
    for (int ci = 0; ci < chunks; ++ci) {
        __syncthreads();            // the chunk before is read
        store();
        __syncthreads();
        if (ci + 1 < chunks) load(ci + 1);
        if (ci & 1) mma(acc[1]);
        else mma(acc[0]);
    }

    const long long n = (long long)nt * FS_NT + wave * 16 + col;
    const bool live = n < total;
    const DlBatchPixel px(live ? n : 0, rows, a.T);
    if constexpr (!GX) {
        // the embedding: K element 4 step + k is (time tap, sin | cos), six
        // of the eight, read from the table at the tap's input row
#pragma unroll
        for (int kf = 0; kf < 3; ++kf) {
            const int row = S * px.h - 1 + kf;
            const bool ok = live && row >= 0 && row < a.F;
#pragma unroll
            for (int step = 0; step < 2; ++step) {
                const int id = 4 * step + k, kt = id >> 1, e = id & 1;
                const int tt = px.w + kt - 1;
                float v = 0.f;
                if (ok && id < 6 && tt >= 0 && tt < a.T)
                    v = a.table[2 * row + e];
#pragma unroll
                for (int m = 0; m < MM; ++m) {
                    const float w = id < 6
                        ? a.w[((long long)(m0 + 16 * m + col) * CIN + a.C +
                               e) * 9 + kf * 3 + kt]
                        : 0.f;
                    acc[step][m] = DL_MFMA(w, v, acc[step][m]);
                }
            }
        }
    }
    if (!live) return;
    long long pixel = n;
    if (GX && S == 2)
        pixel = ((long long)px.b * a.F + 2 * px.h + cls) * a.T + px.w;
    float* out = a.out + pixel * M + m0 + 4 * k;
#pragma unroll
    for (int m = 0; m < MM; ++m) {
        const dl_f4 sum = acc[0][m] + acc[1][m];
        if (GX) {
            *(float4*)(out + 16 * m) =
                make_float4(sum[0], sum[1], sum[2], sum[3]);
        } else {
            const float4 bias = *(const float4*)(a.bias + m0 + 16 * m + 4 * k);
            *(float4*)(out + 16 * m) = make_float4(
                fd_activate(sum[0] + bias.x, a.act),
                fd_activate(sum[1] + bias.y, a.act),
                fd_activate(sum[2] + bias.z, a.act),
                fd_activate(sum[3] + bias.w, a.act));
        }
    }
}

// ---------------------------------------------------------------------------
// The general weight and bias gradients: see the head of this file. Workgroup
// (tile, part): tile = o tile x c tile, the c tiles fastest; wave (ob, cb) of
// the tile's 4 / CB x CB blocks. Lane l: K element (pixel of the step) l >> 4,
// row o / column c l & 15.
// LDS: gz [FS_GW_PIX][ZP], x [tap][FS_GW_PIX][XP], the embedding columns
// [FS_GW_PIX][48], zero where the tap or the pixel is outside: 35 840 bytes
// at CB = 2.
// ---------------------------------------------------------------------------
template <int S, int CB>
__global__ __launch_bounds__(FD_THREADS) void fs_gw_kernel(FsArgs a) {
    constexpr int OB = 4 / CB, OT = 16 * OB, CT = 16 * CB;
    constexpr int ZP = OT + 16, XP = CB == 1 ? 16 : 48, EP = 48;
    constexpr int QN = CT / 4;                      // float4 of a staged x row
    constexpr int XN = 9 * FS_GW_PIX * QN;          // and of a chunk
    constexpr int XV = (XN + FD_THREADS - 1) / FD_THREADS;
    constexpr int ZN = FS_GW_PIX * OT / 4;
    constexpr int EV = FS_GW_PIX * 32 / FD_THREADS;
    static_assert(ZN <= FD_THREADS, "one float4 of gz a thread");
    __shared__ __attribute__((aligned(16))) float zl[FS_GW_PIX * ZP];
    __shared__ __attribute__((aligned(16))) float xl[9 * FS_GW_PIX * XP];
    __shared__ float el[FS_GW_PIX * EP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, k = lane >> 4;
    const int ob = wave % OB, cb = wave / OB;
    const int CIN = a.C + 2;
    const int ctiles = a.C / CT, otiles = (a.O + OT - 1) / OT;
    const int tiles = ctiles * otiles;
    const int tile = (int)blockIdx.x % tiles, part = (int)blockIdx.x / tiles;
    const int c0 = (tile % ctiles) * CT, o0 = (tile / ctiles) * OT;
    const bool active = o0 + 16 * ob < a.O;         // (O = 32 under OT = 64)
    const bool with_embedding = c0 == 0 && cb == 0;

    dl_f4 acc[9], acce[2];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = dl_f4{0.f, 0.f, 0.f, 0.f};
    acce[0] = acce[1] = dl_f4{0.f, 0.f, 0.f, 0.f};

    float4 gr, yr, xr[XV];
    float er[EV];
    auto load = [&](int chunk) {
        gr = yr = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((int)threadIdx.x < ZN) {
            const int oq = threadIdx.x % (OT / 4), pix = threadIdx.x / (OT / 4);
            const long long n = (long long)chunk * FS_GW_PIX + pix;
            if (n < a.pixels && o0 + 4 * oq < a.O) {
                const long long at = n * a.O + o0 + 4 * oq;
                gr = *(const float4*)(a.g + at);
                yr = *(const float4*)(a.y + at);
            }
        }
        {
            // (the pixel of a thread is the same at every tap it stages)
            const int pix = ((int)threadIdx.x / QN) % FS_GW_PIX;
            const long long n = (long long)chunk * FS_GW_PIX + pix;
            const bool live = n < a.pixels;
            const DlBatchPixel px(live ? n : 0, a.Fo, a.T);
#pragma unroll
            for (int u = 0; u < XV; ++u) {
                const int idx = threadIdx.x + u * FD_THREADS;
                const int tap = idx / (QN * FS_GW_PIX);
                const int row = S * px.h - 1 + tap / 3;
                const int tt = px.w - 1 + tap % 3;
                xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live && idx < XN && row >= 0 && row < a.F && tt >= 0 &&
                    tt < a.T)
                    xr[u] = *(const float4*)(
                        a.x + (((long long)px.b * a.F + row) * a.T + tt) *
                        a.C + c0 + 4 * (idx % QN));
            }
        }
        if (c0 == 0) {
            // columns 2 tap + (sin | cos), then a column of ones
#pragma unroll
            for (int u = 0; u < EV; ++u) {
                const int idx = threadIdx.x + u * FD_THREADS;
                const int column = idx & 31, pix = idx >> 5;
                const long long n = (long long)chunk * FS_GW_PIX + pix;
                er[u] = 0.f;
                if (n < a.pixels && column < 18) {
                    const DlBatchPixel px(n, a.Fo, a.T);
                    const int tap = column >> 1;
                    const int row = S * px.h - 1 + tap / 3;
                    const int tt = px.w - 1 + tap % 3;
                    if (row >= 0 && row < a.F && tt >= 0 && tt < a.T)
                        er[u] = a.table[2 * row + (column & 1)];
                } else if (n < a.pixels && column == 18) {
                    er[u] = 1.f;
                }
            }
        }
    };

    const int first = part * a.per;
    const int last = first + a.per < a.chunks ? first + a.per : a.chunks;
    if (first < last) load(first);
    for (int chunk = first; chunk < last; ++chunk) {
        __syncthreads();
        if ((int)threadIdx.x < ZN)
            *(float4*)(zl + (threadIdx.x / (OT / 4)) * ZP +
                       4 * (threadIdx.x % (OT / 4))) =
                fs_gate4(gr, yr, a.act);
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int idx = threadIdx.x + u * FD_THREADS;
            if (idx < XN)
                *(float4*)(xl + (idx / QN) * XP + 4 * (idx % QN)) = xr[u];
        }
        if (c0 == 0)
#pragma unroll
            for (int u = 0; u < EV; ++u) {
                const int idx = threadIdx.x + u * FD_THREADS;
                el[(idx >> 5) * EP + (idx & 31)] = er[u];
            }
        __syncthreads();
        if (chunk + 1 < last) load(chunk + 1);
        if (!active) continue;
#pragma unroll
        for (int step = 0; step < FS_GW_PIX / 4; ++step) {
            const float gz = zl[(4 * step + k) * ZP + 16 * ob + i];
#pragma unroll
            for (int t = 0; t < 9; ++t)
                acc[t] = DL_MFMA(
                    gz, xl[(t * FS_GW_PIX + 4 * step + k) * XP + 16 * cb + i],
                    acc[t]);
            if (with_embedding) {
                acce[0] = DL_MFMA(gz, el[(4 * step + k) * EP + i], acce[0]);
                acce[1] =
                    DL_MFMA(gz, el[(4 * step + k) * EP + 16 + i], acce[1]);
            }
        }
    }
    if (!active) return;
    // rows o = o0 + 16 ob + 4 k + r, column c = c0 + 16 cb + i: every float of
    // the partial is written by exactly one thread
    const long long weights = (long long)a.O * CIN * 9;
    float* base = a.parts + (long long)part * (weights + a.O);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long o = o0 + 16 * ob + 4 * k + r;
#pragma unroll
        for (int t = 0; t < 9; ++t)
            base[(o * CIN + c0 + 16 * cb + i) * 9 + t] = acc[t][r];
        if (with_embedding) {
            // column i: the pair (tap i / 2, sin | cos); column 16 + i: the
            // last tap's pair, then the ones
            base[(o * CIN + a.C + (i & 1)) * 9 + (i >> 1)] = acce[0][r];
            if (i < 2) base[(o * CIN + a.C + i) * 9 + 8] = acce[1][r];
            if (i == 2) base[weights + o] = acce[1][r];
        }
    }
}

// ---------------------------------------------------------------------------
// The first layer, 1 -> 16 at stride s: x (B, F, T), W (16, 3, 3, 3) with the
// channels (x, sin, cos).
// ---------------------------------------------------------------------------
// forward: four output channels of a pixel a thread; W in LDS as
// [tap][x | sin | cos][16]
__global__ __launch_bounds__(FD_THREADS) void fs_first_conv_kernel(FsArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[27 * 16];
    for (int idx = threadIdx.x; idx < 432; idx += FD_THREADS) {
        const int o = idx / 27, which = idx % 27 / 9, tap = idx % 9;
        wl[(tap * 3 + which) * 16 + o] = a.w[idx];
    }
    __syncthreads();
    const long long idx = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (idx >= a.pixels * 4) return;
    const long long p = idx >> 2;
    const int q = (int)(idx & 3);
    const DlBatchPixel px(p, a.Fo, a.T);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kf = 0; kf < 3; ++kf) {
        const int row = a.s * px.h - 1 + kf;
        if (row < 0 || row >= a.F) continue;
        const float sin = a.table[2 * row], cos = a.table[2 * row + 1];
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int tt = px.w - 1 + kt;
            if (tt < 0 || tt >= a.T) continue;
            const float v = a.x[((long long)px.b * a.F + row) * a.T + tt];
            const float* w = wl + (kf * 3 + kt) * 48 + 4 * q;
            const float4 w0 = *(const float4*)w;
            const float4 w1 = *(const float4*)(w + 16);
            const float4 w2 = *(const float4*)(w + 32);
            acc.x = fmaf(w2.x, cos, fmaf(w1.x, sin, fmaf(w0.x, v, acc.x)));
            acc.y = fmaf(w2.y, cos, fmaf(w1.y, sin, fmaf(w0.y, v, acc.y)));
            acc.z = fmaf(w2.z, cos, fmaf(w1.z, sin, fmaf(w0.z, v, acc.z)));
            acc.w = fmaf(w2.w, cos, fmaf(w1.w, sin, fmaf(w0.w, v, acc.w)));
        }
    }
    const float4 bias = *(const float4*)(a.bias + 4 * q);
    *(float4*)(a.out + p * 16 + 4 * q) = make_float4(
        fd_activate(acc.x + bias.x, a.act), fd_activate(acc.y + bias.y, a.act),
        fd_activate(acc.z + bias.z, a.act), fd_activate(acc.w + bias.w, a.act));
}

// input gradient, one input pixel a thread: the taps kf with
// s fo + kf - 1 = f for an output row fo
__global__ __launch_bounds__(FD_THREADS) void fs_first_gx_kernel(FsArgs a) {
    const long long p = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (p >= a.pixels) return;
    const DlBatchPixel px(p, a.F, a.T);
    float acc = 0.f;
#pragma unroll
    for (int kf = 0; kf < 3; ++kf) {
        const int num = px.h + 1 - kf;
        if (num < 0 || num % a.s != 0 || num / a.s >= a.Fo) continue;
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int tt = px.w + 1 - kt;
            if (tt < 0 || tt >= a.T) continue;
            const long long at =
                (((long long)px.b * a.Fo + num / a.s) * a.T + tt) * 16;
            const int tap = kf * 3 + kt;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 gz =
                    fs_gate4(*(const float4*)(a.g + at + 4 * q),
                             *(const float4*)(a.y + at + 4 * q), a.act);
                acc = fmaf(a.w[(4 * q + 0) * 27 + tap], gz.x, acc);
                acc = fmaf(a.w[(4 * q + 1) * 27 + tap], gz.y, acc);
                acc = fmaf(a.w[(4 * q + 2) * 27 + tap], gz.z, acc);
                acc = fmaf(a.w[(4 * q + 3) * 27 + tap], gz.w, acc);
            }
        }
    }
    a.out[p] = acc;
}

// gW (16, 3, 3, 3) and gb: a workgroup takes `span` output pixels, thread
// (slice = tid / 16, o = tid % 16) every sixteenth of them in ascending order;
// the sixteen slices are added in order. One partial of 432 + 16 floats.
__global__ __launch_bounds__(FD_THREADS) void fs_first_gw_kernel(FsArgs a) {
    __shared__ float lds[16][28][16];
    const int o = threadIdx.x & 15, slice = threadIdx.x >> 4;
    const long long begin = (long long)blockIdx.x * a.span;
    const long long end =
        begin + a.span < a.pixels ? begin + a.span : a.pixels;
    float acc[28];
#pragma unroll
    for (int e = 0; e < 28; ++e) acc[e] = 0.f;
    for (long long p = begin + slice; p < end; p += 16) {
        const DlBatchPixel px(p, a.Fo, a.T);
        const float gz = fd_gate(a.g[p * 16 + o], a.y[p * 16 + o], a.act);
#pragma unroll
        for (int kf = 0; kf < 3; ++kf) {
            const int row = a.s * px.h - 1 + kf;
            const bool in_f = row >= 0 && row < a.F;
            const float sin = in_f ? a.table[2 * row] : 0.f;
            const float cos = in_f ? a.table[2 * row + 1] : 0.f;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
                const int tt = px.w - 1 + kt;
                const bool in = in_f && tt >= 0 && tt < a.T;
                const float v =
                    in ? a.x[((long long)px.b * a.F + row) * a.T + tt] : 0.f;
                const int tap = kf * 3 + kt;
                acc[tap] = fmaf(gz, v, acc[tap]);
                acc[9 + tap] = fmaf(gz, in ? sin : 0.f, acc[9 + tap]);
                acc[18 + tap] = fmaf(gz, in ? cos : 0.f, acc[18 + tap]);
            }
        }
        acc[27] += gz;
    }
#pragma unroll
    for (int e = 0; e < 28; ++e) lds[slice][e][o] = acc[e];
    __syncthreads();
    float* part = a.parts + (long long)blockIdx.x * 448;
    for (int idx = threadIdx.x; idx < 448; idx += FD_THREADS) {
        const int e = idx >> 4, oo = idx & 15;
        float sum = lds[0][e][oo];
        for (int s = 1; s < 16; ++s) sum += lds[s][e][oo];
        part[e < 27 ? oo * 27 + e : 432 + oo] = sum;
    }
}

// ---------------------------------------------------------------------------
// The last layer, C -> 1 at stride 1, C = 32 ... 256: W (1, C + 2, 3, 3), the
// nine taps of a channel in a run. Tap (kf, kt) of the pixel p is the pixel
// p + (kf - 1) T + (kt - 1) where it lies inside the map.
// ---------------------------------------------------------------------------
// forward: eight lanes a pixel, a lane the channels 4 l + 32 u ..., the lanes
// added by a butterfly in a fixed order; lane 0 adds the embedding
__global__ __launch_bounds__(FD_THREADS) void fs_last_conv_kernel(FsArgs a) {
    const long long idx = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    const long long p = idx >> 3;
    const int l = (int)(idx & 7);
    const bool live = p < a.pixels;
    const DlPixel px(live ? p : 0, a.F, a.T);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int c = 4 * l; c < a.C; c += 32) {
            float wv[36];
#pragma unroll
            for (int f = 0; f < 9; ++f) {
                const float4 w = *(const float4*)(a.w + 9 * c + 4 * f);
                wv[4 * f] = w.x; wv[4 * f + 1] = w.y;
                wv[4 * f + 2] = w.z; wv[4 * f + 3] = w.w;
            }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                if (fd_tap_f(px, tap, 1, a.F, a.T) < 0) continue;
                const float4 v = *(const float4*)(
                    a.x + (p + fd_tap_offset(tap, 1, a.T)) * a.C + c);
                acc.x = fmaf(wv[tap], v.x, acc.x);
                acc.y = fmaf(wv[9 + tap], v.y, acc.y);
                acc.z = fmaf(wv[18 + tap], v.z, acc.z);
                acc.w = fmaf(wv[27 + tap], v.w, acc.w);
            }
        }
    float sum = (acc.x + acc.y) + (acc.z + acc.w);
    if (live && l == 0)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ff = fd_tap_f(px, tap, 1, a.F, a.T);
            if (ff < 0) continue;
            sum = fmaf(a.w[a.C * 9 + tap], a.table[2 * ff], sum);
            sum = fmaf(a.w[(a.C + 1) * 9 + tap], a.table[2 * ff + 1], sum);
        }
#pragma unroll
    for (int step = 4; step > 0; step >>= 1) sum += __shfl_xor(sum, step, 64);
    if (live && l == 0) a.out[p] = fd_activate(sum + a.bias[0], a.act);
}

// input gradient: four input channels of a pixel a thread
__global__ __launch_bounds__(FD_THREADS) void fs_last_gx_kernel(FsArgs a) {
    const long long idx = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
    const int quads = a.C / 4;
    if (idx >= a.pixels * quads) return;
    const long long p = idx / quads;
    const int c = 4 * (int)(idx % quads);
    const DlPixel px(p, a.F, a.T);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (fd_tap_f(px, tap, 1, a.F, a.T, -1) < 0) continue;
        const long long at = p - fd_tap_offset(tap, 1, a.T);
        const float gz = fd_gate(a.g[at], a.y[at], a.act);
        acc.x = fmaf(a.w[(c + 0) * 9 + tap], gz, acc.x);
        acc.y = fmaf(a.w[(c + 1) * 9 + tap], gz, acc.y);
        acc.z = fmaf(a.w[(c + 2) * 9 + tap], gz, acc.z);
        acc.w = fmaf(a.w[(c + 3) * 9 + tap], gz, acc.w);
    }
    *(float4*)(a.out + p * a.C + c) = acc;
}

// gW (1, C + 2, 3, 3) and gb: a workgroup takes `span` pixels of the input,
// thread (slice, quad of channels) every 1024 / C-th of them in ascending
// order against gz at the nine mirrored taps; the quad-0 threads add the
// embedding rows and gb (the centre tap). The slices are added in order. One
// partial of (C + 2) 9 + 1 floats.
__global__ __launch_bounds__(FD_THREADS) void fs_last_gw_kernel(FsArgs a) {
    __shared__ float lds[FD_THREADS * 36];
    __shared__ float lde[32][19];
    const int quads = a.C / 4, slices = FD_THREADS / quads;
    const int quad = threadIdx.x % quads, slice = threadIdx.x / quads;
    const long long begin = (long long)blockIdx.x * a.span;
    const long long end =
        begin + a.span < a.pixels ? begin + a.span : a.pixels;
    float acc[4][9], emb[2][9], accb = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        acc[0][t] = acc[1][t] = acc[2][t] = acc[3][t] = 0.f;
        emb[0][t] = emb[1][t] = 0.f;
    }
    for (long long p = begin + slice; p < end; p += slices) {
        const DlPixel px(p, a.F, a.T);
        const float4 v = *(const float4*)(a.x + p * a.C + 4 * quad);
        const float sin = a.table[2 * px.h], cos = a.table[2 * px.h + 1];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            // (a tap that leaves the map adds nothing: no product of its zero
            // with x, which an infinite x would turn into a NaN)
            if (fd_tap_f(px, tap, 1, a.F, a.T, -1) < 0) continue;
            const long long at = p - fd_tap_offset(tap, 1, a.T);
            const float gz = fd_gate(a.g[at], a.y[at], a.act);
            acc[0][tap] = fmaf(gz, v.x, acc[0][tap]);
            acc[1][tap] = fmaf(gz, v.y, acc[1][tap]);
            acc[2][tap] = fmaf(gz, v.z, acc[2][tap]);
            acc[3][tap] = fmaf(gz, v.w, acc[3][tap]);
            if (quad == 0) {
                emb[0][tap] = fmaf(gz, sin, emb[0][tap]);
                emb[1][tap] = fmaf(gz, cos, emb[1][tap]);
                if (tap == 4) accb += gz;
            }
        }
    }
    // lds[slice][(4 quad + e) 9 + tap]
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 9; ++t)
            lds[slice * a.C * 9 + (4 * quad + e) * 9 + t] = acc[e][t];
    if (quad == 0) {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            lde[slice][t] = emb[0][t];
            lde[slice][9 + t] = emb[1][t];
        }
        lde[slice][18] = accb;
    }
    __syncthreads();
    float* part = a.parts + (long long)blockIdx.x * ((a.C + 2) * 9 + 1);
    for (int idx = threadIdx.x; idx < a.C * 9 + 19; idx += FD_THREADS) {
        float sum;
        if (idx < a.C * 9) {
            sum = lds[idx];
            for (int s = 1; s < slices; ++s) sum += lds[s * a.C * 9 + idx];
        } else {
            sum = lde[0][idx - a.C * 9];
            for (int s = 1; s < slices; ++s) sum += lde[s][idx - a.C * 9];
        }
        part[idx] = sum;
    }
}

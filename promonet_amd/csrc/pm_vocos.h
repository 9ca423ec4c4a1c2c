// Vocos mel vocoder kernels (promonet/model/vocos.py, config/baselines/vocos.py)
//
// Every activation between kernels is fp32 and CHANNELS-LAST: row r = b T + t
// of a (B T, C) matrix. The MFMA operand type ET (ElemF32 / ElemF16 /
// ElemBF16, pm_common.h) is used for the contractions only; LayerNorm
// statistics, the depthwise conv, the residual stream, the spectral head's
// exp / sin / cos and the inverse STFT are fp32.
//
// vocos_gemm_kernel   out = sum_tap x[t + tap - TAPS/2] W[:, :, tap] + bias
//                     (+ per-utterance bias): conv_pre + cond, embed, head.out
// vocos_ln_kernel     LayerNorm over the C channels of every row, in place
// vocos_block_kernel  one whole ConvNeXtBlock (vocos.py:113-146): depthwise
//                     k7 conv + LayerNorm into an LDS tile of MT rows, then
//                     for every 64-wide chunk of the H hidden channels
//                     h = GELU(xn W1c^T + b1c) (LDS only) and acc += h W2c^T;
//                     y = x + gamma (acc + b2). The (rows x H) hidden
//                     activation never leaves the workgroup.
// vocos_istft_frame_kernel  spectrum of one frame -> windowed inverse real FFT
//                     (1024 points as a 512-point complex FFT in LDS)
// vocos_ola_kernel    overlap-add of the 4 frames covering a sample, crop 384,
//                     divide by the overlap-added window^2 (vocos.py:175-206)
//
// RAGGED (a compile-time switch of every kernel that derives (b, t) from
// row / T): the rows are PACKED. Utterance b of lengths[b] frames owns rows
// [off[b], off[b + 1]) of R = off[B] rows; vocos_rowmap_kernel writes off and
// the per-row lookup VocosRow from the device array lengths. Grids are sized
// on the host from the bound B T and workgroups past R exit, so nothing reads
// lengths on the host. A row's arithmetic is that of the uniform kernels, in
// the same order: a ragged utterance equals its stand-alone synthesis bit
// for bit.
#pragma once
#include "pm_common.h"

#define PM_VOCOS_C 512
#define PM_VOCOS_NFFT 1024
#define PM_VOCOS_HOP 256
#define PM_VOCOS_BINS 513
#define PM_VOCOS_PAD 384
#define PM_VOCOS_HEAD_OUT (PM_VOCOS_NFFT + 2)
#define PM_VOCOS_HC 64                 // hidden channels per chunk
#define PM_VOCOS_GEMM_ROWS 64          // vocos_gemm_kernel tile: rows x cols
#define PM_VOCOS_GEMM_COLS 128

// One packed row of a ragged batch: utterance, frame within it, the
// utterance's length and its first row. 16 bytes, one load from global / L2.
struct __attribute__((aligned(16))) VocosRow {
    int b, t, len, off;
};

// Packed-row lookup of the RAGGED instantiations (both null when uniform)
struct VocosRagged {
    const VocosRow* map;  // (R) valid rows only
    const int* off;       // (B + 1) first row of every utterance; off[B] = R
};

// MT rows of the ConvNeXt tile: 128 for the 16-bit types (xn tile 130 KiB),
// 64 for fp32 (the same bytes)
template <class ET> struct VocosTile {
    static constexpr int MT = ET::ESZ == 2 ? 128 : 64;
    static constexpr int THREADS = MT * 4;
    static constexpr int SX = PM_VOCOS_C * ET::ESZ + 16;
    static constexpr int SH = PM_VOCOS_HC * ET::ESZ + 16;
    static constexpr int SMEM = MT * (SX + SH);
};

__device__ __forceinline__ float vc_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// 8 fp32 values -> one MFMA fragment (lane's 8 consecutive k)
template <class ET>
__device__ __forceinline__ typename ET::frag_t vc_frag(float4 lo, float4 hi) {
    typename ET::frag_t f;
    if constexpr (ET::ESZ == 4) {
        f.lo = lo;
        f.hi = hi;
    } else {
        f[0] = ET::cvt(lo.x); f[1] = ET::cvt(lo.y);
        f[2] = ET::cvt(lo.z); f[3] = ET::cvt(lo.w);
        f[4] = ET::cvt(hi.x); f[5] = ET::cvt(hi.y);
        f[6] = ET::cvt(hi.z); f[7] = ET::cvt(hi.w);
    }
    return f;
}

template <class ET>
__device__ __forceinline__ typename ET::frag_t vc_load(const void* p) {
    return *reinterpret_cast<const typename ET::frag_t*>(p);
}

// row of the 32 x 32 accumulator tile held in element r of lane (ln, lh)
__device__ __forceinline__ int vc_acc_row(int r, int lh) {
    return (r >> 2) * 8 + lh * 4 + (r & 3);
}

// exact-erf GELU (torch.nn.GELU(), approximate='none')
__device__ __forceinline__ float vc_gelu(float v) {
    return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
}

// ---------------------------------------------------------------------------
// packing (finalize): fp32 (N, K, taps) -> ET [Np][taps][K], rows >= N zero
// ---------------------------------------------------------------------------
template <class ET>
__global__ __launch_bounds__(256) void vocos_pack_kernel(
    const float* w, void* out, int N, int Np, int K, int taps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)Np * taps * K;
    if (i >= total) return;
    const int k = (int)(i % K);
    const int tap = (int)((i / K) % taps);
    const int n = (int)(i / ((long long)K * taps));
    const float v = n < N ? w[((long long)n * K + k) * taps + tap] : 0.f;
    ET::pack_store(out, i, v);
}

// depthwise weights (C, 1, 7) -> [7][C]
__global__ __launch_bounds__(256) void vocos_dw_pack_kernel(
    const float* w, float* out, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 7 * C) return;
    out[i] = w[(i % C) * 7 + i / C];
}

// ragged prologue: lengths (B) -> off (B + 1) and the row map. Workgroup
// (x, b) sums the lengths before b itself (B is small, the loads are scalar)
// and fills 256 rows of utterance b. A length is clamped to [0, T]: R never
// exceeds the B T rows the workspace holds, whatever lengths contains.
__global__ __launch_bounds__(256) void vocos_rowmap_kernel(
    const int* lengths, int* off, VocosRow* map, int B, int T) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    int first = 0;
    for (int i = 0; i < b; ++i) first += min(max(lengths[i], 0), T);
    const int len = min(max(lengths[b], 0), T);
    if (t == 0) {
        off[b] = first;
        if (b == B - 1) off[B] = first + len;
    }
    if (t < len) {
        VocosRow r;
        r.b = b; r.t = t; r.len = len; r.off = first;
        map[first + t] = r;
    }
}

// cond: gb (Bg, N) = W (N, G) g (Bg, G) + b          vocos.py:47-49
__global__ __launch_bounds__(256) void vocos_cond_kernel(
    const float* g, const float* w, const float* b, float* out, int G, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y;
    if (n >= N) return;
    const float* gr = g + (size_t)row * G;
    const float* wr = w + (size_t)n * G;
    float acc = 0.f;
    for (int k = 0; k < G; ++k) acc = fmaf(wr[k], gr[k], acc);
    out[(size_t)row * N + n] = acc + b[n];
}

// ---------------------------------------------------------------------------
// conv / linear: 64 rows x 128 columns a workgroup, 4 waves of 32 x 64
// ---------------------------------------------------------------------------
struct VocosGemmArgs {
    const float* x;       // (B, T, K) channels-last, or (B, K, T) when CF
    const void* w;        // ET [Np][TAPS][K], Np a multiple of 128
    const float* bias;    // (N)
    const float* gbias;   // (gbatch, N) added after the bias, or null
    int gbatch;
    float* out;           // (B T, ldo)
    int B, T, K, N, ldo;
    VocosRagged rg;       // RAGGED: x (CF: padded (B, K, T)) and out packed
};

template <class ET, int TAPS, bool CF, bool RAGGED>
__global__ __launch_bounds__(256) void vocos_gemm_kernel(VocosGemmArgs a) {
    typedef typename ET::lds_t et;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ln = lane & 31, lh = lane >> 5;
    const int rows = RAGGED ? a.rg.off[a.B] : a.B * a.T;
    const int r0 = blockIdx.x * PM_VOCOS_GEMM_ROWS + (wave >> 1) * 32;
    const int n0 = blockIdx.y * PM_VOCOS_GEMM_COLS + (wave & 1) * 64;
    if (r0 >= rows) return;                 // (no barrier in this kernel)
    const int row = r0 + ln;
    const bool live = row < rows;
    int b, t, len, first;                   // first: row of the utterance's t = 0
    if constexpr (RAGGED) {
        VocosRow m = {0, 0, 0, 0};
        if (live) m = a.rg.map[row];
        b = m.b; t = m.t; len = m.len; first = m.off;
    } else {
        b = live ? row / a.T : 0;
        t = live ? row - b * a.T : 0;
        len = a.T;
        first = b * a.T;
    }

    floatx16 acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    const et* w = reinterpret_cast<const et*>(a.w);
    const et* w0 = w + (size_t)(n0 + ln) * TAPS * a.K + lh * 8;
    const et* w1 = w0 + (size_t)32 * TAPS * a.K;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap) {
        const int ts = t + tap - TAPS / 2;
        const bool ok = live && ts >= 0 && ts < len;
        const float* xr = CF
            ? a.x + (size_t)b * a.K * a.T + (ok ? ts : 0) + (size_t)lh * 8 * a.T
            : a.x + ((size_t)first + (ok ? ts : 0)) * a.K + lh * 8;
        const et* wt0 = w0 + (size_t)tap * a.K;
        const et* wt1 = w1 + (size_t)tap * a.K;
#pragma unroll 1
        for (int k0 = 0; k0 < a.K; k0 += 16) {
            float4 lo = zero, hi = zero;
            if (ok) {
                if constexpr (CF) {
                    const float* p = xr + (size_t)k0 * a.T;
                    const size_t s = a.T;
                    lo = make_float4(p[0], p[s], p[2 * s], p[3 * s]);
                    hi = make_float4(p[4 * s], p[5 * s], p[6 * s], p[7 * s]);
                } else {
                    lo = *reinterpret_cast<const float4*>(xr + k0);
                    hi = *reinterpret_cast<const float4*>(xr + k0 + 4);
                }
            }
            const typename ET::frag_t av = vc_frag<ET>(lo, hi);
            ET::mma(av, vc_load<ET>(wt0 + k0), acc[0]);
            ET::mma(av, vc_load<ET>(wt1 + k0), acc[1]);
        }
    }

#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = n0 + nt * 32 + ln;
        if (n >= a.N) continue;
        const float bias = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = r0 + vc_acc_row(r, lh);
            if (rr >= rows) continue;
            float v = acc[nt][r] + bias;
            if (a.gbias) {
                int gb = 0;
                if (a.gbatch != 1) {
                    if constexpr (RAGGED) gb = a.rg.map[rr].b;
                    else gb = rr / a.T;
                }
                v += a.gbias[(size_t)gb * a.N + n];
            }
            a.out[(size_t)rr * a.ldo + n] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// LayerNorm over C = 512 channels (eps 1e-6): one wave a row, 8 channels a lane
// ---------------------------------------------------------------------------
__device__ __forceinline__ void vc_layer_norm8(
    float (&v)[8], const float* g, const float* beta, int c0) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
    const float mean = vc_wave_sum(s) * (1.f / PM_VOCOS_C);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] -= mean;
        q = fmaf(v[e], v[e], q);
    }
    const float var = vc_wave_sum(q) * (1.f / PM_VOCOS_C);
    const float rstd = 1.f / sqrtf(var + 1e-6f);
    const float4 g0 = *reinterpret_cast<const float4*>(g + c0);
    const float4 g1 = *reinterpret_cast<const float4*>(g + c0 + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(beta + c0);
    const float4 b1 = *reinterpret_cast<const float4*>(beta + c0 + 4);
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] * rstd * gg[e] + bb[e];
}

// (rows: the host's bound B T; RAGGED reads the packed row count off[B])
template <bool RAGGED>
__global__ __launch_bounds__(256) void vocos_ln_kernel(
    float* x, const float* g, const float* beta, int rows, const int* total) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if constexpr (RAGGED) rows = *total;
    if (row >= rows) return;
    float* p = x + (size_t)row * PM_VOCOS_C + lane * 8;
    const float4 lo = *reinterpret_cast<const float4*>(p);
    const float4 hi = *reinterpret_cast<const float4*>(p + 4);
    float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    vc_layer_norm8(v, g, beta, lane * 8);
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ---------------------------------------------------------------------------
// ConvNeXt block
// ---------------------------------------------------------------------------
struct VocosBlockArgs {
    const float* x;       // (B T, 512) residual stream in
    float* y;             // (B T, 512) out (a different buffer: the conv
                          // reads its neighbours' rows)
    const float* dw_w;    // [7][512]
    const float* dw_b;
    const float* ln_w;
    const float* ln_b;
    const void* w1;       // ET (H, 512)
    const float* b1;      // (H)
    const void* w2;       // ET (512, H)
    const float* b2;
    const float* gamma;
    int B, T, H;
    VocosRagged rg;       // RAGGED: x and y packed
};

template <class ET, bool RAGGED>
__global__ __launch_bounds__(VocosTile<ET>::THREADS) void vocos_block_kernel(
    VocosBlockArgs a) {
    typedef VocosTile<ET> Tile;
    typedef typename ET::lds_t et;
    typedef typename ET::frag_t frag_t;
    constexpr int C = PM_VOCOS_C, MT = Tile::MT, NW = MT / 16;
    constexpr int SX = Tile::SX, SH = Tile::SH, ESZ = ET::ESZ;
    constexpr int MTW = MT / 32;          // second GEMM: M tiles a wave
    constexpr int NTW = 8 / MTW;          // ... and N tiles: 8 accumulators
    static_assert(NW * NTW * 32 == C, "waves cover the channels");
    static_assert((MT / 32) * 2 == NW, "one hidden tile a wave");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* xs = smem;
    char* hs = smem + MT * SX;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ln = lane & 31, lh = lane >> 5;
    const int rows = RAGGED ? a.rg.off[a.B] : a.B * a.T;
    const int m0 = blockIdx.x * MT;
    if constexpr (RAGGED)
        if (m0 >= rows) return;           // the whole workgroup, before a barrier

    // depthwise k7 conv (zero padding at each utterance's ends) + LayerNorm
    for (int i = wave; i < MT; i += NW) {
        const int row = m0 + i;
        char* dst = xs + i * SX + lane * 8 * ESZ;
        float v[8];
        if (row < rows) {
            int t, len;                   // (a tile may hold several ends)
            if constexpr (RAGGED) {
                const VocosRow m = a.rg.map[row];
                t = m.t;
                len = m.len;
            } else {
                t = row % a.T;
                len = a.T;
            }
            const float4 d0 = *reinterpret_cast<const float4*>(a.dw_b + lane * 8);
            const float4 d1 =
                *reinterpret_cast<const float4*>(a.dw_b + lane * 8 + 4);
            float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 7; ++tap) {
                const int ts = t + tap - 3;
                if (ts < 0 || ts >= len) continue;
                const float* src = a.x + (size_t)(row + tap - 3) * C + lane * 8;
                const float* wt = a.dw_w + tap * C + lane * 8;
                const float4 x0 = *reinterpret_cast<const float4*>(src);
                const float4 x1 = *reinterpret_cast<const float4*>(src + 4);
                const float4 w0 = *reinterpret_cast<const float4*>(wt);
                const float4 w1 = *reinterpret_cast<const float4*>(wt + 4);
                s[0] = fmaf(x0.x, w0.x, s[0]); s[1] = fmaf(x0.y, w0.y, s[1]);
                s[2] = fmaf(x0.z, w0.z, s[2]); s[3] = fmaf(x0.w, w0.w, s[3]);
                s[4] = fmaf(x1.x, w1.x, s[4]); s[5] = fmaf(x1.y, w1.y, s[5]);
                s[6] = fmaf(x1.z, w1.z, s[6]); s[7] = fmaf(x1.w, w1.w, s[7]);
            }
            v[0] = s[0] + d0.x; v[1] = s[1] + d0.y;
            v[2] = s[2] + d0.z; v[3] = s[3] + d0.w;
            v[4] = s[4] + d1.x; v[5] = s[5] + d1.y;
            v[6] = s[6] + d1.z; v[7] = s[7] + d1.w;
            vc_layer_norm8(v, a.ln_w, a.ln_b, lane * 8);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
        *reinterpret_cast<frag_t*>(dst) = vc_frag<ET>(
            make_float4(v[0], v[1], v[2], v[3]),
            make_float4(v[4], v[5], v[6], v[7]));
    }
    __syncthreads();

    floatx16 acc[MTW * NTW];
#pragma unroll
    for (int j = 0; j < MTW * NTW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int mi = wave >> 1, ni = wave & 1;      // this wave's hidden tile
    const int c0 = wave * NTW * 32;               // this wave's output columns
    const et* w1 = reinterpret_cast<const et*>(a.w1);
    const et* w2 = reinterpret_cast<const et*>(a.w2);
    const char* arow = xs + (mi * 32 + ln) * SX + lh * 8 * ESZ;

#pragma unroll 1
    for (int hc = 0; hc < a.H; hc += PM_VOCOS_HC) {
        // h = GELU(xn W1[chunk]^T + b1[chunk]) -> LDS
        floatx16 c1;
#pragma unroll
        for (int r = 0; r < 16; ++r) c1[r] = 0.f;
        const et* w1p = w1 + (size_t)(hc + ni * 32 + ln) * C + lh * 8;
#pragma unroll 8
        for (int k0 = 0; k0 < C; k0 += 16)
            ET::mma(vc_load<ET>(arow + k0 * ESZ), vc_load<ET>(w1p + k0), c1);
        const int j = ni * 32 + ln;
        const float bias = a.b1[hc + j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = mi * 32 + vc_acc_row(r, lh);
            *reinterpret_cast<et*>(hs + i * SH + j * ESZ) =
                ET::cvt(vc_gelu(c1[r] + bias));
        }
        __syncthreads();

        // acc += h W2[:, chunk]^T
#pragma unroll
        for (int kk = 0; kk < PM_VOCOS_HC; kk += 16) {
            frag_t av[MTW];
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt)
                av[mt] = vc_load<ET>(
                    hs + (mt * 32 + ln) * SH + (kk + lh * 8) * ESZ);
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const frag_t bv = vc_load<ET>(
                    w2 + (size_t)(c0 + nt * 32 + ln) * a.H + hc + kk + lh * 8);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt)
                    ET::mma(av[mt], bv, acc[mt * NTW + nt]);
            }
        }
        __syncthreads();
    }

    // y = x + gamma (acc + b2)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int c = c0 + nt * 32 + ln;
        const float bias = a.b2[c], gamma = a.gamma[c];
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + mt * 32 + vc_acc_row(r, lh);
                if (row >= rows) continue;
                const size_t at = (size_t)row * C + c;
                a.y[at] = a.x[at] + gamma * (acc[mt * NTW + nt][r] + bias);
            }
    }
}

// ---------------------------------------------------------------------------
// inverse STFT
// ---------------------------------------------------------------------------
struct VocosIstftArgs {
    const float* spec;    // MODE 0: head logits (B T, 1026): log-magnitude
                          // [0, 513) | phase [513, 1026)   (vocos.py:163-169)
                          // MODE 1: complex spectrum (B, 513, T) as (re, im)
    const float* window;  // (1024) the loaded head.istft.window
    float* frames;        // (B T, 1024) windowed irfft of every frame
    int B, T;
    const int* total;     // RAGGED: the packed row count off[B]
};

__device__ __forceinline__ unsigned vc_bitrev9(unsigned v) {
    return __builtin_bitreverse32(v) >> 23;
}

// One workgroup = one frame. The 513 bins X fold into 512 complex points
// Z[k] = E[k] + i O[k], E = (X[k] + conj X[512 - k]) / 2,
// O = (X[k] - conj X[512 - k]) e^{+2 pi i k / 1024} / 2, whose 512-point
// inverse DFT z[n] is x[2n] + i x[2n + 1] (the mirror of pm_fft.h's forward
// packing). The imaginary parts of bins 0 and 512 are dropped, as the C2R
// irfft does.
template <int MODE, bool RAGGED>
__global__ __launch_bounds__(256) void vocos_istft_frame_kernel(
    VocosIstftArgs a) {
    static_assert(MODE == 0 || !RAGGED, "the (B, 513, T) spectrum is uniform");
    __shared__ float2 z[512];
    __shared__ float2 tw[512];          // e^{+2 pi i j / 512}
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    if constexpr (RAGGED)
        if (row >= *a.total) return;    // the whole workgroup, before a barrier
    const int b = row / a.T, t = row - b * a.T;

    auto bin = [&](int k) -> float2 {
        float re, im;
        if constexpr (MODE == 0) {
            const float* l = a.spec + (size_t)row * PM_VOCOS_HEAD_OUT;
            float mag = expf(l[k]);
            mag = mag > 100.f ? 100.f : mag;     // torch.clip: NaN stays NaN
            float s, c;
            sincosf(l[PM_VOCOS_BINS + k], &s, &c);
            re = mag * c;
            im = mag * s;
        } else {
            const float* p =
                a.spec + (((size_t)b * PM_VOCOS_BINS + k) * a.T + t) * 2;
            re = p[0];
            im = p[1];
        }
        if (k == 0 || k == PM_VOCOS_BINS - 1) im = 0.f;
        return make_float2(re, im);
    };

#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = tid + h * 256;
        float s, c;
        sincospif((float)j * (1.f / 256.f), &s, &c);
        tw[j] = make_float2(c, s);
        const float2 xk = bin(j), xm = bin(512 - j);
        const float er = 0.5f * (xk.x + xm.x), ei = 0.5f * (xk.y - xm.y);
        const float dr = 0.5f * (xk.x - xm.x), di = 0.5f * (xk.y + xm.y);
        sincospif((float)j * (1.f / 512.f), &s, &c);
        const float orr = dr * c - di * s, oi = dr * s + di * c;
        z[vc_bitrev9(j)] = make_float2(er - oi, ei + orr);
    }
    __syncthreads();

    // radix-2 decimation in time, positive exponent (inverse transform)
#pragma unroll 1
    for (int half = 1; half < 512; half <<= 1) {
        const int m = tid & (half - 1);
        const int i0 = (tid - m) * 2 + m, i1 = i0 + half;
        const float2 w = tw[m * (256 / half)];
        const float2 u = z[i0], v = z[i1];
        const float vr = v.x * w.x - v.y * w.y, vi = v.x * w.y + v.y * w.x;
        z[i0] = make_float2(u.x + vr, u.y + vi);
        z[i1] = make_float2(u.x - vr, u.y - vi);
        __syncthreads();
    }

    float* out = a.frames + (size_t)row * PM_VOCOS_NFFT;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = tid + h * 256;
        const float2 v = z[n];
        const float2 w = *reinterpret_cast<const float2*>(a.window + 2 * n);
        *reinterpret_cast<float2*>(out + 2 * n) =
            make_float2(v.x * (1.f / 512.f) * w.x, v.y * (1.f / 512.f) * w.y);
    }
}

// audio (B, 256 T): sample n sits at n + 384 of the uncropped overlap-add;
// frames are summed in increasing order (as torch fold does), then divided by
// the window^2 envelope summed the same way. No atomics.
// RAGGED: the frames of utterance b are its len packed rows from off[b]; its
// last frame is len - 1, so the envelope is that of the frames that exist,
// and the samples from 256 len up to the padded 256 T are exact zeros.
template <bool RAGGED>
__global__ __launch_bounds__(256) void vocos_ola_kernel(
    const float* frames, const float* window, float* audio, int T,
    const int* off) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= T * PM_VOCOS_HOP) return;
    int first = b * T, len = T;
    if constexpr (RAGGED) {
        first = off[b];
        len = off[b + 1] - first;
        if (n >= len * PM_VOCOS_HOP) {
            audio[(size_t)b * T * PM_VOCOS_HOP + n] = 0.f;
            return;
        }
    }
    const int p = n + PM_VOCOS_PAD;
    const int hi = min(p / PM_VOCOS_HOP, len - 1);
    const int lo = max(0, (p - PM_VOCOS_NFFT + PM_VOCOS_HOP) / PM_VOCOS_HOP);
    float y = 0.f, env = 0.f;
    for (int f = lo; f <= hi; ++f) {
        const int i = p - f * PM_VOCOS_HOP;
        y += frames[((size_t)first + f) * PM_VOCOS_NFFT + i];
        const float w = window[i];
        env += w * w;
    }
    audio[(size_t)b * T * PM_VOCOS_HOP + n] = y / env;
}

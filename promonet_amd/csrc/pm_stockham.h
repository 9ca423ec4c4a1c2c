// The short-time transform of the spectral-convergence loss (pm_loss.h) and of
// the discriminator spectrograms (pm_disc_spec.h), stated once: the plan, the
// loader and the FFT.
//
// A frame of N real points (N = 2^a or 5 2^a, 64 <= N <= 2560) is the complex
// transform of M = N / 2 points z[m] = v[2m] + i v[2m+1] and the split
// X[k] = E[k] + W^k O[k],  E = (Z[k] + conj Z[M-k]) / 2,
// O = -i (Z[k] - conj Z[M-k]) / 2,  W = exp(-2 pi i / N),  0 <= k <= M.
// The M-point transform is a Stockham autosort FFT between two LDS buffers:
// one radix-5 stage for the 5 2^a sizes, then radix-4 stages and at most one
// radix-2 stage. A workgroup carries `fpg` frames of one row at once (and, for
// the loss, the same frames of the target), and the butterflies of all of them
// are dealt to the 256 threads as one pool: at N = 64 a workgroup holds 32
// frames, at N = 2560 one. Twiddles come from one table W^m, m < N, rounded
// from float64 on the host.
//
// A row is reflect padded by `pad` samples on each side, pad < T, and frame f
// begins at padded sample f hop: frames = 1 + (T + 2 pad - N) / hop. The
// centred transform of the loss is pad = N / 2, frames = 1 + T / hop.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_host.h"

#define SC_THREADS 256
#define SC_MAX_STAGES 8
#define SC_MAX_POINTS 1280          // complex points of a workgroup's pool

struct ScPlan {
    int N, M, hop, pad, frames, T, fpg, groups; // groups: workgroups per row
    int stages;
    int radix[SC_MAX_STAGES];
};

// The radix plan of a size and the split of a row's frames over workgroups:
// 5 first where N = 5 2^a, then 4s, then one 2 where a power of 4 does not
// finish. Returns NULL, or what is wrong with the sizes. The grids it checks
// are those of a launch over the workgroups and of one over the samples.
inline const char* sc_make_plan(int batch, int samples, int fft_size,
                                int hop_size, int pad, ScPlan* p) {
    if (batch < 1) return "batch must be at least 1";
    if (fft_size < 64 || fft_size > 2560)
        return "fft_size must be between 64 and 2560";
    int rest = fft_size;
    if (rest % 5 == 0) rest /= 5;
    if (rest & (rest - 1)) return "fft_size must be 2^a or 5 * 2^a";
    if (hop_size < 1 || hop_size > fft_size)
        return "hop_size must be between 1 and fft_size";
    if (pad < 0 || pad > fft_size) return "pad must be between 0 and fft_size";
    if (samples <= pad)
        return "the row must be longer than its margin (reflect padding)";
    if (samples > (1 << 30)) return "the row must not exceed 2^30 samples";
    if (samples + 2 * pad < fft_size)
        return "the padded row is shorter than one frame";
    p->N = fft_size;
    p->M = fft_size / 2;
    p->hop = hop_size;
    p->pad = pad;
    p->T = samples;
    p->frames = 1 + (samples + 2 * pad - fft_size) / hop_size;
    p->fpg = SC_MAX_POINTS / p->M;
    if (p->fpg > p->frames) p->fpg = p->frames;
    p->groups = (p->frames + p->fpg - 1) / p->fpg;
    p->stages = 0;
    int m = p->M;
    if (m % 5 == 0) { p->radix[p->stages++] = 5; m /= 5; }
    while (m % 4 == 0) { p->radix[p->stages++] = 4; m /= 4; }
    if (m == 2) p->radix[p->stages++] = 2;
    if ((long long)batch * p->groups > PM_MAX_GRID ||
        ((long long)batch * samples + SC_THREADS - 1) / SC_THREADS >
            PM_MAX_GRID)
        return "too many frames or samples for one launch";
    return nullptr;
}

__device__ __forceinline__ float2 sc_mul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// One Stockham stage of radix R over `slots` transforms of M points that lie
// back to back in `in`; Ns is the product of the radices already done.
template <int R>
__device__ __forceinline__ void sc_stage(const float2* __restrict__ in,
                                         float2* __restrict__ out,
                                         const float2* __restrict__ tw,
                                         int slots, int M, int Ns) {
    const int per = M / R;                  // butterflies of one transform
    const int step = M / (Ns * R);          // W_M^(k step) = W_(Ns R)^k
    const int total = slots * per;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        const int slot = i / per, j = i - slot * per;
        const int k = j % Ns;
        const float2* __restrict__ src = in + slot * M;
        float2 v[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            v[q] = src[j + q * per];
            // (the table has N = 2 M entries: W_M^m is entry 2 m)
            if (q) v[q] = sc_mul(v[q], tw[2 * (q * k * step)]);
        }
        float2 o[R];
        if (R == 2) {
            o[0] = make_float2(v[0].x + v[1].x, v[0].y + v[1].y);
            o[1] = make_float2(v[0].x - v[1].x, v[0].y - v[1].y);
        } else if (R == 4) {
            const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
            const float2 a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
            const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
            // -i (v1 - v3)
            const float2 a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);
            o[0] = make_float2(a0.x + a2.x, a0.y + a2.y);
            o[1] = make_float2(a1.x + a3.x, a1.y + a3.y);
            o[2] = make_float2(a0.x - a2.x, a0.y - a2.y);
            o[3] = make_float2(a1.x - a3.x, a1.y - a3.y);
        } else {
            const float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;
            const float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
            const float2 t1 = make_float2(v[1].x + v[4].x, v[1].y + v[4].y);
            const float2 t2 = make_float2(v[2].x + v[3].x, v[2].y + v[3].y);
            const float2 t3 = make_float2(v[1].x - v[4].x, v[1].y - v[4].y);
            const float2 t4 = make_float2(v[2].x - v[3].x, v[2].y - v[3].y);
            o[0] = make_float2(v[0].x + t1.x + t2.x, v[0].y + t1.y + t2.y);
            const float2 m1 = make_float2(v[0].x + c1 * t1.x + c2 * t2.x,
                                          v[0].y + c1 * t1.y + c2 * t2.y);
            const float2 m2 = make_float2(v[0].x + c2 * t1.x + c1 * t2.x,
                                          v[0].y + c2 * t1.y + c1 * t2.y);
            const float2 n1 = make_float2(s1 * t3.x + s2 * t4.x,
                                          s1 * t3.y + s2 * t4.y);
            const float2 n2 = make_float2(s2 * t3.x - s1 * t4.x,
                                          s2 * t3.y - s1 * t4.y);
            // X1 = m1 - i n1, X4 = m1 + i n1, X2 = m2 - i n2, X3 = m2 + i n2
            o[1] = make_float2(m1.x + n1.y, m1.y - n1.x);
            o[4] = make_float2(m1.x - n1.y, m1.y + n1.x);
            o[2] = make_float2(m2.x + n2.y, m2.y - n2.x);
            o[3] = make_float2(m2.x - n2.y, m2.y + n2.x);
        }
        float2* __restrict__ dst = out + slot * M + (j / Ns) * Ns * R + k;
#pragma unroll
        for (int q = 0; q < R; ++q) dst[q * Ns] = o[q];
    }
}

// Every stage of the plan over the pool; returns the buffer the result is in.
// Every thread of the workgroup must call it (it holds barriers).
__device__ __forceinline__ float2* sc_fft(float2* a, float2* b,
                                          const float2* __restrict__ tw,
                                          const ScPlan& p, int slots) {
    int Ns = 1;
    __syncthreads();
    for (int s = 0; s < p.stages; ++s) {
        const int r = p.radix[s];
        if (r == 5) sc_stage<5>(a, b, tw, slots, p.M, Ns);
        else if (r == 4) sc_stage<4>(a, b, tw, slots, p.M, Ns);
        else sc_stage<2>(a, b, tw, slots, p.M, Ns);
        Ns *= r;
        __syncthreads();
        float2* t = a; a = b; b = t;
    }
    return a;
}

// Frames [f0, f0 + count) of one row, windowed, reflect padded and packed
// into `count` transforms of M complex points. Frame f begins at padded
// sample f hop, which is sample f hop - pad.
__device__ __forceinline__ void sc_load(float2* __restrict__ dst,
                                        const float* __restrict__ x,
                                        const float* __restrict__ window,
                                        const ScPlan& p, int f0, int count) {
    const int total = count * p.M;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        const int fl = i / p.M, m = i - fl * p.M;
        const int start = (f0 + fl) * p.hop - p.pad;
        float pair[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int n = start + 2 * m + h;
            if (n < 0) n = -n;
            if (n >= p.T) n = 2 * (p.T - 1) - n;
            // (T > pad: one reflection reaches every sample; the clamp only
            // keeps a caller's mistake inside the row)
            n = n < 0 ? 0 : (n >= p.T ? p.T - 1 : n);
            pair[h] = x[n] * window[2 * m + h];
        }
        dst[i] = make_float2(pair[0], pair[1]);
    }
}

// Bin k (0 <= k <= M) of a real frame from its packed transform Z.
__device__ __forceinline__ float2 sc_bin(const float2* __restrict__ Z,
                                         const float2* __restrict__ tw,
                                         int M, int k) {
    const float2 zk = Z[k == M ? 0 : k];
    const float2 zc = Z[k == 0 ? 0 : M - k];
    const float er = .5f * (zk.x + zc.x), ei = .5f * (zk.y - zc.y);
    const float orr = .5f * (zk.y + zc.y), oi = -.5f * (zk.x - zc.x);
    float2 w = make_float2(-1.f, 0.f);                  // W^M
    if (k < M) w = tw[k];
    return make_float2(er + (orr * w.x - oi * w.y),
                       ei + (orr * w.y + oi * w.x));
}

// Sum over the workgroup, in a fixed order; the result is valid in thread 0.
__device__ __forceinline__ float sc_block_sum(float v, float* scratch) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float total = scratch[0];
    for (int w = 1; w < SC_THREADS / 64; ++w) total += scratch[w];
    return total;
}

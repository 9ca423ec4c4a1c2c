// Training-side losses of the FARGAN configurations (promonet/train/loss.py):
// the spectral-convergence loss (:61-150) as a centred STFT, its bin gradient
// and the adjoint of the STFT, and the waveform `signal` loss (:158-162).
//
// The transform, its plan and its loader are pm_stockham.h's, centred:
// pad = N / 2. The adjoint pair below takes the margin from the plan, so the
// discriminator spectrograms (pm_disc_spec.hip) launch it too.
//
// Nothing here uses a float atomic: sums go through per-workgroup partials and
// one final pass, overlap-add is in gather form, so every output is the same
// bits on every run.
//
// NON-FINITE VALUES. This header promises torch's semantics on inf and NaN
// (DESIGN section 27): sqrt(clamp(|X|, min=1e-7)) of a NaN bin is NaN, and so
// are its bin gradient, the two sums and the loss. The object is built with
// -fhonor-nans (Makefile), or the test of a NaN folds.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_nonfinite.h"
#include "pm_stockham.h"

#define SC_FLOOR 1e-7f              // torch.clamp(magnitude, min=1e-7)

struct ScForwardArgs {
    const float* x;         // (B, T)
    const float* y;         // (B, T) target, PAIR kernels only
    const float* window;    // (N), already padded to N
    const float* twiddle;   // (N, 2): cos, -sin of 2 pi m / N
    const float* upstream;  // (B, bins, frames) or NULL: d loss / d s instead
                            // of -sign(s_y - s_x) as the factor of G
    float* s;               // (B, bins, frames) or NULL
    float* G;               // (B, bins, frames, 2) or NULL
    float* partials;        // (workgroups, 2) or NULL
    ScPlan p;
};

// pm_sc_stft (PAIR = false: s of x, or G from an upstream gradient) and
// pm_sc_forward (PAIR = true: the two sums and G). LDS: two buffers of
// slots * M complex points, slots = fpg or 2 fpg.
template <bool PAIR>
__global__ __launch_bounds__(SC_THREADS) void sc_forward_kernel(
    ScForwardArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 sc_lds[];
    __shared__ float scratch[SC_THREADS / 64];
    const ScPlan& p = a.p;
    const int row = blockIdx.x / p.groups;
    const int f0 = (blockIdx.x - row * p.groups) * p.fpg;
    const int count = p.frames - f0 < p.fpg ? p.frames - f0 : p.fpg;
    const int slots = PAIR ? 2 * count : count;
    float2* buf0 = sc_lds;
    float2* buf1 = sc_lds + (PAIR ? 2 : 1) * p.fpg * p.M;
    const float2* __restrict__ tw = (const float2*)a.twiddle;
    sc_load(buf0, a.x + (long long)row * p.T, a.window, p, f0, count);
    if (PAIR)
        sc_load(buf0 + count * p.M, a.y + (long long)row * p.T, a.window, p,
                f0, count);
    const float2* __restrict__ Z = sc_fft(buf0, buf1, tw, p, slots);
    const int bins = p.M + 1;
    const long long base = (long long)row * bins * p.frames;
    float sum1 = 0.f, sum2 = 0.f;
    const int total = bins * count;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        // (the frame is the fast index: bins of one frame are `frames` apart)
        const int k = i / count, fl = i - k * count;
        const long long at = base + (long long)k * p.frames + f0 + fl;
        const float2 X = sc_bin(Z + fl * p.M, tw, p.M, k);
        const float mx = sqrtf(X.x * X.x + X.y * X.y);
        const float sx = sqrtf(pm_max_nan(mx, SC_FLOOR));
        float factor = 0.f;
        if (PAIR) {
            const float2 Y = sc_bin(Z + (count + fl) * p.M, tw, p.M, k);
            const float sy =
                sqrtf(pm_max_nan(sqrtf(Y.x * Y.x + Y.y * Y.y), SC_FLOOR));
            const float d = sy - sx;
            sum1 += fabsf(d);
            sum2 += sy;
            factor = d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f);
        } else {
            if (a.s) a.s[at] = sx;
            if (a.upstream) factor = a.upstream[at];
        }
        if (a.G) {
            float2 g = make_float2(0.f, 0.f);
            // (0 at and under the floor; a NaN bin keeps its NaN, as the
            // phase X / |X| of torch's gradient does)
            if (!(mx <= SC_FLOOR)) {
                const float c = factor * .5f / (sx * mx);
                g = make_float2(c * X.x, c * X.y);
            }
            ((float2*)a.G)[at] = g;
        }
    }
    if (PAIR) {
        sum1 = sc_block_sum(sum1, scratch);
        sum2 = sc_block_sum(sum2, scratch);
        if (threadIdx.x == 0) {
            a.partials[2 * (long long)blockIdx.x] = sum1;
            a.partials[2 * (long long)blockIdx.x + 1] = sum2;
        }
    }
}

// The final pass over the partials: out = (S1, S2, S1 / S2). One workgroup;
// each thread sums a strided share in ascending order, then a tree; in double,
// so that the pass adds no rounding of its own to a batch of any size.
__global__ __launch_bounds__(SC_THREADS) void sc_sums_kernel(
    const float* __restrict__ partials, long long count,
    float* __restrict__ out) {
    __shared__ double scratch[2][SC_THREADS];
    double sum1 = 0., sum2 = 0.;
    for (long long i = threadIdx.x; i < count; i += SC_THREADS) {
        sum1 += (double)partials[2 * i];
        sum2 += (double)partials[2 * i + 1];
    }
    scratch[0][threadIdx.x] = sum1;
    scratch[1][threadIdx.x] = sum2;
    __syncthreads();
    for (int half = SC_THREADS / 2; half >= 1; half >>= 1) {
        if (threadIdx.x < half) {
            scratch[0][threadIdx.x] += scratch[0][threadIdx.x + half];
            scratch[1][threadIdx.x] += scratch[1][threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)scratch[0][0];
        out[1] = (float)scratch[1][0];
        out[2] = (float)(scratch[0][0] / scratch[1][0]);
    }
}

// ---------------------------------------------------------------------------
// The adjoint, first half: frame f of a row's bin gradient G to the windowed
// time-domain frame  u[n] = w[n] Re sum_{k=0..M} G[k] exp(+2 pi i k n / N),
// each bin counted once, the imaginary parts of bins 0 and M ignored. With
// H[0] = Re G[0], H[M] = Re G[M], H[k] = G[k] / 2 otherwise,
//   Zs[k] = (H[k] + conj H[M-k]) + i conj(W^k) (H[k] - conj H[M-k]),  k < M,
// and z = conj FFT_M(conj Zs) holds u[2m] + i u[2m+1] before the window.
// ---------------------------------------------------------------------------
struct ScAdjointArgs {
    const float* G;         // (B, bins, frames, 2)
    const float* window;    // (N)
    const float* twiddle;   // (N, 2)
    float* frames_out;      // (B, frames, N) workspace
    ScPlan p;
};

__device__ __forceinline__ float2 sc_half_bin(const float2* __restrict__ G,
                                              long long stride, int M, int k) {
    const float2 g = G[k * stride];
    if (k == 0 || k == M) return make_float2(g.x, 0.f);
    return make_float2(.5f * g.x, .5f * g.y);
}

__global__ __launch_bounds__(SC_THREADS) void sc_adjoint_frames_kernel(
    ScAdjointArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 sc_lds[];
    const ScPlan& p = a.p;
    const int row = blockIdx.x / p.groups;
    const int f0 = (blockIdx.x - row * p.groups) * p.fpg;
    const int count = p.frames - f0 < p.fpg ? p.frames - f0 : p.fpg;
    float2* buf0 = sc_lds;
    float2* buf1 = sc_lds + p.fpg * p.M;
    const float2* __restrict__ tw = (const float2*)a.twiddle;
    const int bins = p.M + 1;
    const float2* __restrict__ G =
        (const float2*)a.G + (long long)row * bins * p.frames + f0;
    const int total = count * p.M;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        const int k = i / count, fl = i - k * count;
        const float2 h = sc_half_bin(G + fl, p.frames, p.M, k);
        const float2 c = sc_half_bin(G + fl, p.frames, p.M, p.M - k);
        const float2 even = make_float2(h.x + c.x, h.y - c.y);
        const float2 odd = make_float2(h.x - c.x, h.y + c.y);
        const float2 w = tw[k];                     // (cos, -sin): W^k
        // i conj(W^k) odd, conj(W^k) = (w.x, -w.y)
        const float2 r = sc_mul(make_float2(w.x, -w.y), odd);
        // conj Zs
        buf0[fl * p.M + k] = make_float2(even.x - r.y, -(even.y + r.x));
    }
    const float2* __restrict__ z = sc_fft(buf0, buf1, tw, p, count);
    float* __restrict__ out =
        a.frames_out + ((long long)row * p.frames + f0) * p.N;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        const int m = i % p.M;
        const float2 v = z[i];
        const float2 w = *(const float2*)&a.window[2 * m];
        // (frames of a group are back to back: i indexes them all)
        *(float2*)&out[2 * (long long)i] = make_float2(v.x * w.x, -v.y * w.y);
    }
}

// Second half: overlap-add in gather form and the adjoint of a reflect margin
// of `pad`. Sample i of a row is padded sample i + pad; samples 1 .. pad also
// own the left margin's pad - i, samples T-1-pad .. T-2 the right margin's
// pad + 2 (T - 1) - i. A padded sample sums the frames that cover it in
// ascending order (one past the last frame sums nothing); the (up to) three
// padded samples are added centre, left, right.
// grad_x = (or +=) scale[0] * that; a null scale is 1.
struct ScOverlapArgs {
    const float* frames_in;     // (B, frames, N)
    const float* scale;         // device scalar or NULL
    float* grad_x;              // (B, T)
    int N, pad, hop, frames, T, accumulate;
    long long total;            // B * T
};

__device__ __forceinline__ float sc_padded_sample(
    const float* __restrict__ fr, int N, int hop, int frames, int j) {
    // frames f with f hop <= j < f hop + N
    int lo = j - N + 1;
    lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
    int hi = j / hop;
    hi = hi > frames - 1 ? frames - 1 : hi;
    float sum = 0.f;
    for (int f = lo; f <= hi; ++f) sum += fr[(long long)f * N + (j - f * hop)];
    return sum;
}

__global__ __launch_bounds__(SC_THREADS) void sc_overlap_kernel(
    ScOverlapArgs a) {
    const long long at = (long long)blockIdx.x * SC_THREADS + threadIdx.x;
    if (at >= a.total) return;
    const int row = (int)(at / a.T), i = (int)(at - (long long)row * a.T);
    const float* __restrict__ fr =
        a.frames_in + (long long)row * a.frames * a.N;
    float sum = sc_padded_sample(fr, a.N, a.hop, a.frames, i + a.pad);
    if (i >= 1 && i <= a.pad)
        sum += sc_padded_sample(fr, a.N, a.hop, a.frames, a.pad - i);
    if (i <= a.T - 2 && i >= a.T - 1 - a.pad)
        sum += sc_padded_sample(fr, a.N, a.hop, a.frames,
                                a.pad + 2 * (a.T - 1) - i);
    const float v = a.scale ? a.scale[0] * sum : sum;
    a.grad_x[at] = a.accumulate ? a.grad_x[at] + v : v;
}

// ---------------------------------------------------------------------------
// signal (loss.py:158-162): mean over rows of 1 - <p, t> / ((e + |p|)(e + |t|))
// with e = 1e-15. One workgroup a row reduces sum t^2, sum p^2, sum p t into
// stats (rows, 4) = (tt, pp, pt, the row's loss); the final pass takes the mean.
// ---------------------------------------------------------------------------
#define SC_EPS 1e-15f

__global__ __launch_bounds__(SC_THREADS) void sc_signal_rows_kernel(
    const float* __restrict__ y_true, const float* __restrict__ y_pred,
    float* __restrict__ stats, int T) {
    __shared__ float scratch[SC_THREADS / 64];
    const float* __restrict__ t = y_true + (long long)blockIdx.x * T;
    const float* __restrict__ p = y_pred + (long long)blockIdx.x * T;
    float tt = 0.f, pp = 0.f, pt = 0.f;
    for (int i = threadIdx.x; i < T; i += SC_THREADS) {
        const float tv = t[i], pv = p[i];
        tt = fmaf(tv, tv, tt);
        pp = fmaf(pv, pv, pp);
        pt = fmaf(pv, tv, pt);
    }
    tt = sc_block_sum(tt, scratch);
    pp = sc_block_sum(pp, scratch);
    pt = sc_block_sum(pt, scratch);
    if (threadIdx.x == 0) {
        float* __restrict__ o = stats + 4 * (long long)blockIdx.x;
        o[0] = tt; o[1] = pp; o[2] = pt;
        o[3] = 1.f - pt / ((SC_EPS + sqrtf(pp)) * (SC_EPS + sqrtf(tt)));
    }
}

__global__ __launch_bounds__(SC_THREADS) void sc_signal_mean_kernel(
    const float* __restrict__ stats, int rows, float* __restrict__ out) {
    __shared__ float scratch[SC_THREADS / 64];
    float sum = 0.f;
    for (int i = threadIdx.x; i < rows; i += SC_THREADS) sum += stats[4 * i + 3];
    sum = sc_block_sum(sum, scratch);
    if (threadIdx.x == 0) out[0] = sum / (float)rows;
}

// d loss / d p[i] = -(g / rows) (t[i] / ((e + |t|)(e + |p|))
//                                - <p, t> p[i] / ((e + |t|) |p| (e + |p|)^2));
// the second term is 0 for a row of zeros, as the norm's gradient is there.
__global__ __launch_bounds__(SC_THREADS) void sc_signal_backward_kernel(
    const float* __restrict__ y_true, const float* __restrict__ y_pred,
    const float* __restrict__ stats, const float* __restrict__ grad_out,
    float* __restrict__ grad, int rows, int T) {
    const long long at = (long long)blockIdx.x * SC_THREADS + threadIdx.x;
    if (at >= (long long)rows * T) return;
    const float* __restrict__ st = stats + 4 * (at / T);
    const float nt = SC_EPS + sqrtf(st[0]);
    const float np = sqrtf(st[1]), ne = SC_EPS + np;
    const float g = -grad_out[0] / (float)rows;
    float v = y_true[at] / (nt * ne);
    if (np > 0.f) v -= st[2] * y_pred[at] / (nt * np * ne * ne);
    grad[at] = g * v;
}

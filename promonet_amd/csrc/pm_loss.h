// Training-side losses of the FARGAN configurations (promonet/train/loss.py):
// the spectral-convergence loss (:61-150) as a centred STFT, its bin gradient
// and the adjoint of the STFT, and the waveform `signal` loss (:158-162).
//
// The transform. A frame of N real points (N = 2^a or 5 2^a, 64 <= N <= 2560)
// is the complex transform of M = N / 2 points z[m] = v[2m] + i v[2m+1] and
// the split  X[k] = E[k] + W^k O[k],  E = (Z[k] + conj Z[M-k]) / 2,
// O = -i (Z[k] - conj Z[M-k]) / 2,  W = exp(-2 pi i / N),  0 <= k <= M.
// The M-point transform is a Stockham autosort FFT between two LDS buffers:
// one radix-5 stage for the 5 2^a sizes, then radix-4 stages and at most one
// radix-2 stage (the plan is made on the host, pm_loss.hip). A workgroup
// carries `fpg` frames of one row at once (and, for the loss, the same frames
// of the target), and the butterflies of all of them are dealt to the 256
// threads as one pool: at N = 64 a workgroup holds 32 frames, at N = 2560 one.
// Twiddles come from one table W^m, m < N, rounded from float64 on the host.
//
// Nothing here uses a float atomic: sums go through per-workgroup partials and
// one final pass, overlap-add is in gather form, so every output is the same
// bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#define SC_THREADS 256
#define SC_MAX_STAGES 8
#define SC_MAX_POINTS 1280          // complex points of a workgroup's pool
#define SC_FLOOR 1e-7f              // torch.clamp(magnitude, min=1e-7)

struct ScPlan {
    int N, M, hop, frames, T, fpg, groups;  // groups: workgroups per row
    int stages;
    int radix[SC_MAX_STAGES];
};

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
// into `count` transforms of M complex points.
__device__ __forceinline__ void sc_load(float2* __restrict__ dst,
                                        const float* __restrict__ x,
                                        const float* __restrict__ window,
                                        const ScPlan& p, int f0, int count) {
    const int total = count * p.M;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        const int fl = i / p.M, m = i - fl * p.M;
        const int start = (f0 + fl) * p.hop - p.M;      // centre: N / 2 = M
        float pair[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int n = start + 2 * m + h;
            if (n < 0) n = -n;
            if (n >= p.T) n = 2 * (p.T - 1) - n;
            // (T > N / 2: one reflection reaches every sample; the clamp only
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
        const float sx = sqrtf(fmaxf(mx, SC_FLOOR));
        float factor = 0.f;
        if (PAIR) {
            const float2 Y = sc_bin(Z + (count + fl) * p.M, tw, p.M, k);
            const float sy =
                sqrtf(fmaxf(sqrtf(Y.x * Y.x + Y.y * Y.y), SC_FLOOR));
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
            if (mx > SC_FLOOR) {
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

// Second half: overlap-add in gather form and the adjoint of the reflect
// padding. Sample i of a row is padded sample i + M; samples 1 .. M also own
// the left margin's M - i, samples T-1-M .. T-2 the right margin's
// M + 2 (T - 1) - i. A padded sample sums the frames that cover it in
// ascending order; the (up to) three padded samples are added centre, left,
// right. grad_x = (or +=) scale[0] * that.
struct ScOverlapArgs {
    const float* frames_in;     // (B, frames, N)
    const float* scale;         // device scalar
    float* grad_x;              // (B, T)
    int N, M, hop, frames, T, accumulate;
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
    float sum = sc_padded_sample(fr, a.N, a.hop, a.frames, i + a.M);
    if (i >= 1 && i <= a.M)
        sum += sc_padded_sample(fr, a.N, a.hop, a.frames, a.M - i);
    if (i <= a.T - 2 && i >= a.T - 1 - a.M)
        sum += sc_padded_sample(fr, a.N, a.hop, a.frames,
                                a.M + 2 * (a.T - 1) - i);
    const float v = a.scale[0] * sum;
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

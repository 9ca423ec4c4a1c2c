// The look-ahead limiter of promonet/preprocess/loudness.py:114-141 and the
// loudness shift of :179-193 on the device (promonet_amd.preprocess.loudness).
//
// Limiter, all fp32, every operation rounded on its own (this object is built
// with -ffp-contract=off), for n = 0 .. len + delay - 2, x[n] = 0 from len on,
// e[-1] = 0, g[-1] = 1:
//
//   e[n] = max(|x[n]|, e[n-1] * r)
//   t[n] = e[n] > th ? (1 / e[n]) * th : 1
//   g[n] = g[n-1] * a + t[n] * b
//   out[j] = x[j] * g[j + delay - 1]
//
// PRECONDITION: x is finite (the object is built with -fno-honor-nans).
//
// One workgroup owns a row and takes it in tiles of LM_TILE steps n; a lane
// owns a chunk of LM_CHUNK consecutive steps. Three facts make the three
// recurrences parallel and still exact:
//   1. v -> v * r is monotone, so it commutes with max: a chunk computes its
//      envelope from e = 0, and the carry c from the left is laid over it
//      afterwards, c = c * r while c > local[i]; once c <= local[i] it is
//      dominated for good.
//   2. e is used through "e > th" only and v * r <= v, so a carry <= th is
//      dropped (carry 0): audio under the threshold has no serial work.
//   3. With t = 1 the gain has fixed points (1.0f before any limiting, 1 - 4
//      ulp after): a chunk whose envelope stays <= th and whose incoming g
//      satisfies g * a + b == g has g constant.
// Per tile: (0) the tile's x, loaded one tile ahead, goes to LDS; (1) local
// envelopes, one lane a chunk; (2a) thread 0 walks the chunks' carries, only
// while a carry is above th, LM_GROUP chunks per round trip to LDS; (2b) the lanes lay the carries over their chunks
// and compute t * b; (2c) thread 0 walks g through the chunks that are active
// or not at a fixed point; (3) out and gain leave in coalesced stores. A tile
// with nothing above th, no carry and g at a fixed point skips 2a - 2c.
// No workgroup waits on another, nothing spins on memory, every loop is
// bounded by the row's length. `lengths` is read here and nowhere on the host.
#pragma once
#include <hip/hip_runtime.h>

#define LM_THREADS 256
#define LM_CHUNK 4                          // steps per lane: one float4
#define LM_TILE (LM_THREADS * LM_CHUNK)     // steps per workgroup pass
#define LM_GROUP 8                          // chunks thread 0 reads at once
#define LM_STATS 4                          // int32 per row in the workspace

struct LimitArgs {
    const float* x;         // rows of `samples`, x_stride apart
    const int* lengths;     // (rows) or NULL: every row has `samples`
    float* out;             // rows of `samples`, out_stride apart
    float* gain;            // rows of samples + delay - 1, or NULL
    int* stats;             // (rows, LM_STATS): envelope steps, gain steps,
                            // chunks walked, tiles skipped
    long long x_stride, out_stride;
    int samples, delay;
    float a, b, r, th;
};

// g after one step at t = 1 (t * b == b exactly)
__device__ __forceinline__ float lm_rest(float g, float a, float b) {
    return g * a + b;
}

__global__ __launch_bounds__(LM_THREADS) void pm_limit_kernel(LimitArgs p) {
    __shared__ __attribute__((aligned(16))) float xs[2][LM_TILE];   // x ring
    __shared__ __attribute__((aligned(16))) float es[LM_TILE];      // local e
    __shared__ __attribute__((aligned(16))) float tbs[LM_TILE];     // t * b
    __shared__ __attribute__((aligned(16))) float gs[LM_TILE];      // g
    __shared__ float c_in[LM_THREADS];      // the carry entering a chunk
    __shared__ float g_in[LM_THREADS];      // g entering a chunk
    __shared__ int walked[LM_THREADS];      // 1: gs holds the chunk's g
    __shared__ float s_carry, s_g;          // state between tiles
    __shared__ int s_rest;                  // s_g is a fixed point under t = 1

    const int t = threadIdx.x, row = blockIdx.x;
    const int delay = p.delay, lag = delay - 1;
    const float a = p.a, b = p.b, r = p.r, th = p.th;
    int len = p.lengths ? p.lengths[row] : p.samples;
    len = len < 0 ? 0 : (len > p.samples ? p.samples : len);
    const long long steps = (long long)len + lag;       // n = 0 .. steps - 1
    const float* __restrict__ x = p.x + (long long)row * p.x_stride;
    float* __restrict__ out = p.out + (long long)row * p.out_stride;
    const long long gain_stride = (long long)p.samples + lag;
    float* __restrict__ gain =
        p.gain ? p.gain + (long long)row * gain_stride : nullptr;

    for (int j = len + t; j < p.samples; j += LM_THREADS) out[j] = 0.f;
    if (gain)
        for (long long n = steps + t; n < gain_stride; n += LM_THREADS)
            gain[n] = 0.f;
    if (t == 0) { s_carry = 0.f; s_g = 1.f; s_rest = lm_rest(1.f, a, b) == 1.f; }
    int env_steps = 0, gain_steps = 0, chunks_walked = 0, tiles_skipped = 0;

    // x of the first tile; from then on one tile ahead of its use
    float ahead[LM_CHUNK];
#pragma unroll
    for (int k = 0; k < LM_CHUNK; ++k) {
        const long long n = t + k * LM_THREADS;
        ahead[k] = n < len ? x[n] : 0.f;
    }

    int ring = 0;
    for (long long n0 = 0; n0 < steps; n0 += LM_TILE, ring ^= 1) {
        const int count =
            steps - n0 < LM_TILE ? (int)(steps - n0) : LM_TILE;
        const int chunks = (count + LM_CHUNK - 1) / LM_CHUNK;
        // (0) this tile's x to LDS, the next tile's into registers
#pragma unroll
        for (int k = 0; k < LM_CHUNK; ++k)
            xs[ring][t + k * LM_THREADS] = ahead[k];
#pragma unroll
        for (int k = 0; k < LM_CHUNK; ++k) {
            const long long n = n0 + LM_TILE + t + k * LM_THREADS;
            ahead[k] = n < len ? x[n] : 0.f;
        }
        __syncthreads();
        // the state the tile before left (written before its last barrier,
        // and not again before the next one)
        const bool idle = s_carry == 0.f && s_rest;
        const float g_idle = s_g;

        // (1) the chunk's envelope from e = 0
        float e[LM_CHUNK];
        {
            const float4 v = *(const float4*)&xs[ring][t * LM_CHUNK];
            const float in[LM_CHUNK] = {v.x, v.y, v.z, v.w};
            float run = 0.f;
#pragma unroll
            for (int i = 0; i < LM_CHUNK; ++i) {
                run = fmaxf(fabsf(in[i]), run * r);
                e[i] = run;
            }
        }
        // (the largest local e of a chunk is its largest |x|)
        const float top = fmaxf(fmaxf(e[0], e[1]), fmaxf(e[2], e[3]));
        *(float4*)&es[t * LM_CHUNK] = make_float4(e[0], e[1], e[2], e[3]);
        const int loud = __syncthreads_or(t < chunks && top > th);
        if (!loud && idle) {
            // nothing above th, no carry, g at rest: g is constant
            const float g = g_idle;
            for (int i = t; i < count; i += LM_THREADS) {
                const long long n = n0 + i;
                if (gain) gain[n] = g;
                const long long j = n - lag;
                if (j >= 0) {
                    const float xj = lag <= LM_TILE
                        ? xs[(j / LM_TILE) & 1][j % LM_TILE] : x[j];
                    out[j] = xj * g;
                }
            }
            if (t == 0) ++tiles_skipped;
            __syncthreads();
            continue;
        }

        // (2a) the carries, by one lane: a chunk costs a step per sample only
        // while a carry above th is alive in it
        if (t == 0) {
            float carry = s_carry;
            // a group of chunks per round trip to LDS
            for (int k0 = 0; k0 < chunks; k0 += LM_GROUP) {
                float4 v[LM_GROUP];
#pragma unroll
                for (int q = 0; q < LM_GROUP; ++q)
                    v[q] = *(const float4*)&es[(k0 + q) * LM_CHUNK];
#pragma unroll
                for (int q = 0; q < LM_GROUP; ++q) {
                    if (k0 + q >= chunks) break;
                    c_in[k0 + q] = carry;
                    float leave = v[q].w;   // the chunk's last local e
                    if (carry > th) {
                        const float local[LM_CHUNK] = {
                            v[q].x, v[q].y, v[q].z, v[q].w};
                        bool alive = true;
#pragma unroll
                        for (int i = 0; i < LM_CHUNK; ++i) {
                            if (alive) {
                                carry = carry * r;
                                ++env_steps;
                                // dominated, or under th: nothing later can
                                // need it
                                alive = carry > local[i] && carry > th;
                            }
                        }
                        if (alive) leave = carry;
                    }
                    carry = leave > th ? leave : 0.f;
                }
            }
            s_carry = carry;
        }
        __syncthreads();

        // (2b) the carry over the chunk, then t * b
        bool active = false;
        if (t < chunks) {
            float carry = c_in[t];
            bool alive = carry > th;
            float tb[LM_CHUNK];
#pragma unroll
            for (int i = 0; i < LM_CHUNK; ++i) {
                if (alive) {
                    carry = carry * r;
                    alive = carry > e[i] && carry > th;
                    if (alive) e[i] = carry;
                }
                const bool over = e[i] > th;
                active |= over;
                const float reciprocal = 1.f / e[i];
                tb[i] = over ? (reciprocal * th) * b : b;
            }
            *(float4*)&tbs[t * LM_CHUNK] =
                make_float4(tb[0], tb[1], tb[2], tb[3]);
        }
        c_in[t] = active ? 1.f : 0.f;       // now: the chunk limits
        __syncthreads();

        // (2c) the gain, by one lane: only chunks that limit, or that g
        // enters away from a fixed point, are walked
        if (t == 0) {
            float g = s_g;
            for (int k0 = 0; k0 < chunks; k0 += LM_GROUP) {
                float4 v[LM_GROUP];
                float limits[LM_GROUP];
#pragma unroll
                for (int q = 0; q < LM_GROUP; ++q) {
                    v[q] = *(const float4*)&tbs[(k0 + q) * LM_CHUNK];
                    limits[q] = c_in[k0 + q];
                }
#pragma unroll
                for (int q = 0; q < LM_GROUP; ++q) {
                    const int k = k0 + q;
                    if (k >= chunks) break;
                    g_in[k] = g;
                    const bool walk =
                        limits[q] != 0.f || lm_rest(g, a, b) != g;
                    walked[k] = walk;
                    if (walk) {
                        float4 w;
                        w.x = g = g * a + v[q].x;
                        w.y = g = g * a + v[q].y;
                        w.z = g = g * a + v[q].z;
                        w.w = g = g * a + v[q].w;
                        *(float4*)&gs[k * LM_CHUNK] = w;
                        gain_steps += LM_CHUNK;
                        ++chunks_walked;
                    }
                }
            }
            // a partial last chunk of the row walks past `steps`: that g is
            // never read (the row ends with this tile)
            s_g = g;
            s_rest = lm_rest(g, a, b) == g;
        }
        __syncthreads();

        // (3) out[j] = x[j] * g[j + delay - 1], and g itself
        for (int i = t; i < count; i += LM_THREADS) {
            const int k = i / LM_CHUNK;
            const float g = walked[k] ? gs[i] : g_in[k];
            const long long n = n0 + i;
            if (gain) gain[n] = g;
            const long long j = n - lag;
            if (j >= 0) {
                const float xj = lag <= LM_TILE
                    ? xs[(j / LM_TILE) & 1][j % LM_TILE] : x[j];
                out[j] = xj * g;
            }
        }
        __syncthreads();
    }
    if (t == 0 && p.stats) {
        int* stats = p.stats + (long long)row * LM_STATS;
        stats[0] = env_steps; stats[1] = gain_steps;
        stats[2] = chunks_walked; stats[3] = tiles_skipped;
    }
}

// out = x * gain, gain = 2^(db / 10) per frame, interpolated linearly to the
// row's samples as torch.nn.functional.interpolate(align_corners=False) does:
// src = max(0, (n + .5) F / N - .5) = ((2 n + 1) F - N) / 2 N, taken apart in
// integers (a float src loses bits at a few hundred thousand samples).
#define LS_THREADS 256

struct ShiftArgs {
    const float* x;
    const float* db;            // rows of `frames`, db_stride apart
    const int* lengths;         // (rows) or NULL
    const int* frame_lengths;   // (rows) or NULL
    float* out;
    long long x_stride, db_stride, out_stride;
    int samples, frames;
};

__global__ __launch_bounds__(LS_THREADS) void pm_loudness_shift_kernel(
        ShiftArgs p) {
    const int row = blockIdx.y;
    const int n = blockIdx.x * LS_THREADS + threadIdx.x;
    if (n >= p.samples) return;
    int N = p.lengths ? p.lengths[row] : p.samples;
    N = N < 0 ? 0 : (N > p.samples ? p.samples : N);
    float* __restrict__ out = p.out + (long long)row * p.out_stride;
    if (n >= N) { out[n] = 0.f; return; }
    int F = p.frame_lengths ? p.frame_lengths[row] : p.frames;
    F = F < 1 ? 1 : (F > p.frames ? p.frames : F);
    const float* __restrict__ db = p.db + (long long)row * p.db_stride;
    const float v = p.x[(long long)row * p.x_stride + n];
    if (F == 1) { out[n] = v * exp2f(db[0] / 10.f); return; }
    const long long numerator = (2ll * n + 1) * F - N, denominator = 2ll * N;
    int i0 = 0;
    float w = 0.f;
    if (numerator > 0) {
        long long rest;
        if ((2ll * N + 1) * F < 0xffffffffll) {     // the usual, 32-bit case
            const unsigned q = (unsigned)numerator / (unsigned)denominator;
            i0 = (int)q;
            rest = numerator - (long long)q * denominator;
        } else {
            const long long q = numerator / denominator;
            i0 = (int)q;
            rest = numerator - q * denominator;
        }
        w = (float)rest / (float)denominator;
    }
    // (n < N: src < F - .5, so i0 <= F - 1)
    const int i1 = i0 + 1 < F ? i0 + 1 : F - 1;
    const float g0 = exp2f(db[i0] / 10.f), g1 = exp2f(db[i1] / 10.f);
    out[n] = v * ((1.f - w) * g0 + w * g1);
}

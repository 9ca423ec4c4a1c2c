// The spectrograms at the entrance of the spectral discriminators
// (promonet/model/discriminator.py), forward and backward, on the transform of
// pm_stockham.h (the plan, the loader, the FFT, the tables and the split of a
// row's frames over workgroups are that file's):
//   R    DiscriminatorR.spectrogram (:129-143): |X| as (B, bins, frames);
//   CMB  DiscriminatorCMB.spectrogram (:175-192): |X| as (B, frames, bins),
//        which the caller slices into bands;
//   DB   SpecDiscriminatorBase.spectrogram (:278-299): 20 log10 max(|X|, 1e-5)
//        under a floor of 80 dB below the maximum of the WHOLE batch.
// The frames are not centred by the transform: the caller names the reflect
// margin `pad` ((n_fft - hop) / 2 for R and CMB, n_fft / 2 for DB), pad < T,
// and frames = 1 + (T + 2 pad - N) / hop.
//
// Backward: the transform again from x, the bin gradient G (B, bins, frames, 2)
// from the upstream gradient, and the adjoint pair of pm_loss.h through
// pm_sc_adjoint_launch (pm_host.h): the frames, then their overlap-add in
// gather form with the plan's `pad`.
// DB reads the forward's output and its (max, floor) instead of a second
// reduction over a second transform: an element is on the floor where the
// saved output is <= floor, it holds the maximum where the saved output equals
// max. The sum of the upstream over the floored elements goes to the maximum,
// shared evenly among the elements that hold it. An element exactly AT the
// floor before the floor was applied cannot be told from one below it, so its
// whole upstream goes to the floor (torch gives each side a half).
//
// No float atomics, fixed-order partial sums: the same bits on every run.
//
// NON-FINITE VALUES. This header promises torch's semantics on inf and NaN
// (DESIGN section 27): torch.clamp, amax and maximum keep a NaN, so one NaN
// bin makes the maximum, the floor and with them the whole decibel
// spectrogram NaN, and amax's backward (the upstream over the number of
// maxima, none of which equals a NaN) makes the whole gradient NaN. The
// object is built with -fhonor-nans (Makefile), or the test of a NaN folds.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_nonfinite.h"
#include "pm_stockham.h"

#define DS_R 0
#define DS_CMB 1
#define DS_DB 2
#define DS_AMIN 1e-5f                   // amplitude_to_DB(amin=1e-5)
#define DS_TOP_DB 80.f                  // top_db
#define DS_DB_SLOPE 8.6858896380650366f // 20 / ln 10
#define DS_SUM_GROUPS 1024              // most workgroups of ds_floor_sums

struct DsArgs {
    const float* x;         // (B, T)
    const float* window;    // (N), already padded to N
    const float* twiddle;   // (N, 2)
    const float* upstream;  // GRAD: in the layout of the mode's output
    const float* saved;     // GRAD, DB: the forward's output (B, bins, frames)
    const float* stats;     // GRAD, DB: (max, floor) of the forward
    const float* share;     // GRAD, DB: floored upstream / number of maxima
    float* out;             // forward: R, DB (B, bins, frames); CMB (B, frames, bins)
    float* G;               // GRAD: (B, bins, frames, 2)
    float* partials;        // forward, DB: one maximum a workgroup
    ScPlan p;
};

// Maximum over the workgroup (NaN if any is); the result is valid in thread 0.
__device__ __forceinline__ float ds_block_max(float v, float* scratch) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = pm_max_nan(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float top = scratch[0];
    for (int w = 1; w < SC_THREADS / 64; ++w) top = pm_max_nan(top, scratch[w]);
    return top;
}

// The transform of `fpg` frames of one row and the epilogue of a mode.
// GRAD = false: the mode's output (DB: before the floor, and the workgroup's
// maximum). GRAD = true: G from the upstream gradient,
//   R, CMB  u X / |X|, 0 where |X| = 0;
//   DB      (u above the floor + share at a maximum) (20 / ln 10) X / |X|^2,
//           0 where |X| < 1e-5.
// LDS: two buffers of fpg * M complex points.
template <int MODE, bool GRAD>
__global__ __launch_bounds__(SC_THREADS) void ds_transform_kernel(DsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 ds_lds[];
    __shared__ float scratch[SC_THREADS / 64];
    const ScPlan& p = a.p;
    const int row = blockIdx.x / p.groups;
    const int f0 = (blockIdx.x - row * p.groups) * p.fpg;
    const int count = p.frames - f0 < p.fpg ? p.frames - f0 : p.fpg;
    float2* buf0 = ds_lds;
    float2* buf1 = ds_lds + p.fpg * p.M;
    const float2* __restrict__ tw = (const float2*)a.twiddle;
    sc_load(buf0, a.x + (long long)row * p.T, a.window, p, f0, count);
    const float2* __restrict__ Z = sc_fft(buf0, buf1, tw, p, count);
    const int bins = p.M + 1;
    const long long base = (long long)row * bins * p.frames;
    float top = -3.0e38f, peak = 0.f, floor_db = 0.f, share = 0.f;
    if (MODE == DS_DB && GRAD) {
        peak = a.stats[0];
        floor_db = a.stats[1];
        share = a.share[0];
    }
    const int total = bins * count;
    for (int i = threadIdx.x; i < total; i += SC_THREADS) {
        // the fast index of the loop is the fast index of what it writes: the
        // bin for CMB's output, the frame for everything else (G included)
        int k, fl;
        if (MODE == DS_CMB && !GRAD) {
            fl = i / bins; k = i - fl * bins;
        } else {
            k = i / count; fl = i - k * count;
        }
        const long long plain = base + (long long)k * p.frames + f0 + fl;
        const long long at =
            MODE == DS_CMB ? base + (long long)(f0 + fl) * bins + k : plain;
        const float2 X = sc_bin(Z + fl * p.M, tw, p.M, k);
        const float mx = sqrtf(X.x * X.x + X.y * X.y);
        if (!GRAD) {
            if (MODE == DS_DB) {
                const float db = 20.f * log10f(pm_max_nan(mx, DS_AMIN));
                top = pm_max_nan(top, db);
                a.out[at] = db;
            } else {
                a.out[at] = mx;
            }
        } else {
            float c = 0.f;
            if (MODE == DS_DB) {
                const float o = a.saved[at];
                float f = o > floor_db ? a.upstream[at] : 0.f;
                if (o == peak) f += share;
                // (a NaN maximum: no element holds it, and the floored
                // upstream over their number, none, is NaN everywhere)
                if (peak != peak) f = peak;
                if (mx >= DS_AMIN) c = f * DS_DB_SLOPE / (mx * mx);
            } else if (mx > 0.f) {
                c = a.upstream[at] / mx;
            }
            ((float2*)a.G)[plain] = make_float2(c * X.x, c * X.y);
        }
    }
    if (MODE == DS_DB && !GRAD) {
        top = ds_block_max(top, scratch);
        if (threadIdx.x == 0) a.partials[blockIdx.x] = top;
    }
}

// DB, the rest of the forward: stats = (max, max - 80) from the workgroups'
// maxima (one workgroup; a maximum does not depend on the order) ...
__global__ __launch_bounds__(SC_THREADS) void ds_floor_kernel(
    const float* __restrict__ partials, long long count,
    float* __restrict__ stats) {
    __shared__ float scratch[SC_THREADS / 64];
    float top = -3.0e38f;
    for (long long i = threadIdx.x; i < count; i += SC_THREADS)
        top = pm_max_nan(top, partials[i]);
    top = ds_block_max(top, scratch);
    if (threadIdx.x == 0) {
        stats[0] = top;
        stats[1] = top - DS_TOP_DB;
    }
}

// ... and out = max(out, floor).
__global__ __launch_bounds__(SC_THREADS) void ds_apply_floor_kernel(
    float* __restrict__ out, long long total,
    const float* __restrict__ stats) {
    const long long at = (long long)blockIdx.x * SC_THREADS + threadIdx.x;
    if (at >= total) return;
    out[at] = pm_max_nan(out[at], stats[1]);
}

// DB, before the bin gradient: per workgroup the sum of the upstream over the
// floored elements and the number of elements that hold the maximum, in
// double, each thread over a strided share in ascending order, then a tree.
__device__ __forceinline__ void ds_tree_sum(double (*scratch)[SC_THREADS],
                                            double v0, double v1) {
    scratch[0][threadIdx.x] = v0;
    scratch[1][threadIdx.x] = v1;
    __syncthreads();
    for (int half = SC_THREADS / 2; half >= 1; half >>= 1) {
        if (threadIdx.x < half) {
            scratch[0][threadIdx.x] += scratch[0][threadIdx.x + half];
            scratch[1][threadIdx.x] += scratch[1][threadIdx.x + half];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SC_THREADS) void ds_floor_sums_kernel(
    const float* __restrict__ saved, const float* __restrict__ upstream,
    long long total, const float* __restrict__ stats,
    double* __restrict__ partials) {
    __shared__ double scratch[2][SC_THREADS];
    const float peak = stats[0], floor_db = stats[1];
    double floored = 0., maxima = 0.;
    const long long stride = (long long)gridDim.x * SC_THREADS;
    for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x;
         i < total; i += stride) {
        const float o = saved[i];
        if (o <= floor_db) floored += (double)upstream[i];
        if (o == peak) maxima += 1.;
    }
    ds_tree_sum(scratch, floored, maxima);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = scratch[0][0];
        partials[2 * blockIdx.x + 1] = scratch[1][0];
    }
}

// share = (floored upstream) / (number of maxima): what each element that
// holds the maximum receives through the floor. One workgroup.
__global__ __launch_bounds__(SC_THREADS) void ds_share_kernel(
    const double* __restrict__ partials, int count, float* __restrict__ share) {
    __shared__ double scratch[2][SC_THREADS];
    double floored = 0., maxima = 0.;
    for (int i = threadIdx.x; i < count; i += SC_THREADS) {
        floored += partials[2 * i];
        maxima += partials[2 * i + 1];
    }
    ds_tree_sum(scratch, floored, maxima);
    if (threadIdx.x == 0)
        share[0] = scratch[1][0] > 0. ? (float)(scratch[0][0] / scratch[1][0])
                                      : 0.f;
}

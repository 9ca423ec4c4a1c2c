// The last third of a training step (promonet/train/core.py:335-369) on the
// device: the statistics of every gradient, the clip coefficient, the AdamW
// update and the update of the loss scale, on the pattern of pm_adv.h. An
// entry is one parameter: param, exp_avg and exp_avg_sq dense fp32, grad dense
// fp32, f16 or bf16 and read as stored. The table of entries travels in the
// kernel arguments (OPT_MAX_ENTRIES a launch, longer lists take several
// launches); one workgroup a chunk of OPT_CHUNK elements, and a chunk never
// spans two tensors.
//
// The statistics pass: every workgroup writes five partials of its chunk (the
// maximum, the minimum, the sum, the sum of squares, the count of NaN and
// +-inf), the two sums in pm_adv.h's order: thread t takes the 8 elements
// from (256 j + t) 8 on, j = 0 .. 3, one by one in fp32, and the workgroup
// sums its threads as adv_block_sum does. A non-finite element raises the
// count and adds +0 to both sums, which changes no bit of them. One final
// workgroup takes the maximum and the minimum of the partials (exact in any
// order), sums the chunks of the whole list in ascending order in double
// (mean = sum / numel and norm = sqrt(sum of squares), each rounded once),
// and writes the step's control block: found_inf, inv_scale, the clip
// coefficient, and the optimizer's state advanced by one step
// (opt_final_kernel states the rules). Nothing of it is read on the host.
//
// The update pass: every element on its own,
//   g = (grad inv_scale) coef
//   p = p (float)(1 - lr wd)
//   m = m + (float)(1 - beta1) (g - m)
//   v = v (float)beta2 + (float)(1 - beta2) (g g)
//   d = sqrtf(v) / (float)sqrt(1 - b2pow) + (float)eps
//   p = p + (float)(-lr / (1 - b1pow)) (m / d)
// each fp32 operation rounded on its own, division and square root correctly
// rounded (hipcc's default). Neither factor of g is skipped: both products are
// always made, and x 1.f is x for every fp32 x, so a step without a scale or
// without a clip has the bits of one that skips them. The constants are
// formed in double by every thread from the state block (b1pow = beta1^step
// and b2pow = beta2^step as doubles multiplied up step by step: no pow) and
// from lr, beta1, beta2, eps and weight_decay, which are kernel arguments: a
// captured graph replays the values it was captured with, and changing one
// means capturing again. When found_inf is set the pass writes nothing. A
// whole chunk of a tensor whose four pointers are 16-byte aligned issues every
// load before the first arithmetic; tails and other tensors go 8 elements at
// a time, one by one, and produce the same bits.
//
// Built with -ffp-contract=off -fhonor-nans (Makefile): every product and sum
// rounds on its own, in fp32 and in the double constants, as
// tests/optim_oracle.py states them, and NaN gradients are seen. No float
// atomic anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include "promonet_hip.h"
#include "pm_multi.h"

#define OPT_THREADS ADV_THREADS
#define OPT_CHUNK ADV_CHUNK
#define OPT_MAX_ENTRIES 64
#define OPT_MAX_FOUND 8         // found_inf scalars a scaler update reads

struct OptEntry {
    float* p;               // the update only
    float* m;
    float* v;
    const void* g;
    long long numel;
    int first;              // the entry's first workgroup within the launch
    unsigned char dtype, aligned, unused[2];
};

struct OptTable {           // 3 088 bytes of kernel arguments
    OptEntry e[OPT_MAX_ENTRIES];
    int count;
    int unused;
    long long base;         // workgroups of the launches before this one
};

struct OptPartials {        // one value a workgroup of the whole list, each
    float* max;
    float* min;
    float* sum;
    float* sq;
    unsigned* bad;
};

struct OptHyper { double lr, beta1, beta2, eps, weight_decay; };

struct OptFound { float* p[OPT_MAX_FOUND]; int count; };

// ---------------------------------------------------------------------------
// The statistics pass: five partials a workgroup
// ---------------------------------------------------------------------------
struct OptStats { float max, min, sum, sq; unsigned bad; };

// (pm_optim.o is built with -fhonor-nans: under the library's -fno-honor-nans
// the compiler reads this test of the exponent bits as |g| != inf, and a NaN
// is taken for finite. The maximum and the minimum never see a NaN.)
__device__ __forceinline__ void opt_take(OptStats& s, float g) {
    const bool finite = (__float_as_uint(g) & 0x7f800000u) != 0x7f800000u;
    const float x = finite ? g : 0.f;
    s.max = fmaxf(s.max, finite ? g : -INFINITY);
    s.min = fminf(s.min, finite ? g : INFINITY);
    s.sum += x;
    s.sq += x * x;
    s.bad += finite ? 0u : 1u;
}

template <typename T>
__device__ __forceinline__ void opt_stats_full(const OptEntry& e,
                                               long long start, OptStats& s) {
    float g[ADV_ROUNDS][ADV_VEC];
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j)
        AdvIo<T>::load8(
            e.g, start + (j * OPT_THREADS + (int)threadIdx.x) * ADV_VEC, g[j]);
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j)
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i) opt_take(s, g[j][i]);
}

__device__ __forceinline__ void opt_stats_tail(const OptEntry& e,
                                               long long start, int n,
                                               OptStats& s) {
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const int i0 = (j * OPT_THREADS + (int)threadIdx.x) * ADV_VEC;
        const int valid = n - i0;
        if (valid <= 0) break;
        float g[ADV_VEC];
        adv_load_any(e.g, e.dtype, e.aligned && valid >= ADV_VEC, start + i0,
                     valid, g);
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            if (i < valid) opt_take(s, g[i]);
    }
}

// max, min or an integer sum over the workgroup; valid in thread 0
template <typename T, typename Op>
__device__ __forceinline__ T opt_block_reduce(T v, T* scratch, Op op) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m, 64));
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    T total = scratch[0];
    for (int w = 1; w < OPT_THREADS / 64; ++w) total = op(total, scratch[w]);
    return total;
}

struct OptMax {
    __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct OptMin {
    __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct OptAdd {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};

__global__ __launch_bounds__(OPT_THREADS) void opt_partials_kernel(
    OptTable t, OptPartials out) {
    __shared__ float scratch[4][OPT_THREADS / 64];
    __shared__ unsigned counts[OPT_THREADS / 64];
    const int k = adv_find(t, blockIdx.x);
    const OptEntry& e = t.e[k];
    const long long start = (long long)(blockIdx.x - e.first) * OPT_CHUNK;
    const long long left = e.numel - start;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    OptStats s = {-INFINITY, INFINITY, 0.f, 0.f, 0u};
    if (n == OPT_CHUNK && e.aligned) {
        if (e.dtype == PM_F32) opt_stats_full<float>(e, start, s);
        else if (e.dtype == PM_F16) opt_stats_full<_Float16>(e, start, s);
        else opt_stats_full<__bf16>(e, start, s);
    } else {
        opt_stats_tail(e, start, n, s);
    }
    s.max = opt_block_reduce(s.max, scratch[0], OptMax());
    s.min = opt_block_reduce(s.min, scratch[1], OptMin());
    s.sum = adv_block_sum(s.sum, scratch[2]);
    s.sq = adv_block_sum(s.sq, scratch[3]);
    s.bad = opt_block_reduce(s.bad, counts, OptAdd());
    if (threadIdx.x == 0) {
        const long long at = t.base + blockIdx.x;
        out.max[at] = s.max;
        out.min[at] = s.min;
        out.sum[at] = s.sum;
        out.sq[at] = s.sq;
        out.bad[at] = s.bad;
    }
}

// ---------------------------------------------------------------------------
// The final pass, one workgroup: the five figures and the control block.
// stats (PM_OPTIM_STATS floats, promonet_hip.h) and state {step, b1pow, b2pow}
//   found_inf = 1 if the count is not 0 or the incoming found_inf is not 0
//   inv_scale = (float)(1.0 / (double)grad_scale[0]), 1 without a grad_scale
//   coef      = 1; with a clip (clip >= 0) the reference's order: the largest
//               magnitude of the gradients AS THEY ARE (still scaled) against
//               the threshold, and only above it  total = magnitude inv_scale,
//               coef = min((float)clip / (total + 1e-6f), 1.f)
//   unless found_inf: step += 1, b1pow *= beta1, b2pow *= beta2
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void opt_final_kernel(
    OptPartials part, long long groups, long long numel,
    const float* __restrict__ grad_scale, const float* __restrict__ found_in,
    double clip, double beta1, double beta2, double* __restrict__ state,
    float* __restrict__ stats) {
    __shared__ float scratch[2][OPT_THREADS / 64];
    __shared__ unsigned long long counts[OPT_THREADS / 64];
    __shared__ double squares;
    float max = -INFINITY, min = INFINITY;
    unsigned long long bad = 0;
    for (long long i = threadIdx.x; i < groups; i += OPT_THREADS) {
        max = fmaxf(max, part.max[i]);
        min = fminf(min, part.min[i]);
        bad += part.bad[i];
    }
    max = opt_block_reduce(max, scratch[0], OptMax());
    min = opt_block_reduce(min, scratch[1], OptMin());
    bad = opt_block_reduce(bad, counts, OptAdd());
    // the two sums side by side: wave 0 the sum, wave 1 the sum of squares
    const int wave = threadIdx.x >> 6;
    double sum = 0.;
    if (wave == 0) sum = adv_ordered_sum(part.sum, groups);
    if (wave == 1) {
        const double sq = adv_ordered_sum(part.sq, groups);
        if ((threadIdx.x & 63) == 0) squares = sq;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const bool found = bad != 0 || (found_in && found_in[0] != 0.f);
    const float inv_scale =
        grad_scale ? (float)(1.0 / (double)grad_scale[0]) : 1.f;
    float coef = 1.f;
    const float magnitude = fmaxf(max, fabsf(min));
    if (clip >= 0. && (double)magnitude > clip) {
        const float total = magnitude * inv_scale;
        coef = fminf((float)clip / (total + 1e-6f), 1.f);
    }
    stats[PM_OPTIM_MAX] = max;
    stats[PM_OPTIM_MIN] = min;
    stats[PM_OPTIM_MEAN] = (float)(sum / (double)numel);
    stats[PM_OPTIM_NORM] = (float)sqrt(squares);
    stats[PM_OPTIM_NORM_SQ] = (float)squares;
    stats[PM_OPTIM_NONFINITE] = (float)bad;
    stats[PM_OPTIM_FOUND_INF] = found ? 1.f : 0.f;
    stats[PM_OPTIM_INV_SCALE] = inv_scale;
    stats[PM_OPTIM_COEF] = coef;
    if (state && !found) {
        state[0] += 1.;
        state[1] *= beta1;
        state[2] *= beta2;
    }
}

// ---------------------------------------------------------------------------
// The update pass
// ---------------------------------------------------------------------------
struct OptConst {
    float inv_scale, coef, decay, one_minus_beta1, beta2, one_minus_beta2,
        bias2, eps, step;
};

__device__ __forceinline__ OptConst opt_constants(
    const float* __restrict__ stats, const double* __restrict__ state,
    const OptHyper& h) {
    OptConst c;
    c.inv_scale = stats[PM_OPTIM_INV_SCALE];
    c.coef = stats[PM_OPTIM_COEF];
    c.decay = (float)(1. - h.lr * h.weight_decay);
    c.one_minus_beta1 = (float)(1. - h.beta1);
    c.beta2 = (float)h.beta2;
    c.one_minus_beta2 = (float)(1. - h.beta2);
    c.bias2 = (float)sqrt(1. - state[2]);
    c.eps = (float)h.eps;
    c.step = (float)(-h.lr / (1. - state[1]));
    return c;
}

__device__ __forceinline__ void opt_update(const OptConst& c, float g,
                                           float& p, float& m, float& v) {
    g = (g * c.inv_scale) * c.coef;
    p = p * c.decay;
    m = m + c.one_minus_beta1 * (g - m);
    v = v * c.beta2 + c.one_minus_beta2 * (g * g);
    const float d = sqrtf(v) / c.bias2 + c.eps;
    p = p + c.step * (m / d);
}

template <typename T>
__device__ __forceinline__ void opt_step_full(
    const OptEntry& e, long long start, const float* __restrict__ stats,
    const double* __restrict__ state, const OptHyper& h) {
    float g[ADV_ROUNDS][ADV_VEC], p[ADV_ROUNDS][ADV_VEC],
        m[ADV_ROUNDS][ADV_VEC], v[ADV_ROUNDS][ADV_VEC];
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const long long at =
            start + (j * OPT_THREADS + (int)threadIdx.x) * ADV_VEC;
        AdvIo<T>::load8(e.g, at, g[j]);
        AdvIo<float>::load8(e.p, at, p[j]);
        AdvIo<float>::load8(e.m, at, m[j]);
        AdvIo<float>::load8(e.v, at, v[j]);
    }
    const OptConst c = opt_constants(stats, state, h);
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const long long at =
            start + (j * OPT_THREADS + (int)threadIdx.x) * ADV_VEC;
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            opt_update(c, g[j][i], p[j][i], m[j][i], v[j][i]);
        AdvIo<float>::store8(e.p, at, p[j]);
        AdvIo<float>::store8(e.m, at, m[j]);
        AdvIo<float>::store8(e.v, at, v[j]);
    }
}

__device__ __forceinline__ void opt_step_tail(
    const OptEntry& e, long long start, int n,
    const float* __restrict__ stats, const double* __restrict__ state,
    const OptHyper& h) {
    const OptConst c = opt_constants(stats, state, h);
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const int i0 = (j * OPT_THREADS + (int)threadIdx.x) * ADV_VEC;
        const int valid = n - i0;
        if (valid <= 0) break;
        const bool vector = e.aligned && valid >= ADV_VEC;
        const long long at = start + i0;
        float g[ADV_VEC], p[ADV_VEC], m[ADV_VEC], v[ADV_VEC];
        adv_load_any(e.g, e.dtype, vector, at, valid, g);
        adv_load_any(e.p, PM_F32, vector, at, valid, p);
        adv_load_any(e.m, PM_F32, vector, at, valid, m);
        adv_load_any(e.v, PM_F32, vector, at, valid, v);
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            opt_update(c, g[i], p[i], m[i], v[i]);
        adv_store_any(e.p, PM_F32, vector, at, valid, p);
        adv_store_any(e.m, PM_F32, vector, at, valid, m);
        adv_store_any(e.v, PM_F32, vector, at, valid, v);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void opt_step_kernel(
    OptTable t, const float* __restrict__ stats,
    const double* __restrict__ state, OptHyper h) {
    if (stats[PM_OPTIM_FOUND_INF] != 0.f) return;
    const int k = adv_find(t, blockIdx.x);
    const OptEntry& e = t.e[k];
    const long long start = (long long)(blockIdx.x - e.first) * OPT_CHUNK;
    const long long left = e.numel - start;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    if (n == OPT_CHUNK && e.aligned) {
        if (e.dtype == PM_F32) opt_step_full<float>(e, start, stats, state, h);
        else if (e.dtype == PM_F16)
            opt_step_full<_Float16>(e, start, stats, state, h);
        else opt_step_full<__bf16>(e, start, stats, state, h);
    } else {
        opt_step_tail(e, start, n, stats, state, h);
    }
}

// ---------------------------------------------------------------------------
// torch.amp.GradScaler.update()'s rule, one thread: found = any of the
// found_inf scalars is not 0. On found  scale *= backoff  and the tracker goes
// to 0; else the tracker is incremented and, at growth_interval,  scale *=
// growth  (unless that is inf) and the tracker goes to 0. The products are
// torch's: in double, rounded once. Then every found_inf scalar is cleared.
// ---------------------------------------------------------------------------
__global__ void opt_scaler_kernel(float* __restrict__ scale,
                                  int* __restrict__ tracker, OptFound found,
                                  double growth, double backoff,
                                  int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool any = false;
    for (int i = 0; i < found.count; ++i) any = any || found.p[i][0] != 0.f;
    if (any) {
        scale[0] = (float)((double)scale[0] * backoff);
        tracker[0] = 0;
    } else {
        const int successful = tracker[0] + 1;
        if (successful == interval) {
            const float grown = (float)((double)scale[0] * growth);
            if ((__float_as_uint(grown) & 0x7fffffffu) != 0x7f800000u)
                scale[0] = grown;
            tracker[0] = 0;
        } else {
            tracker[0] = successful;
        }
    }
    for (int i = 0; i < found.count; ++i) found.p[i][0] = 0.f;
}

// The adversarial half of promonet/train/loss.py (:11-53): feature matching
// and the discriminator / generator losses, as one multi-tensor mean. For a
// list of K entries  mean_k = (1 / numel_k) sum_i op_k(a_k[i], b_k[i])  and
// the total of the means; the backward writes d total / d input scaled by a
// device scalar.
//
// Every tensor is cut into chunks of ADV_CHUNK elements, one workgroup a
// chunk, and a chunk never spans two tensors: a tensor's mean has the same
// bits alone and in any list. The table of entries travels in the kernel
// arguments (at most ADV_MAX_ENTRIES a launch; longer lists take several
// launches that write their own slice of one partials buffer), so there is no
// host-to-device copy and every launch captures into a graph.
//
// The order of a chunk's sum is fixed and the same on every path: thread t
// takes the 8 elements from (256 j + t) 8 on, j = 0 .. 3, adds their terms
// one by one in ascending order, and the workgroup sums its threads as
// sc_block_sum does. A tensor whose pointers are 16-byte aligned reads those
// 8 elements as 16-byte vectors, any other one by one: the bits do not
// depend on the alignment. 16-bit values are read as stored and converted in
// registers. One final workgroup sums each tensor's partials in ascending
// order in double. No float atomic anywhere.
//
// Built with -ffp-contract=off (Makefile): every product and sum rounds on
// its own, as the fp32 restatement of the tests does.
//
// NON-FINITE VALUES. This header promises torch's semantics on inf and NaN
// (DESIGN section 27): a term of a NaN is NaN, as torch.clamp(min=0) keeps
// it, so an overflowed logit reaches the mean, the total and the scaler. The
// object is built with -fhonor-nans (Makefile), or the test of a NaN folds.
#pragma once
#include <hip/hip_runtime.h>

#include "promonet_hip.h"
// the chunk, the loads and stores, adv_block_sum and adv_ordered_sum
#include "pm_multi.h"
#include "pm_nonfinite.h"

#define ADV_MAX_ENTRIES 64
#define ADV_FINAL_THREADS 1024

struct AdvEntry {
    const void* a;
    const void* b;          // ABS_DIFF only
    void* grad;             // backward only: of b for ABS_DIFF, of a otherwise
    long long numel;
    int first;              // the entry's first workgroup within the launch
    unsigned char op, dtype, aligned, unused;
};

struct AdvTable {           // 2 576 bytes of kernel arguments
    AdvEntry e[ADV_MAX_ENTRIES];
    int count;
    int index0;             // list index of e[0]
    long long base;         // workgroups of the launches before this one
};

struct AdvMeta {            // written by an entry's first workgroup
    long long numel;
    long long first;        // index of its first partial
};

// ---------------------------------------------------------------------------
// The five terms and their derivatives (torch's: the sign of 0 is 0, and
// clamp(min=0) passes the gradient at the boundary)
// ---------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ float adv_term(float a, float b) {
    if (OP == PM_ADV_ABS_DIFF) return fabsf(a - b);
    if (OP == PM_ADV_SQ_ONE_MINUS) { const float d = 1.f - a; return d * d; }
    if (OP == PM_ADV_SQ) return a * a;
    if (OP == PM_ADV_HINGE_ONE_MINUS) return pm_max_nan(1.f - a, 0.f);
    return pm_max_nan(1.f + a, 0.f);
}

// c = grad_out / numel; at most one multiplication that rounds (2 x is exact)
template <int OP>
__device__ __forceinline__ float adv_gradient(float a, float b, float c) {
    if (OP == PM_ADV_ABS_DIFF) {            // of b: -sign(a - b) c
        const float d = a - b;
        return d > 0.f ? -c : (d < 0.f ? c : 0.f);
    }
    if (OP == PM_ADV_SQ_ONE_MINUS) return (2.f * (a - 1.f)) * c;
    if (OP == PM_ADV_SQ) return (2.f * a) * c;
    if (OP == PM_ADV_HINGE_ONE_MINUS) return 1.f - a >= 0.f ? -c : 0.f;
    return 1.f + a >= 0.f ? c : 0.f;
}

// ---------------------------------------------------------------------------
// Forward: one partial a workgroup
// ---------------------------------------------------------------------------

// A whole chunk of an aligned tensor: every load issued before the first add
template <int OP, typename T>
__device__ __forceinline__ float adv_sum_full(const AdvEntry& e,
                                              long long start) {
    float a[ADV_ROUNDS][ADV_VEC], b[ADV_ROUNDS][ADV_VEC];
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const long long at =
            start + (j * ADV_THREADS + (int)threadIdx.x) * ADV_VEC;
        AdvIo<T>::load8(e.a, at, a[j]);
        if (OP == PM_ADV_ABS_DIFF) AdvIo<T>::load8(e.b, at, b[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j)
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            sum += adv_term<OP>(a[j][i], OP == PM_ADV_ABS_DIFF ? b[j][i] : 0.f);
    return sum;
}

// The last chunk of a tensor and every chunk of one that is not aligned
template <int OP>
__device__ __forceinline__ float adv_sum_tail(const AdvEntry& e,
                                              long long start, int n) {
    float sum = 0.f;
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const int i0 = (j * ADV_THREADS + (int)threadIdx.x) * ADV_VEC;
        const int valid = n - i0;
        if (valid <= 0) break;
        const bool vector = e.aligned && valid >= ADV_VEC;
        float a[ADV_VEC], b[ADV_VEC];
        adv_load_any(e.a, e.dtype, vector, start + i0, valid, a);
        if (OP == PM_ADV_ABS_DIFF)
            adv_load_any(e.b, e.dtype, vector, start + i0, valid, b);
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            if (i < valid)
                sum += adv_term<OP>(a[i], OP == PM_ADV_ABS_DIFF ? b[i] : 0.f);
    }
    return sum;
}

template <int OP>
__device__ __forceinline__ float adv_sum(const AdvEntry& e, long long start,
                                         int n) {
    if (n == ADV_CHUNK && e.aligned) {
        if (e.dtype == PM_F32) return adv_sum_full<OP, float>(e, start);
        if (e.dtype == PM_F16) return adv_sum_full<OP, _Float16>(e, start);
        return adv_sum_full<OP, __bf16>(e, start);
    }
    return adv_sum_tail<OP>(e, start, n);
}

__global__ __launch_bounds__(ADV_THREADS) void adv_partials_kernel(
    AdvTable t, float* __restrict__ partials, AdvMeta* __restrict__ meta) {
    __shared__ float scratch[ADV_THREADS / 64];
    const int k = adv_find(t, blockIdx.x);
    const AdvEntry& e = t.e[k];
    const int chunk = blockIdx.x - e.first;
    const long long start = (long long)chunk * ADV_CHUNK;
    const long long left = e.numel - start;
    const int n = left < ADV_CHUNK ? (int)left : ADV_CHUNK;
    float sum;
    switch (e.op) {
    case PM_ADV_ABS_DIFF: sum = adv_sum<PM_ADV_ABS_DIFF>(e, start, n); break;
    case PM_ADV_SQ_ONE_MINUS:
        sum = adv_sum<PM_ADV_SQ_ONE_MINUS>(e, start, n); break;
    case PM_ADV_SQ: sum = adv_sum<PM_ADV_SQ>(e, start, n); break;
    case PM_ADV_HINGE_ONE_MINUS:
        sum = adv_sum<PM_ADV_HINGE_ONE_MINUS>(e, start, n); break;
    default: sum = adv_sum<PM_ADV_HINGE_ONE_PLUS>(e, start, n); break;
    }
    sum = adv_block_sum(sum, scratch);
    if (threadIdx.x == 0) {
        partials[t.base + blockIdx.x] = sum;
        if (chunk == 0) {
            AdvMeta m;
            m.numel = e.numel;
            m.first = t.base + e.first;
            meta[t.index0 + k] = m;
        }
    }
}

// ---------------------------------------------------------------------------
// The final pass, one workgroup (adv_ordered_sum: pm_multi.h)
// ---------------------------------------------------------------------------

// out (count + 1): mean_k = the partials of entry k summed in ascending order
// in double, over numel in double, rounded once; then the total: the double
// means summed in list order, rounded once. One wave an entry.
__global__ __launch_bounds__(ADV_FINAL_THREADS) void adv_final_kernel(
    const float* __restrict__ partials, const AdvMeta* __restrict__ meta,
    double* wide, int count, float* __restrict__ out) {
    const int wave = threadIdx.x >> 6;
    for (int k = wave; k < count; k += ADV_FINAL_THREADS / 64) {
        const AdvMeta m = meta[k];
        const long long chunks = (m.numel + ADV_CHUNK - 1) / ADV_CHUNK;
        const double mean =
            adv_ordered_sum(partials + m.first, chunks) / (double)m.numel;
        if ((threadIdx.x & 63) == 0) {
            wide[k] = mean;
            out[k] = (float)mean;
        }
    }
    __threadfence();
    __syncthreads();
    __threadfence();
    if (wave == 0) {
        const double total = adv_ordered_sum((const double*)wide, count);
        if (threadIdx.x == 0) out[count] = (float)total;
    }
}

// ---------------------------------------------------------------------------
// Backward: grad[i] = (grad_out / numel) * d op / d input, in the input's dtype
// ---------------------------------------------------------------------------
template <int OP, typename T>
__device__ __forceinline__ void adv_backward_full(const AdvEntry& e,
                                                  long long start, float c) {
    float a[ADV_ROUNDS][ADV_VEC], b[ADV_ROUNDS][ADV_VEC];
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const long long at =
            start + (j * ADV_THREADS + (int)threadIdx.x) * ADV_VEC;
        AdvIo<T>::load8(e.a, at, a[j]);
        if (OP == PM_ADV_ABS_DIFF) AdvIo<T>::load8(e.b, at, b[j]);
    }
#pragma unroll
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const long long at =
            start + (j * ADV_THREADS + (int)threadIdx.x) * ADV_VEC;
        float g[ADV_VEC];
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            g[i] = adv_gradient<OP>(
                a[j][i], OP == PM_ADV_ABS_DIFF ? b[j][i] : 0.f, c);
        AdvIo<T>::store8(e.grad, at, g);
    }
}

template <int OP>
__device__ __forceinline__ void adv_backward_tail(const AdvEntry& e,
                                                  long long start, int n,
                                                  float c) {
    for (int j = 0; j < ADV_ROUNDS; ++j) {
        const int i0 = (j * ADV_THREADS + (int)threadIdx.x) * ADV_VEC;
        const int valid = n - i0;
        if (valid <= 0) break;
        const bool vector = e.aligned && valid >= ADV_VEC;
        float a[ADV_VEC], b[ADV_VEC], g[ADV_VEC];
        adv_load_any(e.a, e.dtype, vector, start + i0, valid, a);
        if (OP == PM_ADV_ABS_DIFF)
            adv_load_any(e.b, e.dtype, vector, start + i0, valid, b);
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            g[i] = adv_gradient<OP>(
                a[i], OP == PM_ADV_ABS_DIFF ? b[i] : 0.f, c);
        adv_store_any(e.grad, e.dtype, vector, start + i0, valid, g);
    }
}

template <int OP>
__device__ __forceinline__ void adv_backward(const AdvEntry& e,
                                             long long start, int n, float c) {
    if (n == ADV_CHUNK && e.aligned) {
        if (e.dtype == PM_F32) adv_backward_full<OP, float>(e, start, c);
        else if (e.dtype == PM_F16)
            adv_backward_full<OP, _Float16>(e, start, c);
        else adv_backward_full<OP, __bf16>(e, start, c);
    } else {
        adv_backward_tail<OP>(e, start, n, c);
    }
}

__global__ __launch_bounds__(ADV_THREADS) void adv_backward_kernel(
    AdvTable t, const float* __restrict__ grad_out) {
    const int k = adv_find(t, blockIdx.x);
    const AdvEntry& e = t.e[k];
    const int chunk = blockIdx.x - e.first;
    const long long start = (long long)chunk * ADV_CHUNK;
    const long long left = e.numel - start;
    const int n = left < ADV_CHUNK ? (int)left : ADV_CHUNK;
    const float c = grad_out[0] / (float)e.numel;
    switch (e.op) {
    case PM_ADV_ABS_DIFF:
        adv_backward<PM_ADV_ABS_DIFF>(e, start, n, c); break;
    case PM_ADV_SQ_ONE_MINUS:
        adv_backward<PM_ADV_SQ_ONE_MINUS>(e, start, n, c); break;
    case PM_ADV_SQ: adv_backward<PM_ADV_SQ>(e, start, n, c); break;
    case PM_ADV_HINGE_ONE_MINUS:
        adv_backward<PM_ADV_HINGE_ONE_MINUS>(e, start, n, c); break;
    default: adv_backward<PM_ADV_HINGE_ONE_PLUS>(e, start, n, c); break;
    }
}

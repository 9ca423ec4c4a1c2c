// What the multi-tensor passes share (pm_adv.h: the adversarial means;
// pm_optim.h: the optimizer step): the shape of a chunk, the loads and stores
// of 8 consecutive elements whose bits do not depend on the alignment, the
// fixed-order sum of a workgroup and the ordered double sum of the final
// pass. The order they fix is described in pm_adv.h.
#pragma once
#include <hip/hip_runtime.h>

#include "promonet_hip.h"

#define ADV_THREADS 256
#define ADV_VEC 8                       // elements a thread takes at once
#define ADV_ROUNDS 4
#define ADV_CHUNK (ADV_THREADS * ADV_VEC * ADV_ROUNDS)

typedef _Float16 adv_half8 __attribute__((ext_vector_type(8)));
typedef __bf16 adv_bf16x8 __attribute__((ext_vector_type(8)));

// The entry of a launch's table (e[count], each with its `first` workgroup)
// that a workgroup belongs to: the last one whose `first` is not past it
template <class Table>
__device__ __forceinline__ int adv_find(const Table& t, int group) {
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.e[mid].first <= group) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// Loads and stores of 8 consecutive elements from element `at` on
// ---------------------------------------------------------------------------
template <typename T> struct AdvIo;

template <> struct AdvIo<float> {
    __device__ static __forceinline__ void load8(const void* p, long long at,
                                                 float v[ADV_VEC]) {
        const float4* q = (const float4*)((const float*)p + at);
        const float4 x = q[0], y = q[1];
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
    }
    __device__ static __forceinline__ void store8(void* p, long long at,
                                                  const float v[ADV_VEC]) {
        float4* q = (float4*)((float*)p + at);
        q[0] = make_float4(v[0], v[1], v[2], v[3]);
        q[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
};

template <> struct AdvIo<_Float16> {
    __device__ static __forceinline__ void load8(const void* p, long long at,
                                                 float v[ADV_VEC]) {
        const adv_half8 x = *(const adv_half8*)((const _Float16*)p + at);
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i) v[i] = (float)x[i];
    }
    __device__ static __forceinline__ void store8(void* p, long long at,
                                                  const float v[ADV_VEC]) {
        adv_half8 x;
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i) x[i] = (_Float16)v[i];
        *(adv_half8*)((_Float16*)p + at) = x;
    }
};

template <> struct AdvIo<__bf16> {
    __device__ static __forceinline__ void load8(const void* p, long long at,
                                                 float v[ADV_VEC]) {
        const adv_bf16x8 x = *(const adv_bf16x8*)((const __bf16*)p + at);
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i) v[i] = (float)x[i];
    }
    __device__ static __forceinline__ void store8(void* p, long long at,
                                                  const float v[ADV_VEC]) {
        adv_bf16x8 x;
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i) x[i] = (__bf16)v[i];
        *(adv_bf16x8*)((__bf16*)p + at) = x;
    }
};

__device__ __forceinline__ float adv_load1(const void* p, int dtype,
                                           long long at) {
    if (dtype == PM_F32) return ((const float*)p)[at];
    if (dtype == PM_F16) return (float)((const _Float16*)p)[at];
    return (float)((const __bf16*)p)[at];
}

__device__ __forceinline__ void adv_store1(void* p, int dtype, long long at,
                                           float v) {
    if (dtype == PM_F32) ((float*)p)[at] = v;
    else if (dtype == PM_F16) ((_Float16*)p)[at] = (_Float16)v;
    else ((__bf16*)p)[at] = (__bf16)v;
}

// 8 elements of a chunk's tail, or of a tensor that is not aligned: as a
// vector where all 8 exist and the tensor is aligned, else one by one with 0
// past the end
__device__ __forceinline__ void adv_load_any(const void* p, int dtype,
                                             bool vector, long long at,
                                             int valid, float v[ADV_VEC]) {
    if (vector) {
        if (dtype == PM_F32) AdvIo<float>::load8(p, at, v);
        else if (dtype == PM_F16) AdvIo<_Float16>::load8(p, at, v);
        else AdvIo<__bf16>::load8(p, at, v);
    } else {
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            v[i] = i < valid ? adv_load1(p, dtype, at + i) : 0.f;
    }
}

__device__ __forceinline__ void adv_store_any(void* p, int dtype, bool vector,
                                              long long at, int valid,
                                              const float v[ADV_VEC]) {
    if (vector) {
        if (dtype == PM_F32) AdvIo<float>::store8(p, at, v);
        else if (dtype == PM_F16) AdvIo<_Float16>::store8(p, at, v);
        else AdvIo<__bf16>::store8(p, at, v);
    } else {
#pragma unroll
        for (int i = 0; i < ADV_VEC; ++i)
            if (i < valid) adv_store1(p, dtype, at + i, v[i]);
    }
}

// Sum over the workgroup in a fixed order (sc_block_sum of pm_stockham.h); the
// result is valid in thread 0.
__device__ __forceinline__ float adv_block_sum(float v, float* scratch) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float total = scratch[0];
    for (int w = 1; w < ADV_THREADS / 64; ++w) total += scratch[w];
    return total;
}

// ---------------------------------------------------------------------------
// The final pass, one workgroup. sum_{i < n} p[i] in ascending order in
// double, by a whole wave: 64 values a load, then each lane adds all 64 in
// order from the scalar registers (every lane holds the same sum).
// ---------------------------------------------------------------------------
__device__ __forceinline__ double adv_ordered_sum(const float* __restrict__ p,
                                                  long long n) {
    const int lane = threadIdx.x & 63;
    double sum = 0.;
    for (long long base = 0; base < n; base += 64) {
        // (+0 past the end: it changes no bit of a sum that starts at +0)
        const int v = base + lane < n ? __float_as_int(p[base + lane]) : 0;
#pragma unroll
        for (int i = 0; i < 64; ++i)
            sum += (double)__int_as_float(__builtin_amdgcn_readlane(v, i));
    }
    return sum;
}

__device__ __forceinline__ double adv_ordered_sum(const double* __restrict__ p,
                                                  long long n) {
    const int lane = threadIdx.x & 63;
    double sum = 0.;
    for (long long base = 0; base < n; base += 64) {
        const double v = base + lane < n ? p[base + lane] : 0.;
        const int hi = __double2hiint(v), lo = __double2loint(v);
#pragma unroll
        for (int i = 0; i < 64; ++i)
            sum += __hiloint2double(__builtin_amdgcn_readlane(hi, i),
                                    __builtin_amdgcn_readlane(lo, i));
    }
    return sum;
}

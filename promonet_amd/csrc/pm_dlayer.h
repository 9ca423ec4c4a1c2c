// What the conv layers' training kernels share (pm_fdisc.h, pm_dconv.h,
// pm_pconv.h, pm_gconv.h): the leaky activation and its gate, the fp32 MFMA
// step, the flattened pixels of a map (DlPixel walks a stride-1 layer,
// DlBatchPixel finds the batch row too), the span and the epilogue of the gW
// kernels that walk such pixels, and the reduce of the gW | gb partials. The
// gemm kernels of pm_pconv.h and pm_gconv.h share their weight chunk and their
// chains as well: pm_pixel_gemm.h. fp32 throughout; every kernel is a
// workgroup of DL_THREADS, which FD_THREADS, DC_THREADS, PC_THREADS and
// GC_THREADS equal.
#pragma once
#include <hip/hip_runtime.h>

#define DL_THREADS 256

typedef float dl_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float dl_leaky(float v, float slope) {
    return v > 0.f ? v : v * slope;
}
// upstream * leaky'(y): y = 0 takes the slope, as torch does
__device__ __forceinline__ float dl_gate(float g, float y, float slope) {
    return y > 0.f ? g : g * slope;
}
__device__ __forceinline__ float4 dl_gate4(float4 g, float4 y, float slope) {
    return make_float4(dl_gate(g.x, y.x, slope), dl_gate(g.y, y.y, slope),
                       dl_gate(g.z, y.z, slope), dl_gate(g.w, y.w, slope));
}
__device__ __forceinline__ float4 dl_leaky4(float4 v, float slope) {
    return make_float4(dl_leaky(v.x, slope), dl_leaky(v.y, slope),
                       dl_leaky(v.z, slope), dl_leaky(v.w, slope));
}

#define DL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)
// four K steps: the elements of a lane's 16-byte reads of A and B
#define DL_MFMA4(acc, a4, b4)                                               \
    do {                                                                    \
        acc = DL_MFMA((a4).x, (b4).x, acc);                                 \
        acc = DL_MFMA((a4).y, (b4).y, acc);                                 \
        acc = DL_MFMA((a4).z, (b4).z, acc);                                 \
        acc = DL_MFMA((a4).w, (b4).w, acc);                                 \
    } while (0)

// ---------------------------------------------------------------------------
// A pixel p = (b H + h) W + w of the flattened map of a stride-1 layer, and
// where its taps fall: the tap (dh, dw) is the pixel p + dl_offset(dh, dw, W)
// where (h + dh, w + dw) lies inside the map. 32-bit arithmetic: the host
// refuses more than 2^31 - 1 pixels (a 64-bit division a pixel cost more than
// the MFMAs of a gW step).
// ---------------------------------------------------------------------------
struct DlPixel {
    int h, w;
    __device__ __forceinline__ DlPixel(long long p, int H, int W) {
        const unsigned row = (unsigned)p / (unsigned)W;
        w = (int)((unsigned)p - row * (unsigned)W);
        h = (int)(row % (unsigned)H);
    }
    // the pixel n (< 2^16) further on
    __device__ __forceinline__ void advance(int n, int H, int W) {
        w += n;
        while (w >= W) {
            w -= W;
            if (++h == H) h = 0;
        }
    }
    // is the pixel (h + sign dh, w + sign dw) inside? SIGN = -1 mirrors the
    // tap (an input gradient reads gz at p - offset)
    __device__ __forceinline__ bool inside(int dh, int dw, int H, int W,
                                           int sign = 1) const {
        const int hh = h + sign * dh, ww = w + sign * dw;
        return hh >= 0 && hh < H && ww >= 0 && ww < W;
    }
};
// (b, h, w) of the pixel p of a flattened (B, H, W) map, for the kernels of
// the strided layers: their taps lie in another map, which the batch row finds
// (the audio, in the period discriminator's first layer). Apart from DlPixel:
// the kernels that use that one read no b, and none of these walks. The same
// 32-bit arithmetic.
struct DlBatchPixel {
    int b, h, w;
    __device__ __forceinline__ DlBatchPixel(long long p, int H, int W) {
        const unsigned row = (unsigned)p / (unsigned)W;
        w = (int)((unsigned)p - row * (unsigned)W);
        h = (int)(row % (unsigned)H);
        b = (int)(row / (unsigned)H);
    }
};
// (dh in 64 bits: a dilated tap's d T may leave 32)
__device__ __forceinline__ long long dl_offset(long long dh, int dw,
                                               int W) {
    return dh * W + dw;
}

// ---------------------------------------------------------------------------
// gW and gb over flattened pixels (fd_gw_kernel, dc_gw_edge_kernel): MFMA
// tiles with K = pixels, four pixels a step. Workgroup blockIdx.x takes the
// pixels blockIdx.x * span ... + span (span = 16 n), a wave a quarter.
// ---------------------------------------------------------------------------
// The first pixel of a wave and its steps of four pixels, the same for every
// lane of the wave; a lane beyond the last pixel stays beyond it
struct DlGwSpan { long long begin; int steps; };
__device__ __forceinline__ DlGwSpan dl_gw_span(long long P, int span,
                                               int wave) {
    const long long begin = (long long)blockIdx.x * span + wave * (span / 4);
    const long long left = P - begin;
    const int steps = left <= 0 ? 0
        : (int)(left < span / 4 ? (left + 3) / 4 : span / 16);
    return {begin, steps};
}

// The G::NM accumulator tiles of the four waves, added in order, to the
// partial of this workgroup: G::slot(m, i, j) is where row i, column j of
// tile m goes in the G::N floats of a partial, or -1. Every float of the
// partial is written by exactly one thread (the slots are distinct).
template <class G>
__device__ __forceinline__ void dl_gw_store(const dl_f4 (&acc)[G::NM],
                                            float* parts) {
    __shared__ float lds[DL_THREADS / 64][G::NM][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < G::NM; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[wave][m][r][lane] = acc[m][r];
    __syncthreads();
    float* part = parts + (long long)blockIdx.x * G::N;
    for (int e = threadIdx.x; e < G::NM * 256; e += DL_THREADS) {
        const int m = e >> 8, r = (e >> 6) & 3, l = e & 63;
        const int slot = G::slot(m, 4 * (l >> 4) + r, l & 15);
        if (slot < 0) continue;
        float sum = lds[0][m][r][l];
        for (int w = 1; w < DL_THREADS / 64; ++w) sum += lds[w][m][r][l];
        part[slot] = sum;
    }
}

// ---------------------------------------------------------------------------
// gW | gb = the `nparts` partials of `n` floats added in a fixed order, in
// double: 64 entries a workgroup, each wave a quarter of the partials in
// ascending order (eight loads in flight), then the four waves in order. The
// first `weights` entries are gW, the others gb. Internal linkage: every .hip
// that launches it (dl_reduce) has its own copy.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(DL_THREADS) void dl_reduce_kernel(
    const float* __restrict__ parts, int nparts, long long n,
    long long weights, float* __restrict__ grad_weight,
    float* __restrict__ grad_bias) {
    __shared__ double lds[DL_THREADS / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * 64 + lane;
    const int per = (nparts + DL_THREADS / 64 - 1) / (DL_THREADS / 64);
    const int first = wave * per;
    const int last = first + per < nparts ? first + per : nparts;
    double sum = 0.;
    if (e < n) {
        int p = first;
        for (; p + 8 <= last; p += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = parts[(long long)(p + u) * n + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += (double)v[u];
        }
        for (; p < last; ++p) sum += (double)parts[(long long)p * n + e];
    }
    lds[wave][lane] = sum;
    __syncthreads();
    if (wave != 0 || e >= n) return;
    for (int w = 1; w < DL_THREADS / 64; ++w) sum += lds[w][lane];
    if (e < weights) grad_weight[e] = (float)sum;
    else grad_bias[e - weights] = (float)sum;
}

// The tail of a layer's backward: gW (n - out_channels floats) | gb
// (out_channels) from the partials its gW kernel left in the workspace
static inline hipError_t dl_reduce(const float* parts, int nparts, long long n,
                                   int out_channels, float* grad_weight,
                                   float* grad_bias, hipStream_t s) {
    hipLaunchKernelGGL(dl_reduce_kernel, dim3((unsigned)((n + 63) / 64)),
                       dim3(DL_THREADS), 0, s, parts, nparts, n,
                       n - out_channels, grad_weight, grad_bias);
    return hipGetLastError();
}

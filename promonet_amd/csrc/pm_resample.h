// Polyphase windowed-sinc resampling on the device: replaces the host conv1d
// of torchaudio.functional.resample ('sinc_interp_hann') behind
// promonet/load.py:16-28 and promonet/baseline/mels.py:174-.
//
//   out[row][q new + p] = sum_k bank[p][k] x[row][q orig + k - width]
//
// with x = 0 outside [0, len(row)) and out = 0 from ceil(new len / orig) on.
// Every output is ONE fp32 accumulator and an fma chain over k = 0 .. taps - 1
// in ascending order, so its bits depend on its row's samples and its own
// index only: not on the tile it falls in, the row's place in the batch, the
// vector width of the LDS reads or whether lengths were given.
//
// A workgroup takes RS_CHAINS * groups consecutive strides q of one row and
// stages that input segment once in LDS, zero-filled outside the row. A
// thread owns RS_PHASES phases (p, p + ceil(new / RS_PHASES)) and RS_CHAINS
// strides `groups` apart, a register tile of RS_PHASES x RS_CHAINS
// independent chains: a bank load (lanes = consecutive p of the transposed
// bank: coalesced, from L2) feeds RS_CHAINS of them, an LDS read (lanes of
// one stride read the same word: a broadcast) RS_PHASES. V = the widest of
// 4 / 2 / 1 floats that divides `orig`: a stride's segment then starts
// V-aligned and V taps come from one ds_read_b128 / _b64. A filter whose
// segment does not fit RS_LDS_FLOATS is refused (no standard rate pair).
#pragma once
#include <hip/hip_runtime.h>

#define RS_THREADS 256
#ifndef RS_CHAINS
#define RS_CHAINS 4         // strides (independent fma chains) per thread ...
#endif
#ifndef RS_PHASES
#define RS_PHASES 2         // ... times phases per thread (1 when new == 1)
#endif
#ifndef RS_UNROLL
#define RS_UNROLL 2         // V-tap steps in flight
#endif
#define RS_SLOTS 1024       // (phase, stride group) slots a workgroup aims at
#define RS_LDS_FLOATS 8192  // staged segment, 32 KiB at most: 4 workgroups a CU

struct ResampleArgs {
    const float* x;
    const int* lengths;     // NULL: every row has n_in
    const float* bank;      // (taps, new): bank[k * new + p]
    float* out;
    long long x_stride, out_stride;
    int n_in, n_out, orig, new_, width, taps;
    int groups;             // stride groups per workgroup (RS_CHAINS strides each)
    int half;               // ceil(new / phases per thread)
    int tiles;              // workgroups per row
};

static inline int pm_resample_phases(int new_) {
    return new_ < RS_PHASES ? 1 : RS_PHASES;
}

static_assert(RS_LDS_FLOATS * sizeof(float) <= 48 * 1024,
              "the segment must fit the LDS a launch gets without an opt-in");

// Strides per workgroup = RS_CHAINS * groups; 0: the segment of even one
// group does not fit LDS
static inline int pm_resample_groups(int orig, int new_, int width) {
    const long long taps = 2ll * width + orig;
    const int phases = pm_resample_phases(new_);
    const int half = (new_ + phases - 1) / phases;
    long long groups = RS_SLOTS / half > 1 ? RS_SLOTS / half : 1;
    if (taps > RS_LDS_FLOATS) return 0;
    const long long fit = ((RS_LDS_FLOATS - taps) / orig + 1) / RS_CHAINS;
    return (int)(fit < groups ? fit : groups);
}

template <int V, int P>
__global__ __launch_bounds__(RS_THREADS) void pm_resample_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_x[];
    const int t = threadIdx.x;
    const int tile = blockIdx.x % a.tiles;
    const int row = blockIdx.x / a.tiles;
    int len = a.lengths ? a.lengths[row] : a.n_in;
    len = len < 0 ? 0 : (len > a.n_in ? a.n_in : len);
    const long long out_len = ((long long)a.new_ * len + a.orig - 1) / a.orig;
    const int strides = a.groups * RS_CHAINS;
    const long long tile_out = (long long)strides * a.new_;
    const long long n0 = (long long)tile * tile_out;
    float* __restrict__ o = a.out + (long long)row * a.out_stride;
    if (n0 >= out_len) {            // past the row: only the zero tail
        long long end = n0 + tile_out;
        if (end > a.n_out) end = a.n_out;
        for (long long n = n0 + t; n < end; n += RS_THREADS) o[n] = 0.f;
        return;
    }
    const float* __restrict__ x = a.x + (long long)row * a.x_stride;
    const long long i0 = (long long)tile * strides * a.orig - a.width;
    const int segment = (strides - 1) * a.orig + a.taps;
    for (int l = t; l < segment; l += RS_THREADS) {
        const long long i = i0 + l;
        float v = 0.f;
        if (i >= 0 && i < len) v = x[i];
        rs_x[l] = v;
    }
    __syncthreads();
    const int slots = a.groups * a.half;
    for (int s = t; s < slots; s += RS_THREADS) {
        const int p = s % a.half;
        const int g = s / a.half;
        // phases p, p + half, ...; one past the last repeats p and is not
        // written. The phases of a thread are the lanes of one packed fma
        // (v_pk_fma_f32: the sample broadcast, the taps a register pair).
        typedef float phases_t __attribute__((ext_vector_type(P)));
        unsigned column[P];
        bool live[P];
        phases_t acc[RS_CHAINS];
        int off[RS_CHAINS];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            live[i] = p + i * a.half < a.new_;
            column[i] = 4u * (live[i] ? p + i * a.half : p);   // bytes
        }
#pragma unroll
        for (int j = 0; j < RS_CHAINS; ++j) {
            acc[j] = (phases_t)(0.f);
            off[j] = (g + j * a.groups) * a.orig;
        }
        int k = 0;
        if constexpr (V > 1) {
            // (without the assumed alignment the reads come out as pairs of
            // ds_read2_b32, at twice the LDS cycles)
#pragma unroll RS_UNROLL
            for (; k + V <= a.taps; k += V) {
                phases_t w[V > 1 ? V : 1];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    // a uniform row base: scalar address + 32-bit lane offset
                    const char* __restrict__ taps_k =
                        (const char*)(a.bank + (size_t)(k + v) * a.new_);
#pragma unroll
                    for (int i = 0; i < P; ++i)
                        w[v][i] = *(const float*)(taps_k + column[i]);
                }
#pragma unroll
                for (int j = 0; j < RS_CHAINS; ++j) {
                    float xv[V > 1 ? V : 1];
                    if constexpr (V == 4) {
                        const float4 q = *(const float4*)__builtin_assume_aligned(
                            &rs_x[off[j] + k], 16);
                        xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
                    } else {
                        const float2 q = *(const float2*)__builtin_assume_aligned(
                            &rs_x[off[j] + k], 8);
                        xv[0] = q.x; xv[1] = q.y;
                    }
#pragma unroll
                    for (int v = 0; v < V; ++v)
                        acc[j] = __builtin_elementwise_fma(
                            w[v], (phases_t)(xv[v]), acc[j]);
                }
            }
        }
        constexpr int TAIL = V > 1 ? 1 : 4;   // V > 1: the taps % V left over
#pragma unroll TAIL
        for (; k < a.taps; ++k) {
            const char* __restrict__ taps_k =
                (const char*)(a.bank + (size_t)k * a.new_);
            phases_t w;
#pragma unroll
            for (int i = 0; i < P; ++i)
                w[i] = *(const float*)(taps_k + column[i]);
#pragma unroll
            for (int j = 0; j < RS_CHAINS; ++j) {
                const float v = rs_x[off[j] + k];
                acc[j] = __builtin_elementwise_fma(w, (phases_t)(v), acc[j]);
            }
        }
#pragma unroll
        for (int i = 0; i < P; ++i) {
            if (!live[i]) continue;
#pragma unroll
            for (int j = 0; j < RS_CHAINS; ++j) {
                const long long n = n0 +
                    (long long)(g + j * a.groups) * a.new_ + p + i * a.half;
                if (n < out_len) o[n] = acc[j][i];
                else if (n < a.n_out) o[n] = 0.f;
            }
        }
    }
}

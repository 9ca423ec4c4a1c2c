// Batched Viterbi decoding on the device (promonet_amd.viterbi; the decoder
// torbi.from_probabilities is to promonet/preprocess/harmonics.py:270-276).
//
//   d_0[j] = B[0][j] + p[j]
//   m_t[j] = the i that maximises d_{t-1}[i] + A[j][i]          (t >= 1)
//   d_t[j] = B[t][j] + (d_{t-1}[m] + A[j][m])
//
// every sum ONE fp32 add in that association, every maximum with ties to the
// lowest index, the tie of all -inf included. The result is a pure function
// of the fp32 inputs: it does not depend on the lane a candidate falls in.
//
// One workgroup per utterance. d ping-pongs in LDS (2 x S floats). The
// transition arrives banded: row j (the NEXT state) holds A[j][lo_j .. lo_j +
// count_j) contiguous, padded with -inf to a multiple of 4 floats, so a lane
// takes a float4 of four consecutive i; whatever lies outside the band is
// -inf and can never beat the start value (-inf, 0) under a strict ">". A
// wave owns blocks of VT_ROWS consecutive rows, dealt to the waves there and
// back again so that a band that widens with j (the harmonic one) spreads
// evenly; lane r of the wave keeps row r's result, and the block's d and
// back-pointers (int16) leave in one coalesced store each. (value, index)
// pairs reduce with "greater value, or equal value and lower index". The
// back-trace is the last phase of the same launch, by one thread; the other
// threads write the zeros past the row's length. `lengths` is read here and
// nowhere on the host.
#pragma once
#include <hip/hip_runtime.h>

#define VT_THREADS 1024
#define VT_WAVES (VT_THREADS / 64)
#define VT_ROWS 32                  // rows per block of a wave (<= 64)
#define VT_MAX_STATES 32767         // back-pointers are int16
#define VT_LDS_BYTES (64 * 1024)    // what a launch gets without an opt-in

struct ViterbiArgs {
    const float* obs;       // (B, T, S) log observation
    const int* lengths;     // (B) or NULL: every row has T frames
    const float* band;      // packed rows of the log transition
    const int* table;       // (3, S): lo, count, offset (floats, multiple of 4)
    const float* initial;   // (S) log initial
    short* bp;              // (B, T, S) back-pointers (workspace)
    int* out;               // (B, T)
    long long band_floats;
    int T, S;
};

// d arrays hold S floats and at least 3 of padding (-inf) for the last float4
static inline int pm_viterbi_padded(int S) { return (S + 7) & ~3; }
static inline size_t pm_viterbi_lds(int S) {
    return 2 * (size_t)pm_viterbi_padded(S) * sizeof(float);
}

struct VtBest {
    float v;
    int i;
};

__device__ __forceinline__ VtBest vt_better(VtBest a, VtBest b) {
    const bool take = b.v > a.v || (b.v == a.v && b.i < a.i);
    return take ? b : a;
}

__device__ __forceinline__ VtBest vt_wave_reduce(VtBest a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        VtBest b;
        b.v = __shfl_xor(a.v, m, 64);
        b.i = __shfl_xor(a.i, m, 64);
        a = vt_better(a, b);
    }
    return a;
}

__global__ __launch_bounds__(VT_THREADS) void pm_viterbi_kernel(ViterbiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float vt_d[];
    __shared__ float vt_wave_v[VT_WAVES];
    __shared__ int vt_wave_i[VT_WAVES];
    const int S = a.S, T = a.T;
    const int SP = (S + 7) & ~3;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row = blockIdx.x;
    int len = a.lengths ? a.lengths[row] : T;
    len = len < 0 ? 0 : (len > T ? T : len);
    int* __restrict__ out = a.out + (long long)row * T;
    for (int f = len + t; f < T; f += VT_THREADS) out[f] = 0;
    if (len == 0) return;
    const float* __restrict__ obs = a.obs + (long long)row * T * S;
    short* __restrict__ bp = a.bp + (long long)row * T * S;
    const float ninf = -__builtin_inff();

    for (int j = t; j < SP; j += VT_THREADS) {
        vt_d[j] = j < S ? obs[j] + a.initial[j] : ninf;
        vt_d[SP + j] = ninf;
    }
    __syncthreads();

    const int blocks = (S + VT_ROWS - 1) / VT_ROWS;
    for (int f = 1; f < len; ++f) {
        const float* __restrict__ cur = vt_d + ((f - 1) & 1) * SP;
        float* __restrict__ nxt = vt_d + (f & 1) * SP;
        const float* __restrict__ b_f = obs + (long long)f * S;
        short* __restrict__ bp_f = bp + (long long)f * S;
        // blocks 0 .. 2 W - 1 go to waves 0 .. W - 1, W - 1 .. 0, and so on
        for (int round = 0; round * VT_WAVES < blocks; ++round) {
            const int block = round * VT_WAVES +
                ((round & 1) ? VT_WAVES - 1 - wave : wave);
            if (block >= blocks) continue;
            const int j0 = block * VT_ROWS;
            VtBest keep = {ninf, 0};
            for (int r = 0; r < VT_ROWS && j0 + r < S; ++r) {
                const int j = j0 + r;
                int lo = a.table[j], count = a.table[S + j];
                const long long offset = a.table[2 * S + j];
                // a table that points outside the band or the states reads
                // nothing (the host packs them in range; this is the fence)
                lo = lo < 0 ? 0 : (lo > S ? S : lo);
                count = count < 0 ? 0 : (count > S - lo ? S - lo : count);
                const int quads = (count + 3) >> 2;
                if (offset < 0 || (offset & 3) ||
                    offset + 4ll * quads > a.band_floats)
                    count = 0;
                const float4* __restrict__ w4 =
                    (const float4*)(a.band + offset);
                VtBest best = {ninf, 0};
                for (int q = lane; q < (count ? quads : 0); q += 64) {
                    const float4 w = w4[q];
                    const int i = lo + 4 * q;
                    const float c0 = cur[i] + w.x;
                    const float c1 = cur[i + 1] + w.y;
                    const float c2 = cur[i + 2] + w.z;
                    const float c3 = cur[i + 3] + w.w;
                    if (c0 > best.v) { best.v = c0; best.i = i; }
                    if (c1 > best.v) { best.v = c1; best.i = i + 1; }
                    if (c2 > best.v) { best.v = c2; best.i = i + 2; }
                    if (c3 > best.v) { best.v = c3; best.i = i + 3; }
                }
                best = vt_wave_reduce(best);
                if (lane == r) keep = best;
            }
            const int j = j0 + lane;
            if (lane < VT_ROWS && j < S) {
                nxt[j] = b_f[j] + keep.v;
                bp_f[j] = (short)keep.i;
            }
        }
        __syncthreads();
    }

    // the last state: argmax of d_{len-1}, ties to the lowest index
    const float* __restrict__ last = vt_d + ((len - 1) & 1) * SP;
    VtBest best = {ninf, 0};
    for (int j = t; j < S; j += VT_THREADS) {
        const float v = last[j];
        if (v > best.v) { best.v = v; best.i = j; }
    }
    best = vt_wave_reduce(best);
    if (lane == 0) { vt_wave_v[wave] = best.v; vt_wave_i[wave] = best.i; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < VT_WAVES; ++w) {
            VtBest other = {vt_wave_v[w], vt_wave_i[w]};
            best = vt_better(best, other);
        }
        int state = best.i;
        out[len - 1] = state;
        for (int f = len - 1; f >= 1; --f) {
            state = bp[(long long)f * S + state];
            // (states come from this launch: 0 <= state < S)
            out[f - 1] = state;
        }
    }
}

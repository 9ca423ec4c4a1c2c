// HiFi-GAN streaming by overlap-save: the two kernels
// around the engine's unchanged forward. A streaming call synthesises a WINDOW of frames - the history the
// receptive field asks for, then the new chunk - and emits the audio of the
// frames whose whole receptive field lies inside the window (or past a true
// end of the utterance, where the convolutions' zero padding is the truth).
#pragma once
#include <hip/hip_runtime.h>

#include "pm_host.h"

#define PM_STREAM_THREADS 256

// ---------------------------------------------------------------------------
// next (B, keep + c, Cpad) = [ last `keep` frames of prev (B, prev_frames,
// Cpad) | chunk ], one thread per 16 bytes of a row of `next`. The chunk is
// channels-last (B, c, Cpad) - a 16-byte load - or channels-first (B, C, c),
// transposed here: four strided loads, channels >= C written as zero. `prev`
// and `next` are different buffers: no thread reads what another writes.
// ---------------------------------------------------------------------------
struct StreamWindowArgs {
    const float* prev; const float* chunk; float* next;
    int prev_frames, keep, c, C, Cpad, chunk_cl;
    long long quads;         // B * (keep + c) * Cpad / 4
};

__global__ __launch_bounds__(PM_STREAM_THREADS) void pm_stream_window_kernel(
    StreamWindowArgs a) {
    const long long i =
        (long long)blockIdx.x * PM_STREAM_THREADS + threadIdx.x;
    if (i >= a.quads) return;
    const int per_row = a.Cpad >> 2;
    const int W = a.keep + a.c;
    const int q = (int)(i % per_row);
    const long long row = i / per_row;
    const int t = (int)(row % W);
    const long long b = row / W;
    float4 v;
    if (t < a.keep) {
        const long long src = (b * a.prev_frames + (a.prev_frames - a.keep + t))
            * per_row + q;
        v = ((const float4*)a.prev)[src];
    } else if (a.chunk_cl) {
        v = ((const float4*)a.chunk)[(b * a.c + (t - a.keep)) * per_row + q];
    } else {
        const int ch = q << 2;
        const float* p = a.chunk + (b * a.C + ch) * a.c + (t - a.keep);
        v.x = ch < a.C ? p[0] : 0.f;
        v.y = ch + 1 < a.C ? p[a.c] : 0.f;
        v.z = ch + 2 < a.C ? p[2 * (long long)a.c] : 0.f;
        v.w = ch + 3 < a.C ? p[3 * (long long)a.c] : 0.f;
    }
    ((float4*)a.next)[i] = v;
}

// ---------------------------------------------------------------------------
// out (B, n) = audio (B, window_samples)[:, first : first + n]: the emitted
// frames of the window's audio. VEC = 4: 16 bytes per thread (first, n,
// window_samples multiples of 4, both pointers 16-byte aligned); VEC = 1
// otherwise.
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(PM_STREAM_THREADS) void pm_stream_emit_kernel(
    const float* __restrict__ audio, float* __restrict__ out,
    long long window_samples, long long first, long long n, long long total) {
    const long long i =
        (long long)blockIdx.x * PM_STREAM_THREADS + threadIdx.x;
    if (i >= total) return;                 // total = B * n / VEC
    const long long per_row = n / VEC;
    const long long b = i / per_row, j = (i % per_row) * VEC;
    const float* src = audio + b * window_samples + first + j;
    float* dst = out + b * n + j;
    if (VEC == 4) *(float4*)dst = *(const float4*)src;
    else *dst = *src;
}

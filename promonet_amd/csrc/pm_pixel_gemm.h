// What the implicit-GEMM kernels of the period discriminator (pc_gemm_kernel,
// pm_pconv.h) and of the generator's Block convs (gc_gemm_kernel, pm_gconv.h)
// share: their weight is (O, C, K) with the taps innermost and their K chunk
// is 32 channels, so they load and stage the chunk of the weight alike
// (pg_weight_load, pg_weight_store: a layer gives the tap -> slot rule), and
// they split the sum of an output into the same four chains (PgChains). What
// was tried beyond that and is not shared, the chunk loop and the gW body,
// cost registers or time: profiles/pixel_gemm/NOTES.md.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_dlayer.h"

// ---------------------------------------------------------------------------
// The chunk of the weight W (O, C, K) of a tile of the forward (GX false: MT
// rows o from m0, the KC contracted channels from c0) or of gx (GX true: MT
// rows c from m0, the KC contracted o from c0, read transposed): runs of (KC
// or MT channels) x K taps, contiguous in W, a float4 at a time; staged as
// wl[slot][MT rows][PITCH], slot_of(tap) being the slot of a tap or -1.
// ---------------------------------------------------------------------------
template <int K, int MT, int KC> constexpr int pg_weight_vecs() {
    static_assert(MT * KC * K % (4 * DL_THREADS) == 0, "whole float4s");
    return MT * KC * K / 4 / DL_THREADS;
}

template <bool GX, int K, int MT, int KC, int AV>
__device__ __forceinline__ void pg_weight_load(float4 (&ar)[AV],
                                               const float* __restrict__ w,
                                               int C, int m0, int c0) {
    static_assert(AV == pg_weight_vecs<K, MT, KC>(), "the chunk's float4s");
    constexpr int RUN = (GX ? MT : KC) * K / 4;     // float4s of a run
#pragma unroll
    for (int u = 0; u < AV; ++u) {
        const int idx = threadIdx.x + u * DL_THREADS;
        const int outer = idx / RUN, f = idx % RUN;
        // row o: the chunk's channels x the taps; contracted o: the tile's
        // rows c x the taps
        const long long o = GX ? c0 + outer : m0 + outer;
        ar[u] = *(const float4*)(w + (o * C + (GX ? m0 : c0)) * K + 4 * f);
    }
}

template <bool GX, int K, int MT, int KC, int PITCH, int AV, class Slot>
__device__ __forceinline__ void pg_weight_store(const float4 (&ar)[AV],
                                                float* wl,
                                                const Slot& slot_of) {
    static_assert(AV == pg_weight_vecs<K, MT, KC>(), "the chunk's float4s");
    constexpr int RUN = (GX ? MT : KC) * K / 4;
#pragma unroll
    for (int u = 0; u < AV; ++u) {
        const int idx = threadIdx.x + u * DL_THREADS;
        const float v[4] = {ar[u].x, ar[u].y, ar[u].z, ar[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int outer = idx / RUN, jj = 4 * (idx % RUN) + e;
            const int row = GX ? jj / K : outer, con = GX ? outer : jj / K;
            const int slot = slot_of(jj % K);
            if (slot >= 0) wl[(slot * MT + row) * PITCH + con] = v[e];
        }
    }
}

// ---------------------------------------------------------------------------
// The sum of an output over K, split by chunk parity and channel half into
// four chains a row tile, added pairwise: [chunk parity][row tile][channel
// half]. step() hands the chains of a chunk to its MFMAs. (Zeroed by the
// initialiser, not in a constructor: profiles/pixel_gemm/NOTES.md.)
// ---------------------------------------------------------------------------
template <int MM> struct PgChains {
    dl_f4 acc[2][MM][2] = {};
    template <class Mma>
    __device__ __forceinline__ void step(int chunk, Mma mma) {
        if (chunk & 1) mma(acc[1]);
        else mma(acc[0]);
    }
    __device__ __forceinline__ dl_f4 sum(int m) const {
        return (acc[0][m][0] + acc[0][m][1]) + (acc[1][m][0] + acc[1][m][1]);
    }
};

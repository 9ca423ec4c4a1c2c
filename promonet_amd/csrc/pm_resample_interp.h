// Arbitrary-ratio resampling on the device: ONE long windowed-sinc table read
// with linear interpolation at a per-output phase (the structure of resampy's
// resample_f), where pm_resample.h needs a polyphase bank of `new` filters.
// Replaces the resampy.resample calls of promonet/data/augment/{pitch,
// loudness}.py. The contract is stated in include/promonet_hip.h; in short,
// for output t of a row with rates (orig, new), all in integers:
//
//   n = t orig div new, rem = t orig mod new, D = max(orig, new)
//   off = rem P div D,          eta  = fp32((rem P mod D) / D)
//   off' = (new - rem) P div D, eta' = fp32(((new - rem) P mod D) / D)
//   step = min(orig, new) P div orig
//   acc = 0
//   left:  i = 0 .. min(n + 1, (N + 1 - off) div step) - 1:
//            acc = fma(fma(eta, delta[off + i step], win[off + i step]),
//                      x[n - i], acc)
//   right: k = 0 .. min(len - n - 1, (N + 1 - off') div step) - 1:
//            the same with eta', off' and x[n + k + 1]
//
// One workgroup takes RI_TILE consecutive outputs of ONE row, so the rates
// are uniform, and stages the input segment those outputs reach once in LDS,
// zero-filled outside [0, len). A thread owns RI_CHAINS outputs RI_THREADS
// apart (coalesced stores): RI_CHAINS independent fma chains, each in the
// order above, so a sample's bits depend on its row's samples, its row's
// rates and its own index only. n and rem of the tile's first output come
// from one 64-bit division; a lane steps from there in 32 bits, which is why
// rates stay below RI_RATE_MAX. off' and eta' need no second division:
// new P = step D + r0, so (new - rem) P = (step - off) D + (r0 - m) with m =
// rem P mod D, borrowing one D when r0 < m.
//
// The tables (2 x 32 769 floats) do not fit LDS, and lanes read them at
// unrelated `off`: straight from memory every tap is two 64-lane gathers, and
// the L1's address processing, one lane at a time, is the whole run time
// (measured: 48 000 -> 22 050 ran 7 x slower per tap than 88 200 -> 44 100,
// whose lanes all share one phase). So the tables pass through LDS as well.
// At tap i every lane reads inside [i step, i step + P], whatever its phase:
// the workgroup walks a wing in chunks of C taps, copies the window
// [c C step, c C step + (C - 1) step + P] of both tables into LDS with
// coalesced loads, interleaved as (win, delta) pairs, and every lane gathers
// its C taps of every chain from there with one 8-byte LDS read a tap. Both
// wings walk the whole table, the left one first: one accumulator, the order
// of the contract. A chunk no chain of the workgroup reaches ends the walk;
// a chunk every chain of a wave takes whole runs without predicates.
//
// A row whose rates the kernel cannot take (not positive, RI_RATE_MAX or
// more, or a ratio whose segment does not fit RI_LDS_FLOATS) is answered with
// NaN in all of out[0, n_out): the rates are device data, so the host can
// refuse only what it is asked about (pm_resample_interp_tile).
#pragma once
#include <hip/hip_runtime.h>

#define RI_THREADS 256
#ifndef RI_CHAINS
#define RI_CHAINS 4             // outputs (independent fma chains) per thread
#endif
#define RI_TILE (RI_THREADS * RI_CHAINS)    // outputs per workgroup
#define RI_LDS_FLOATS 6144      // staged segment, 24 KiB: ratios from 1 / 5.3 up
#ifndef RI_WINDOW
#define RI_WINDOW 3072          // (win, delta) pairs of a table window, 24 KiB
#endif
#define RI_P 512                // table steps per zero crossing (precision 9)
#define RI_N (64 * RI_P)        // the tables hold RI_N + 1 entries
#define RI_RATE_MAX (1 << 21)   // (RI_TILE - 1) orig + new stays below 2^32

static_assert((unsigned long long)(RI_TILE - 1) * (RI_RATE_MAX - 1) +
              (RI_RATE_MAX - 1) < (1ull << 32), "a lane steps in 32 bits");
static_assert((unsigned long long)(RI_RATE_MAX - 1) * RI_P < (1ull << 32),
              "rem P stays in 32 bits");
static_assert((RI_LDS_FLOATS + 2 * RI_WINDOW) * sizeof(float) <= 48 * 1024,
              "segment and window: 3 workgroups in a CU's 160 KiB of LDS");
static_assert(RI_WINDOW > RI_P, "a window holds one tap of every phase");

struct ResampleInterpArgs {
    const float* x;
    const int* lengths;         // NULL: every row has n_in
    const int* orig;            // per row
    const int* new_;            // per row
    const float* win;           // RI_N + 1
    const float* delta;         // RI_N + 1
    float* out;
    long long x_stride, out_stride;
    int n_in, n_out, tiles;
};

// step = min(orig, new) P div orig: the table stride between two taps
__host__ __device__ static inline int pm_ri_step(int orig, int new_) {
    return (int)((long long)(orig < new_ ? orig : new_) * RI_P / orig);
}

// The most input samples a tile's outputs reach: their span of n and the
// longest wing, (N + 1) div step, either side. 0: the rates are refused.
__host__ __device__ static inline long long pm_ri_segment(int orig, int new_) {
    if (orig < 1 || new_ < 1 || orig >= RI_RATE_MAX || new_ >= RI_RATE_MAX)
        return 0;
    const int step = pm_ri_step(orig, new_);
    if (step < 1) return 0;
    const long long span =
        ((long long)(RI_TILE - 1) * orig + new_ - 1) / new_ + 1;
    const long long segment = span + 2 * ((RI_N + 1) / step);
    return segment > RI_LDS_FLOATS ? 0 : segment;
}

// One wing of every chain of a thread: DIR = -1 walks x[n - i] (left), DIR =
// 1 walks x[n + 1 + i]. A chain past its own count keeps its accumulator: its
// reads go to entry 0 and are dropped. `most` is the thread's longest count;
// the walk ends, for the whole workgroup at once, at the first chunk that no
// chain reaches.
template <int DIR>
__device__ __forceinline__ void pm_ri_wing(
    const ResampleInterpArgs& a, const float* ri_x, float2* ri_table,
    int step, const int (&off)[RI_CHAINS], const float (&eta)[RI_CHAINS],
    const int (&count)[RI_CHAINS], int most, const int (&pos)[RI_CHAINS],
    float (&acc)[RI_CHAINS]) {
    const int lane = threadIdx.x;
    const int chunk = (RI_WINDOW - RI_P - 1) / step + 1;    // taps a window
    const int need = (chunk - 1) * step + RI_P + 1;         // <= RI_WINDOW
    int least = count[0];
#pragma unroll
    for (int j = 1; j < RI_CHAINS; ++j)
        least = count[j] < least ? count[j] : least;
    for (int first = 0;; first += chunk) {
        // everyone is done with the window before; does anyone go on?
        if (!__syncthreads_or(first < most)) break;
        const int base = first * step;
        for (int e = lane; e < need; e += RI_THREADS) {
            const int at = base + e < RI_N ? base + e : RI_N;
            ri_table[e] = make_float2(a.win[at], a.delta[at]);
        }
        __syncthreads();
        if (__all(first + chunk <= least)) {
            // every chain of the wave takes the whole chunk: no predicates
            // (all of a row's interior; the counter pass of the predicated
            // loop alone showed it bound by VALU issue, 14 a tap)
            int ta[RI_CHAINS], xa[RI_CHAINS];
#pragma unroll
            for (int j = 0; j < RI_CHAINS; ++j) {
                ta[j] = off[j];
                xa[j] = DIR < 0 ? pos[j] - first : pos[j] + 1 + first;
            }
#pragma unroll 4
            for (int ii = 0; ii < chunk; ++ii) {
#pragma unroll
                for (int j = 0; j < RI_CHAINS; ++j) {
                    const float2 t = ri_table[ta[j]];
                    acc[j] = fmaf(fmaf(eta[j], t.y, t.x), ri_x[xa[j]], acc[j]);
                    ta[j] += step;
                    xa[j] += DIR;
                }
            }
            continue;
        }
#pragma unroll 2
        for (int ii = 0; ii < chunk; ++ii) {
            const int i = first + ii;
#pragma unroll
            for (int j = 0; j < RI_CHAINS; ++j) {
                const bool live = i < count[j];
                const float2 t = ri_table[live ? off[j] + ii * step : 0];
                const float w = fmaf(eta[j], t.y, t.x);
                const int at = DIR < 0 ? pos[j] - i : pos[j] + 1 + i;
                const float v = fmaf(w, ri_x[live ? at : 0], acc[j]);
                acc[j] = live ? v : acc[j];
            }
        }
    }
}

__global__ __launch_bounds__(RI_THREADS) void pm_resample_interp_kernel(
    ResampleInterpArgs a) {
    __shared__ float ri_x[RI_LDS_FLOATS];
    __shared__ float2 ri_table[RI_WINDOW];
    const int lane = threadIdx.x;
    const int tile = blockIdx.x % a.tiles;
    const int row = blockIdx.x / a.tiles;
    const long long t0 = (long long)tile * RI_TILE;
    float* __restrict__ o = a.out + (long long)row * a.out_stride;
    const int orig = a.orig[row], new_ = a.new_[row];
    if (pm_ri_segment(orig, new_) == 0) {       // refused: NaN, never a walk
        for (int j = 0; j < RI_CHAINS; ++j) {
            const long long t = t0 + lane + j * RI_THREADS;
            if (t < a.n_out) o[t] = __int_as_float(0x7fc00000);
        }
        return;
    }
    int len = a.lengths ? a.lengths[row] : a.n_in;
    len = len < 0 ? 0 : (len > a.n_in ? a.n_in : len);
    const long long out_len = (long long)len * new_ / orig;
    if (t0 >= out_len) {                        // past the row: the zero tail
        for (int j = 0; j < RI_CHAINS; ++j) {
            const long long t = t0 + lane + j * RI_THREADS;
            if (t < a.n_out) o[t] = 0.f;
        }
        return;
    }
    const unsigned uorig = (unsigned)orig, unew = (unsigned)new_;
    const unsigned D = uorig > unew ? uorig : unew;
    const int step = pm_ri_step(orig, new_);
    const int wing = (RI_N + 1) / step;
    // new P = step D + r0
    const unsigned r0 = (unsigned)((unsigned long long)unew * RI_P -
                                   (unsigned long long)step * D);
    const long long n0 = t0 * orig / new_;      // < len: fits an int
    const unsigned rem0 = (unsigned)(t0 * orig - n0 * new_);
    // segment: input samples lo .. lo + count - 1
    const long long lo = n0 - wing + 1;
    const int count =
        (int)((rem0 + (unsigned)(RI_TILE - 1) * uorig) / unew) + 2 * wing;
    const float* __restrict__ x = a.x + (long long)row * a.x_stride;
    for (int l = lane; l < count; l += RI_THREADS) {
        const long long i = lo + l;
        float v = 0.f;
        if (i >= 0 && i < len) v = x[i];
        ri_x[l] = v;
    }       // (the first barrier of pm_ri_wing publishes the segment)

    float acc[RI_CHAINS], eta[RI_CHAINS], eta2[RI_CHAINS];
    int off[RI_CHAINS], off2[RI_CHAINS], left[RI_CHAINS], right[RI_CHAINS];
    int pos[RI_CHAINS];                         // of x[n] in the segment
    int most_left = 0, most_right = 0;
    const float fD = (float)D;                  // exact: D < 2^21
#pragma unroll
    for (int j = 0; j < RI_CHAINS; ++j) {
        const unsigned k = (unsigned)(lane + j * RI_THREADS);
        const unsigned ahead = rem0 + k * uorig;
        const unsigned dn = ahead / unew;
        const unsigned rem = ahead - dn * unew;
        const long long n = n0 + dn;
        const unsigned scaled = rem * RI_P;
        const unsigned q = scaled / D;
        const unsigned m = scaled - q * D;
        off[j] = (int)q;
        eta[j] = __fdiv_rn((float)m, fD);
        const bool borrow = r0 < m;
        off2[j] = step - (int)q - (borrow ? 1 : 0);
        eta2[j] = __fdiv_rn((float)(borrow ? r0 + D - m : r0 - m), fD);
        const bool body = t0 + k < out_len;     // then n < len
        long long l = (RI_N + 1 - off[j]) / step;
        if (n + 1 < l) l = n + 1;
        long long r = (RI_N + 1 - off2[j]) / step;
        if (len - n - 1 < r) r = len - n - 1;
        left[j] = body ? (int)l : 0;
        right[j] = body ? (int)r : 0;
        pos[j] = body ? (int)(n - lo) : wing;
        most_left = left[j] > most_left ? left[j] : most_left;
        most_right = right[j] > most_right ? right[j] : most_right;
        acc[j] = 0.f;
    }
    pm_ri_wing<-1>(a, ri_x, ri_table, step, off, eta, left, most_left, pos,
                   acc);
    pm_ri_wing<1>(a, ri_x, ri_table, step, off2, eta2, right, most_right, pos,
                  acc);
#pragma unroll
    for (int j = 0; j < RI_CHAINS; ++j) {
        const long long t = t0 + lane + j * RI_THREADS;
        if (t < a.n_out) o[t] = t < out_len ? acc[j] : 0.f;
    }
}

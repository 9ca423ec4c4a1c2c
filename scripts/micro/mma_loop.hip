// Micro-benchmark (GPU box): the conv kernels' MFMA loop (mma_taps: weights
// L2 -> VGPR, activations LDS -> VGPR, software pipelined) in isolation, at one
// and two waves per SIMD. Separates "the loop cannot feed the matrix pipe"
// from "the phases around it leave the pipe idle".
// The first block of lines is the dominant kernel's exact shape (bf16, C = 128,
// k 11, 4 x 2 waves of 32 x 128, groups of 4 steps; random operands: zero data
// hides clock effects) with wave 0 of every workgroup stamping the shader
// clock (s_memtime) and the constant 100 MHz clock (s_memrealtime) around the
// loop: cycles per MFMA, the in-kernel clock, wall TFLOP/s - beside a
// register-resident MFMA loop (no operand stream) of the same run. Build once
// per issue order to compare them: -DPM_MMA_ORDER=0|1|2 (pm_conv.h).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -Iinclude \
//       scripts/micro/mma_loop.hip -o promonet_amd/lib/mma_loop
#include "../../promonet_amd/csrc/pm_conv.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// stamps[4 * workgroup + {0, 1}]: shader clocks, + {2, 3}: 100 MHz clock
template <class ET, int K, int WM, int WN, int NTW, int G = 4>
__global__ __launch_bounds__(WM * WN * 64) void loop_kernel(
    const typename ET::afrag_t* __restrict__ w,
    const typename ET::lds_t* __restrict__ fill,
    float* sink, int reps, int dilation, unsigned long long* stamps) {
    typedef typename ET::afrag_t half8;
    typedef typename ET::lds_t elem_t;
    constexpr int C = 128, CH = 64, KC = CH / 16, NCH = C / CH, MTW = (C / 32) / WM;
    constexpr int S = CH * 2 + 16;
    constexpr int ROWS = WN * NTW * 32 + (K - 1) * 5;
    constexpr int W_CHUNK = K * KC * 64, W_MT_STRIDE = NCH * W_CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = threadIdx.x; i < ROWS * S / 2; i += blockDim.x)
        reinterpret_cast<elem_t*>(smem)[i] = fill[i & 4095];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int ln = lane & 31, lh = lane >> 5;
    floatx16 acc[MTW][NTW];
    for (int mt = 0; mt < MTW; ++mt)
        for (int nt = 0; nt < NTW; ++nt)
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    const half8* wp = w + (size_t)wm * MTW * W_MT_STRIDE + lane;
    half8 afirst[G][MTW];
    load_a_group<ET, MTW, G>(afirst, wp, W_MT_STRIDE);
    const char* bptr = smem + (wn * NTW * 32 + ln) * S + lh * 16;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    const unsigned long long r0 = wall_clock64();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
    for (int r = 0; r < reps; ++r)
#pragma unroll 1
        for (int c = 0; c < NCH; ++c)
            mma_taps<ET, K, KC, MTW, NTW, G, S>(
                acc, bptr, dilation * S, wp + (size_t)c * W_CHUNK, W_MT_STRIDE,
                afirst, wp + (size_t)((c + 1) % NCH) * W_CHUNK);
    __builtin_amdgcn_sched_barrier(0);
    if (stamps && threadIdx.x == 0) {
        stamps[4 * blockIdx.x + 0] = c0;
        stamps[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memtime();
        stamps[4 * blockIdx.x + 2] = r0;
        stamps[4 * blockIdx.x + 3] = wall_clock64();
    }
    float s = 0.f;
    for (int mt = 0; mt < MTW; ++mt)
        for (int nt = 0; nt < NTW; ++nt)
            for (int r = 0; r < 16; ++r) s += acc[mt][nt][r];
    if (s == 12345.678f) sink[0] = s;
}

// The matrix pipe alone: 16 independent accumulators, operands in registers.
__global__ __launch_bounds__(512) void probe_kernel(
    const bf16x8* __restrict__ w, float* sink, int reps,
    unsigned long long* stamps) {
    const bf16x8 a = w[threadIdx.x & 63], b = w[64 + (threadIdx.x & 63)];
    floatx16 acc[4];
    for (int i = 0; i < 4; ++i)
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    const unsigned long long r0 = wall_clock64();
#pragma unroll 1
    for (int r = 0; r < reps; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) ElemBF16::mma(a, b, acc[i & 3]);
    if (threadIdx.x == 0) {
        stamps[4 * blockIdx.x + 0] = c0;
        stamps[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memtime();
        stamps[4 * blockIdx.x + 2] = r0;
        stamps[4 * blockIdx.x + 3] = wall_clock64();
    }
    float s = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int r = 0; r < 16; ++r) s += acc[i][r];
    if (s == 12345.678f) sink[0] = s;
}

// mean over workgroups of wave 0's stamps: shader cycles and 100 MHz ticks
static void stamp_means(const unsigned long long* dev, int grid, double* cycles,
                        double* ticks) {
    std::vector<unsigned long long> h(4 * (size_t)grid);
    hipMemcpy(h.data(), dev, h.size() * 8, hipMemcpyDeviceToHost);
    *cycles = *ticks = 0;
    for (int i = 0; i < grid; ++i) {
        *cycles += (double)(h[4 * i + 1] - h[4 * i]) / grid;
        *ticks += (double)(h[4 * i + 3] - h[4 * i + 2]) / grid;
    }
}

template <class ET, int K, int WM, int WN, int NTW, int G = 4>
static void run(const char* name, const typename ET::afrag_t* w,
                const typename ET::lds_t* fill, float* sink, int wgs_per_cu,
                int reps, unsigned long long* stamps = nullptr) {
    constexpr int S = 64 * 2 + 16;
    constexpr int smem = (WN * NTW * 32 + (K - 1) * 5) * S;
    auto kern = loop_kernel<ET, K, WM, WN, NTW, G>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                        hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int grid = 256 * wgs_per_cu;
    float ms = 0;
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WM * WN * 64), smem, 0, w,
                           fill, sink, reps, 5, stamps);
        hipEventRecord(e1); hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
    }
    // MFMAs of one wave, of the grid
    const double wave_mfmas = (double)reps * 2 * K * 4 * NTW * (4 / WM);
    const double mfmas = (double)grid * WM * WN * wave_mfmas;
    printf("%-34s %d WG/CU (%2d waves/CU): %7.2f ms  %6.0f TFLOP/s", name,
           wgs_per_cu, wgs_per_cu * WM * WN, ms, mfmas * 32768.0 / ms / 1e9);
    if (stamps) {
        double cycles, ticks;
        stamp_means(stamps, grid, &cycles, &ticks);
        // (wave 0 is the OLDER wave of its SIMD and is issued first whenever
        // it is ready: beside a second wave its cycles per MFMA are its own
        // stream's - 32 = never stalled - not half the SIMD's)
        printf("  | wave 0: %.1f cyc/MFMA, %.3f GHz", cycles / wave_mfmas,
               cycles / (ticks * 10.0));
    }
    printf("\n");
}

static unsigned short bf16_bits(float v) {
    unsigned u; memcpy(&u, &v, 4);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1)) >> 16);
}

int main() {
    const size_t wn = (size_t)4 * 2 * 11 * 4 * 64;   // frags for C=128 k=11
    std::vector<_Float16> hw(wn * 8), hf(4096);
    std::vector<unsigned short> bw(wn * 8), bf(4096);
    srand(1);
    for (auto& v : hw) v = (_Float16)(((float)rand() / (float)RAND_MAX * 2.f - 1.f) * 0.05f);
    for (auto& v : hf) v = (_Float16)((float)rand() / (float)RAND_MAX * 2.f - 1.f);
    for (size_t i = 0; i < bw.size(); ++i) bw[i] = bf16_bits((float)hw[i]);
    for (size_t i = 0; i < bf.size(); ++i) bf[i] = bf16_bits((float)hf[i]);
    half8* w; _Float16* fill; float* sink;
    bf16x8* w16; __bf16* fill16; unsigned long long* stamps;
    hipMalloc(&w, hw.size() * 2); hipMalloc(&fill, hf.size() * 2); hipMalloc(&sink, 4);
    hipMalloc(&w16, bw.size() * 2); hipMalloc(&fill16, bf.size() * 2);
    hipMalloc(&stamps, 4 * 512 * 8);
    hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(fill, hf.data(), hf.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(w16, bw.data(), bw.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(fill16, bf.data(), bf.size() * 2, hipMemcpyHostToDevice);
    printf("issue order PM_MMA_ORDER = %d\n", (int)PM_MMA_ORDER);
    {   // the register-resident probe: 256 workgroups x 8 waves
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        float ms = 0;
        const int reps = 20000;
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0);
            hipLaunchKernelGGL(probe_kernel, dim3(256), dim3(512), 0, 0, w16,
                               sink, reps, stamps);
            hipEventRecord(e1); hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
        }
        double cycles, ticks;
        stamp_means(stamps, 256, &cycles, &ticks);
        printf("%-34s 1 WG/CU ( 8 waves/CU): %7.2f ms  %6.0f TFLOP/s  | "
               "wave 0: %.1f cyc/MFMA, %.3f GHz\n",
               "probe: MFMAs on registers, bf16", ms,
               256.0 * 8 * reps * 16 * 32768.0 / ms / 1e9,
               cycles / (reps * 16.0), cycles / (ticks * 10.0));
    }
    run<ElemBF16, 11, 4, 2, 4>("bf16 k11 4x2 waves, wave 32x128 G4", w16, fill16, sink, 1, 2000, stamps);
    run<ElemBF16, 11, 4, 1, 4>("bf16 k11 4x1 waves, wave 32x128 G4", w16, fill16, sink, 1, 2000, stamps);
    run<ElemF16, 11, 4, 2, 4>("k11 4x2 waves, wave 32x128", w, fill, sink, 1, 2000);
    run<ElemF16, 11, 2, 4, 2, 2>("k11 2x4 waves, wave 64x64 G2", w, fill, sink, 1, 2000);
    run<ElemF16, 11, 2, 4, 2, 4>("k11 2x4 waves, wave 64x64 G4", w, fill, sink, 1, 2000);
    run<ElemF16, 11, 2, 2, 4, 2>("k11 2x2 waves, wave 64x128 G2", w, fill, sink, 1, 2000);
    run<ElemF16, 11, 2, 2, 4, 2>("k11 2x2 waves, wave 64x128 G2", w, fill, sink, 2, 2000);
    run<ElemF16, 11, 2, 4, 4, 2>("k11 2x4 waves, wave 64x128 G2", w, fill, sink, 1, 1000);
    run<ElemF16, 11, 1, 8, 2, 2>("k11 1x8 waves, wave 128x64 G2", w, fill, sink, 1, 1000);
    return 0;
}

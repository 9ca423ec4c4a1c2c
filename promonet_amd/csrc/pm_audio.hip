// The waveform front end of the C ABI (include/promonet_hip.h): the STFT as
// FFTs and as the framed-DFT GEMM with its backward, mel and its backward,
// loudness and resampling. Kernels: pm_stft.h, pm_fft.h, pm_resample.h; the
// framed DFT's exact-fp32 conv is compiled with the other convs and reached
// through pm_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "pm_host.h"
#include "pm_stft.h"
#include "pm_fft.h"
#include "pm_resample.h"

static const int NFFT = 1024, HOP = 256, BINS = 513, DFT_M = 1088;

static std::mutex g_basis_mutex;
struct DftBasis {
    void* forward = nullptr;     // packed windowed DFT basis (1088 x 256 x 4)
    void* backward = nullptr;    // packed transposed basis (256 x 1088 x 4)
    float* zeros = nullptr;      // 256 zero biases for the backward conv
};
static std::map<int, DftBasis> g_basis;   // per device

static int get_dft_basis(DftBasis* out, hipStream_t s) {
    int dev = 0;
    PM_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_basis_mutex);
    auto it = g_basis.find(dev);
    if (it != g_basis.end()) { *out = it->second; return PM_OK; }
    float* raw = nullptr;
    float* rawt = nullptr;
    DftBasis basis;
    const size_t raw_elems = 2ull * BINS * NFFT;
    const size_t packed_bytes = (size_t)DFT_M * NFFT * sizeof(float);
    PM_HIP_TRY(hipMalloc((void**)&raw, raw_elems * sizeof(float)));
    PM_HIP_TRY(hipMalloc((void**)&rawt, packed_bytes));
    PM_HIP_TRY(hipMalloc(&basis.forward, packed_bytes));
    PM_HIP_TRY(hipMalloc(&basis.backward, packed_bytes));
    PM_HIP_TRY(hipMalloc((void**)&basis.zeros, HOP * sizeof(float)));
    PM_HIP_TRY(hipMemsetAsync(basis.zeros, 0, HOP * sizeof(float), s));
    hipLaunchKernelGGL(pm_dft_basis_kernel,
                       dim3((unsigned)((raw_elems + 255) / 256)), dim3(256), 0,
                       s, raw, BINS, NFFT, HOP);
    PM_HIP_TRY(hipGetLastError());
    PM_HIP_TRY(pm_dft_pack(raw, basis.forward, 2 * BINS, DFT_M, HOP,
                           NFFT / HOP, s));
    // backward: out[q][c] = sum_j sum_m G[q - 3 + j][m] wt[c][m][j]
    const size_t t_elems = (size_t)HOP * DFT_M * (NFFT / HOP);
    hipLaunchKernelGGL(pm_dft_basis_transpose_kernel,
                       dim3((unsigned)((t_elems + 255) / 256)), dim3(256), 0,
                       s, raw, rawt, 2 * BINS, DFT_M, HOP, NFFT / HOP);
    PM_HIP_TRY(hipGetLastError());
    PM_HIP_TRY(pm_dft_pack(rawt, basis.backward, HOP, HOP, DFT_M, NFFT / HOP,
                           s));
    PM_HIP_TRY(hipStreamSynchronize(s));
    hipFree(raw);
    hipFree(rawt);
    g_basis[dev] = basis;
    *out = basis;
    return PM_OK;
}

extern "C" size_t pm_stft_scratch_bytes(int B, int N) {
    if (B < 1 || N < HOP) return 0;
    const size_t T = N / HOP;
    return pm_align256((size_t)B * (T + 3) * HOP * sizeof(float));
}

static int stft_launch(
    int epi, const float* audio, float* out, unsigned* maxbits, int B, int N,
    void* scratch, size_t scratch_bytes, hipStream_t s,
    const float* grad = nullptr) {
    if (!audio || !out || !scratch) return pm_fail(PM_EINVAL, "null argument");
    const int pad = (NFFT - HOP) / 2;
    if (B < 1 || N <= pad)
        return pm_fail(PM_EINVAL,
                       "need more than %d samples (reflect pad)", pad);
    const int T = N / HOP;
    if (T < 1) return pm_fail(PM_EINVAL, "fewer samples than one hop");
    if (scratch_bytes < pm_stft_scratch_bytes(B, N))
        return pm_fail(PM_ENOMEM, "scratch too small");
    DftBasis basis;
    int rc = get_dft_basis(&basis, s);
    if (rc) return rc;
    float* padded = (float*)scratch;
    // only the first (T + 3) * HOP padded samples are ever framed
    const int Np = (T + 3) * HOP;
    hipLaunchKernelGGL(pm_reflect_pad_kernel, dim3((Np + 255) / 256, B),
                       dim3(256), 0, s, audio, padded, N, pad, Np);
    PM_HIP_TRY(hipGetLastError());
    PmDftConv a = {};
    a.x = padded; a.out = out; a.w = basis.forward; a.bias = nullptr;
    a.B = B; a.L = T + 3; a.Lout = T; a.Cin = HOP; a.M = DFT_M;
    a.bins = BINS; a.maxbits = maxbits; a.grad = grad; a.pad = 0;
    PM_HIP_TRY(pm_dft_conv(epi, a, s));
    return PM_OK;
}

// Brute-force cross-check of pm_stft_magnitude: the same spectrogram by the
// framed-DFT GEMM (exact-fp32 MFMA), independent of the FFT code path.
extern "C" int pm_stft_magnitude_dft(
    const float* audio, float* out, int B, int N, void* scratch,
    size_t scratch_bytes, void* stream) {
    return stft_launch(1, audio, out, nullptr, B, N, scratch, scratch_bytes,
                       (hipStream_t)stream);
}

// ---- FFT path (forward transforms; pm_fft.h) --------------------------------
static std::map<int, float*> g_fft_tables;   // per device (g_basis_mutex)
// (per host thread, like the other test / tuning hooks: a setter on one thread
// cannot change the launch geometry of a call in flight on another)
static thread_local int g_fft_frames_per_group = 16;

static int get_fft_tables(const float** out, hipStream_t s) {
    int dev = 0;
    PM_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_basis_mutex);
    auto it = g_fft_tables.find(dev);
    if (it != g_fft_tables.end()) { *out = it->second; return PM_OK; }
    std::vector<float> h(PM_FFT_TAB_FLOATS);
    const double pi2 = 6.283185307179586476925286766559;
    // periodic hann (torch.hann_window(1024), spectrogram.py:29)
    for (int n = 0; n < NFFT; ++n)
        h[n] = (float)(0.5 - 0.5 * cos(pi2 * n / NFFT));
    for (int j = 0; j < 512; ++j) {
        h[PM_FFT_TAB_W512 + 2 * j] = (float)cos(pi2 * j / 512.0);
        h[PM_FFT_TAB_W512 + 2 * j + 1] = (float)-sin(pi2 * j / 512.0);
    }
    for (int k = 0; k <= 512; ++k) {
        h[PM_FFT_TAB_W1024 + 2 * k] = (float)cos(pi2 * k / 1024.0);
        h[PM_FFT_TAB_W1024 + 2 * k + 1] = (float)-sin(pi2 * k / 1024.0);
    }
    float* d = nullptr;
    PM_HIP_TRY(hipMalloc((void**)&d, h.size() * sizeof(float)));
    PM_HIP_TRY(hipMemcpyAsync(d, h.data(), h.size() * sizeof(float),
                              hipMemcpyHostToDevice, s));
    PM_HIP_TRY(hipStreamSynchronize(s));
    g_fft_tables[dev] = d;
    *out = d;
    return PM_OK;
}

// 2 (default): both transforms for every frame; 1: the 8-band loudness runs the
// OPTIMISTIC first pass and transforms a group a second time only where the
// floor bites. Opt-in because it depends on the material: noise at a steady
// level 56 -> 47 us (batch 32 x 10 s), but a group with ANY bin more than 80 dB
// under its utterance's maximum is transformed twice by a first pass that costs
// what the second does (36 + 34 us against 27 + 34 when every group is) - and
// 16 frames x 513 bins of recorded speech usually hold such a bin.
static thread_local int g_loudness_passes = 2;
extern "C" int pm_stft_set_loudness_passes(int passes) {
    if (passes != 1 && passes != 2)
        return pm_fail(PM_EINVAL, "loudness passes: 1 (optimistic) or 2");
    g_loudness_passes = passes;
    return PM_OK;
}

extern "C" int pm_stft_set_frames_per_group(int frames) {
    if (frames != 16 && frames != 32)
        return pm_fail(PM_EINVAL, "frames per workgroup must be 16 or 32");
    g_fft_frames_per_group = frames;
    return PM_OK;
}

// One geometry of the FFT kernel as PERSISTENT workgroups: the grid is what
// the device holds at once (occupancy x CUs, asked once per geometry) and a
// workgroup walks the (utterance, group of NW x FPW frames) pairs with that
// stride.
// `dry` (pm_stft_launch_info): fill a.groups / a.total / a.grid, launch nothing
template <int EPI, int NW, int FPW>
static int fft_launch_shape(FftArgs& a, hipStream_t s, int* dry_grid = nullptr) {
    auto kern = pm_stft_fft_kernel<EPI, NW, FPW>;
    constexpr int smem = pm_fft_smem_bytes<EPI, NW, FPW>();
    PM_HIP_TRY(pm_ensure_dynamic_lds(reinterpret_cast<const void*>(kern),
                                     smem));
    static std::atomic<int> per_cu{0};
    int resident = per_cu.load(std::memory_order_relaxed);
    if (resident == 0) {
        PM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
               &resident, kern, NW * 64, smem));
        if (resident < 1) resident = 1;
        per_cu.store(resident, std::memory_order_relaxed);
    }
    a.groups = (a.T + NW * FPW - 1) / (NW * FPW);
    const long long total = (long long)a.groups * a.B;
    if (total > PM_MAX_GRID) return pm_fail(PM_EINVAL, "batch too large");
    a.total = (int)total;
    const int cus = pm_device_cus() > 0 ? pm_device_cus() : 256;
    const int grid = (int)std::min<long long>(total, (long long)resident * cus);
    if (dry_grid) { *dry_grid = grid; return PM_OK; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), smem, s, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// `frames_per_group`: read ONCE per API call by the caller (pm_loudness runs
// two passes whose per-group maxima must be indexed the same way)
template <int EPI>
static int fft_launch(FftArgs& a, hipStream_t s,
                      int frames_per_group = g_fft_frames_per_group,
                      int* dry_grid = nullptr) {
    const int pad = (NFFT - HOP) / 2;
    if (!a.audio && !dry_grid) return pm_fail(PM_EINVAL, "null argument");
    if (a.B < 1 || a.N <= pad)
        return pm_fail(PM_EINVAL,
                       "need more than %d samples (reflect pad)", pad);
    a.T = a.N / HOP;
    if (a.T < 1) return pm_fail(PM_EINVAL, "fewer samples than one hop");
    if (a.B > 65535) return pm_fail(PM_EINVAL, "batch too large (max 65535)");
    if (!dry_grid) {
        int rc = get_fft_tables(&a.tables, s);
        if (rc) return rc;
    }
    // 16 frames by EIGHT waves of two frames for the magnitude / log-mel
    // launches (two 512-thread workgroups per CU: their 513 x 17 staging tiles
    // fill the LDS), four waves of four frames for the loudness passes, which
    // stage 8 rows or nothing and keep four workgroups per CU resident (round 5:
    // every FFT kernel fits 128 registers; measured shapes and their history:
    // profiles/r04/stft_pmc.txt, profiles/r05/ab_fft_packed.txt)
    if (frames_per_group == 32)
        return fft_launch_shape<EPI, 8, 4>(a, s, dry_grid);
#ifndef PM_FFT_LOUD_8X2
#define PM_FFT_LOUD_8X2 0
#endif
    if constexpr (EPI == 1 || EPI == 4 || PM_FFT_LOUD_8X2)
        return fft_launch_shape<EPI, 8, 2>(a, s, dry_grid);
    else
        return fft_launch_shape<EPI, 4, 4>(a, s, dry_grid);
}

// The geometry the next launch of one FFT transform would take on this device
// and host thread (tests assert that the persistent multi-group walk - more
// groups than resident workgroups - is what they exercise). transform: 1
// magnitude, 4 log-mel, 2 / 3 / 5 / 6 the loudness passes (maximum, generic
// bands, the 8 default bands, their optimistic first pass).
extern "C" int pm_stft_launch_info(
    int transform, int B, int N, int* total_groups, int* workgroups) {
    if (!total_groups || !workgroups)
        return pm_fail(PM_EINVAL, "null argument");
    FftArgs a = {};
    a.B = B; a.N = N;
    int grid = 0, rc;
    switch (transform) {
        case 1: rc = fft_launch<1>(a, nullptr, g_fft_frames_per_group, &grid); break;
        case 2: rc = fft_launch<2>(a, nullptr, g_fft_frames_per_group, &grid); break;
        case 3: rc = fft_launch<3>(a, nullptr, g_fft_frames_per_group, &grid); break;
        case 4: rc = fft_launch<4>(a, nullptr, g_fft_frames_per_group, &grid); break;
        case 5: rc = fft_launch<5>(a, nullptr, g_fft_frames_per_group, &grid); break;
        case 6: rc = fft_launch<6>(a, nullptr, g_fft_frames_per_group, &grid); break;
        default: return pm_fail(PM_EINVAL, "transform must be 1..6");
    }
    if (rc) return rc;
    *total_groups = a.total;
    *workgroups = grid;
    return PM_OK;
}

extern "C" int pm_stft_magnitude(
    const float* audio, float* out, int B, int N, void* scratch,
    size_t scratch_bytes, void* stream) {
    (void)scratch; (void)scratch_bytes;   // (the FFT path needs none)
    if (!out) return pm_fail(PM_EINVAL, "null argument");
    FftArgs a = {};
    a.audio = audio; a.out = out; a.B = B; a.N = N;
    return fft_launch<1>(a, (hipStream_t)stream);
}

// spectrogram.from_audio(audio, mels=True): the log-mel spectrogram straight
// from the FFT workgroup's LDS tile (the (B, 513, T) magnitudes never reach
// HBM). basis (mels, 513) -> pm_stft_mel_prepare -> `prepared`
// (pm_stft_mel_scratch_bytes(mels) bytes, reusable)
struct MelLayout { int* table; float* vals; size_t total; };
static MelLayout mel_layout(int mels, void* base) {
    PmCarve c(base);
    return {c.take<int>((size_t)3 * mels + 1),
            c.take<float>((size_t)mels * BINS), c.used};
}

extern "C" size_t pm_stft_mel_scratch_bytes(int mels) {
    return mels < 1 ? 0 : mel_layout(mels, nullptr).total;
}

// Compact the (mels, 513) filterbank once (per basis): `prepared` then feeds
// any number of pm_stft_mel calls.
extern "C" int pm_stft_mel_prepare(
    const float* basis, int mels, void* prepared, size_t prepared_bytes,
    void* stream) {
    if (!basis || !prepared) return pm_fail(PM_EINVAL, "null argument");
    if (mels < 1 || mels > 1024)
        return pm_fail(PM_EINVAL, "1..1024 mel filters");
    const MelLayout l = mel_layout(mels, prepared);
    if (prepared_bytes < l.total)
        return pm_fail(PM_ENOMEM, "buffer too small");
    hipLaunchKernelGGL(pm_mel_csr_kernel, dim3(1), dim3(256), 0,
                       (hipStream_t)stream, basis, l.table, l.vals, mels, BINS);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stft_mel(
    const float* audio, const void* prepared, float* out, int B, int N,
    int mels, int use_threshold, float log_threshold, void* stream) {
    if (!prepared || !out) return pm_fail(PM_EINVAL, "null argument");
    if (mels < 1 || mels > 1024)
        return pm_fail(PM_EINVAL, "1..1024 mel filters");
    hipStream_t s = (hipStream_t)stream;
    const MelLayout l = mel_layout(mels, const_cast<void*>(prepared));
    FftArgs a = {};
    a.audio = audio; a.out = out; a.B = B; a.N = N;
    a.mel_span = l.table; a.mel_vals = l.vals; a.rows = mels;
    a.use_thr = use_threshold; a.thr = log_threshold;
    return fft_launch<4>(a, s);
}

// Backward of pm_stft_magnitude (the training mel loss differentiates through
// spectrogram.from_audio: promonet/train/core.py:277-305). Two exact-fp32 MFMA
// convs: the framed DFT again, its epilogue turning the incoming gradient into
// the DFT cotangent grad / |X| * (re, im); then the overlap-add of that
// cotangent against the transposed basis; then the adjoint of the reflect pad.
struct StftBackwardLayout { char* stft; float *cot, *gpad; size_t total; };
static StftBackwardLayout stft_backward_layout(int B, int N, void* base) {
    const size_t T = N / HOP;
    PmCarve c(base);
    return {c.take<char>(pm_stft_scratch_bytes(B, N)),   // stft_launch's own
            c.take<float>((size_t)B * T * DFT_M),        // (B, T, 1088)
            c.take<float>((size_t)B * (T + 3) * HOP), c.used};
}

extern "C" size_t pm_stft_backward_scratch_bytes(int B, int N) {
    if (B < 1 || N < HOP) return 0;
    return stft_backward_layout(B, N, nullptr).total;
}

extern "C" int pm_stft_magnitude_backward(
    const float* audio, const float* grad_out, float* grad_audio, int B, int N,
    void* scratch, size_t scratch_bytes, void* stream) {
    if (!audio || !grad_out || !grad_audio || !scratch)
        return pm_fail(PM_EINVAL, "null argument");
    if (B < 1 || N < HOP || scratch_bytes < pm_stft_backward_scratch_bytes(B, N))
        return pm_fail(PM_ENOMEM, "scratch too small");
    hipStream_t s = (hipStream_t)stream;
    const int T = N / HOP;
    const int pad = (NFFT - HOP) / 2;
    const StftBackwardLayout l = stft_backward_layout(B, N, scratch);
    int rc = stft_launch(3, audio, l.cot, nullptr, B, N, l.stft,
                         pm_stft_scratch_bytes(B, N), s, grad_out);
    if (rc) return rc;
    DftBasis basis;
    rc = get_dft_basis(&basis, s);
    if (rc) return rc;
    PmDftConv a = {};
    a.x = l.cot; a.out = l.gpad; a.w = basis.backward; a.bias = basis.zeros;
    a.B = B; a.L = T; a.Lout = T + 3; a.Cin = DFT_M; a.M = HOP;
    a.pad = 3;
    PM_HIP_TRY(pm_dft_conv(0, a, s));
    const int Np = (T + 3) * HOP;
    hipLaunchKernelGGL(pm_reflect_pad_adjoint_kernel,
                       dim3((N + 255) / 256, B), dim3(256), 0, s, l.gpad,
                       grad_audio, N, pad, Np);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// Backward of pm_linear_to_mel: grad_mel (B, M, T) -> grad_spec (B, F, T);
// scratch holds B * M * T floats.
extern "C" int pm_linear_to_mel_backward(
    const float* spec, const float* basis, const float* grad_mel,
    float* grad_spec, float* scratch, int B, int F, int M, int T,
    int use_threshold, float log_threshold, void* stream) {
    if (!spec || !basis || !grad_mel || !grad_spec || !scratch)
        return pm_fail(PM_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pm_mel_backward_rows_kernel,
                       dim3((T + 255) / 256, M, B), dim3(256), 0, s, spec,
                       basis, grad_mel, scratch, F, M, T, use_threshold,
                       log_threshold);
    PM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pm_mel_backward_cols_kernel,
                       dim3((T + 255) / 256, F, B), dim3(256), 0, s, basis,
                       scratch, grad_spec, F, M, T);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_linear_to_mel(
    const float* spec, const float* basis, float* out, int B, int F, int M,
    int T, int use_threshold, float log_threshold, void* stream) {
    if (!spec || !basis || !out) return pm_fail(PM_EINVAL, "null argument");
    hipLaunchKernelGGL(pm_mel_kernel, dim3((T + 255) / 256, M, B), dim3(256),
                       0, (hipStream_t)stream, spec, basis, out, F, M, T,
                       use_threshold, log_threshold);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// one maximum and one minimum per FFT workgroup (>= 16 frames each) and
// utterance
struct LoudnessLayout { float *group_max, *group_min; size_t total; };
static LoudnessLayout loudness_layout(int B, int N, void* base) {
    const size_t groups = ((size_t)(N / HOP) + 15) / 16;
    PmCarve c(base);
    return {c.take<float>((size_t)B * groups),
            c.take<float>((size_t)B * groups), c.used};
}

extern "C" size_t pm_loudness_scratch_bytes(int B, int N) {
    if (B < 1 || N < HOP) return 0;
    return loudness_layout(B, N, nullptr).total;
}

// Two passes over the audio (4 B / sample each) instead of a (B, 513, T) dB
// tensor written and re-read: pass 1 finds every utterance's maximum dB
// (librosa.amplitude_to_db's top_db reference, loudness.py:46), pass 2 repeats
// the FFT and writes the floored, A-weighted band means.
// With pm_stft_set_loudness_passes(1) the default 8 bands run OPTIMISTICALLY:
// pass 1 (EPI 6) already writes the band means, without a floor, and records
// every 16-frame group's minimum dB next to its maximum; pass 2 (EPI 5)
// transforms only the groups that have a bin under their utterance's floor -
// for the others max(v, floor) == v and pass 1's means are final, bit for bit
// (tests/test_gpu_preprocess_full.py). Off by default: see g_loudness_passes.
extern "C" int pm_loudness(
    const float* audio, const float* a_weights, float* out, int B, int N,
    int bands, float min_db, void* scratch, size_t scratch_bytes,
    void* stream) {
    if (!audio || !a_weights || !out || !scratch)
        return pm_fail(PM_EINVAL, "null argument");
    if (bands < 1 || (bands > 16 && bands != BINS))
        return pm_fail(PM_EINVAL, "bands must be 1..16 or 513 (no averaging)");
    if (B < 1 || N < HOP || scratch_bytes < pm_loudness_scratch_bytes(B, N))
        return pm_fail(PM_ENOMEM, "scratch too small");
    hipStream_t s = (hipStream_t)stream;
    FftArgs a = {};
    a.audio = audio; a.out = out; a.B = B; a.N = N;
    const LoudnessLayout l = loudness_layout(B, N, scratch);
    a.group_max = l.group_max;
    const int frames_per_group = g_fft_frames_per_group;   // both passes
    a.weights = a_weights; a.rows = bands;
    const double step = (double)BINS / (double)bands;   // loudness.py:96
    for (int b = 0; b <= bands && b <= 16; ++b)
        a.band_start[b] = (int)(b * step);
    if (bands == 1) { a.band_start[0] = 0; a.band_start[1] = BINS; }
    a.min_db = min_db; a.top_db = 80.f;
    // the default 8 bands: band j = bins 64 j .. 64 j + 63 (+ bin 512 in the
    // last), reduced across the wave out of the registers (EPI 5)
    bool aligned8 = bands == 8;
    for (int b = 0; aligned8 && b < 8; ++b) aligned8 = a.band_start[b] == 64 * b;
#ifdef PM_LOUD_NO_EPI5
    aligned8 = false;
#endif
    aligned8 = aligned8 && a.band_start[8] == BINS;
    if (aligned8 && g_loudness_passes == 1) {
        a.group_min = l.group_min;
        int rc = fft_launch<6>(a, s, frames_per_group);
        if (rc) return rc;
        return fft_launch<5>(a, s, frames_per_group);
    }
    int rc = fft_launch<2>(a, s, frames_per_group);
    if (rc) return rc;
    if (aligned8) return fft_launch<5>(a, s, frames_per_group);
    return fft_launch<3>(a, s, frames_per_group);
}

// Polyphase sinc resampling (pm_resample.h). Every argument is checked before
// the first HIP call, so the checks answer on a machine without a GPU.
extern "C" int pm_resample_tile(int orig, int new_, int width) {
    if (orig < 1 || new_ < 1 || width < 1)
        return pm_fail(PM_EINVAL, "orig, new and width must be at least 1");
    const int groups = pm_resample_groups(orig, new_, width);
    if (groups < 1)
        return pm_fail(PM_EINVAL, "resampling ratio %d / %d: %d strides of a "
                       "%lld-tap filter do not fit %d floats of LDS", orig, new_,
                       RS_CHAINS, 2ll * width + orig, RS_LDS_FLOATS);
    return RS_CHAINS * groups;
}

extern "C" int pm_resample(
    const float* x, const int* lengths, const float* bank, float* out,
    int rows, int n_in, long long x_stride, int orig, int new_, int width,
    int n_out, long long out_stride, void* stream) {
    if (rows < 0 || n_in < 0 || n_out < 0)
        return pm_fail(PM_EINVAL, "negative size");
    if (orig < 1 || new_ < 1 || width < 1)
        return pm_fail(PM_EINVAL, "orig, new and width must be at least 1");
    if (!x || !bank || !out) return pm_fail(PM_EINVAL, "null argument");
    if (n_out < ((long long)new_ * n_in + orig - 1) / orig)
        return pm_fail(PM_EINVAL,
                       "n_out %d is below ceil(new n_in / orig) = %lld",
                       n_out, ((long long)new_ * n_in + orig - 1) / orig);
    if (x_stride < n_in || out_stride < n_out)
        return pm_fail(PM_EINVAL, "a row stride is below its row's length");
    const int strides = pm_resample_tile(orig, new_, width);
    if (strides < 0) return strides;
    if (rows == 0 || n_out == 0) return PM_OK;
    ResampleArgs a;
    a.x = x; a.lengths = lengths; a.bank = bank; a.out = out;
    a.x_stride = x_stride; a.out_stride = out_stride;
    a.n_in = n_in; a.n_out = n_out; a.orig = orig; a.new_ = new_;
    a.width = width; a.taps = 2 * width + orig;
    a.groups = strides / RS_CHAINS;
    const long long tile_out = (long long)strides * new_;
    a.tiles = (int)((n_out + tile_out - 1) / tile_out);
    if ((long long)a.tiles * rows > PM_MAX_GRID)
        return pm_fail(PM_EINVAL, "too many workgroups (%d per row x %d rows)",
                       a.tiles, rows);
    const int phases = pm_resample_phases(new_);
    a.half = (new_ + phases - 1) / phases;
    const int V = orig % 4 == 0 ? 4 : orig % 2 == 0 ? 2 : 1;
    void (*kern)(ResampleArgs);
    if (phases == 1)
        kern = V == 4 ? pm_resample_kernel<4, 1> : V == 2 ? pm_resample_kernel<2, 1>
                                                          : pm_resample_kernel<1, 1>;
    else
        kern = V == 4 ? pm_resample_kernel<4, RS_PHASES>
             : V == 2 ? pm_resample_kernel<2, RS_PHASES>
                      : pm_resample_kernel<1, RS_PHASES>;
    // at most RS_LDS_FLOATS floats (pm_resample.h): under the default limit
    const size_t smem = ((size_t)(strides - 1) * orig + a.taps) * sizeof(float);
    hipLaunchKernelGGL(kern, dim3(a.tiles * rows), dim3(RS_THREADS), smem,
                       (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

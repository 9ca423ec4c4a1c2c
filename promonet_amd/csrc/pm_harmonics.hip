// Viterbi decoding and the harmonic-analysis stages of the C ABI
// (include/promonet_hip.h). Kernels: pm_viterbi.h, pm_harmonics.h. Every
// argument is checked before the first HIP call, so the checks answer on a
// machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_viterbi.h"
#include "pm_harmonics.h"

extern "C" size_t pm_viterbi_workspace(int batch, int frames, int states) {
    if (batch < 1 || frames < 1 || states < 1 || states > VT_MAX_STATES)
        return 0;
    return pm_align256((size_t)batch * frames * states * sizeof(short));
}

extern "C" int pm_viterbi(const float* observation, const int* lengths,
                          const float* band, long long band_floats,
                          const int* table, const float* initial, int* out,
                          int batch, int frames, int states, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (batch < 0 || frames < 0 || states < 1)
        return pm_fail(PM_EINVAL, "batch and frames must not be negative and "
                       "states at least 1");
    if (states > VT_MAX_STATES)
        return pm_fail(PM_EINVAL, "%d states: back-pointers are int16, at most "
                       "%d states", states, VT_MAX_STATES);
    if (pm_viterbi_lds(states) > VT_LDS_BYTES)
        return pm_fail(PM_EINVAL,
                       "%d states: two rows of scores need %zu bytes "
                       "of LDS, above %d", states, pm_viterbi_lds(states),
                       VT_LDS_BYTES);
    if (band_floats < 0 || (band_floats & 3))
        return pm_fail(PM_EINVAL, "the band must hold a multiple of 4 floats");
    if (batch == 0 || frames == 0) return PM_OK;
    if (!observation || !band || !table || !initial || !out || !workspace)
        return pm_fail(PM_EINVAL, "null argument");
    if (workspace_bytes < pm_viterbi_workspace(batch, frames, states))
        return pm_fail(PM_ENOMEM, "workspace too small");
    ViterbiArgs a;
    a.obs = observation; a.lengths = lengths; a.band = band; a.table = table;
    a.initial = initial; a.bp = (short*)workspace; a.out = out;
    a.band_floats = band_floats; a.T = frames; a.S = states;
    hipLaunchKernelGGL(pm_viterbi_kernel, dim3(batch), dim3(VT_THREADS),
                       pm_viterbi_lds(states), (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_harmonics_highpass(const float* x, const int* lengths,
                                     float* y, int rows, int samples,
                                     long long x_stride, long long y_stride,
                                     float b0, float b1, float b2, float a1,
                                     float a2, void* stream) {
    if (rows < 0 || samples < 0) return pm_fail(PM_EINVAL, "negative size");
    if (x_stride < samples || y_stride < samples)
        return pm_fail(PM_EINVAL, "a row stride is below its row's length");
    if (rows == 0 || samples == 0) return PM_OK;
    if (!x || !y) return pm_fail(PM_EINVAL, "null argument");
    HighpassArgs a;
    a.x = x; a.lengths = lengths; a.y = y;
    a.x_stride = x_stride; a.y_stride = y_stride; a.n = samples;
    a.b0 = b0; a.b1 = b1; a.b2 = b2; a.a1 = a1; a.a2 = a2;
    hipLaunchKernelGGL(hm_highpass_kernel, dim3(rows), dim3(HM_HP_THREADS), 0,
                       (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_harmonics_stft(const float* x, const int* geometry,
                                 const float* window, const float* twiddle,
                                 float* out, int rows, long long x_stride,
                                 int frames, int states, int bin0, int hop,
                                 void* stream) {
    if (rows < 0 || frames < 0) return pm_fail(PM_EINVAL, "negative size");
    if (bin0 < 0 || states < 1 || bin0 + states > HM_HALF + 1)
        return pm_fail(PM_EINVAL, "bins [%d, %d) are not bins of a %d-point "
                       "transform", bin0, bin0 + states, HM_FFT);
    if (hop < 1) return pm_fail(PM_EINVAL, "hop must be at least 1");
    if (x_stride < 0) return pm_fail(PM_EINVAL, "negative stride");
    if ((long long)rows * frames > PM_MAX_GRID)
        return pm_fail(PM_EINVAL, "too many frames");
    if (rows == 0 || frames == 0) return PM_OK;
    if (!x || !geometry || !window || !twiddle || !out)
        return pm_fail(PM_EINVAL, "null argument");
    HarmonicStftArgs a;
    a.x = x; a.geometry = geometry; a.window = window; a.twiddle = twiddle;
    a.out = out; a.x_stride = x_stride; a.T = frames; a.S = states;
    a.bin0 = bin0; a.hop = hop;
    hipLaunchKernelGGL(hm_stft_kernel, dim3(rows * frames),
                       dim3(HM_STFT_THREADS), 0, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_harmonics_observation(const float* x, const float* f0,
                                        const float* frequencies,
                                        const int* row_frames, float* out,
                                        int* valid, int rows, int frames,
                                        int states, float low, float high,
                                        void* stream) {
    if (rows < 0 || frames < 0 || states < 1)
        return pm_fail(PM_EINVAL, "rows and frames must not be negative and "
                       "states at least 1");
    if ((long long)rows * frames > PM_MAX_GRID)
        return pm_fail(PM_EINVAL, "too many frames");
    if (rows == 0 || frames == 0) return PM_OK;
    if (!x || !frequencies || !out || !valid)
        return pm_fail(PM_EINVAL, "null argument");
    ObservationArgs a;
    a.x = x; a.f0 = f0; a.frequencies = frequencies; a.frames = row_frames;
    a.out = out; a.valid = valid; a.T = frames; a.S = states;
    a.low = low; a.high = high;
    hipLaunchKernelGGL(hm_observation_kernel, dim3(rows * frames),
                       dim3(HM_OBS_THREADS), 0, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_harmonics_peaks(const float* x, const float* frequencies,
                                  const int* row_frames, float* out, int rows,
                                  int frames, int states, int peaks,
                                  void* stream) {
    if (rows < 0 || frames < 0 || states < 1 || peaks < 0)
        return pm_fail(PM_EINVAL, "rows, frames and peaks must not be negative "
                       "and states at least 1");
    const long long total = (long long)rows * frames;
    if ((total + HM_PEAK_THREADS - 1) / HM_PEAK_THREADS > PM_MAX_GRID)
        return pm_fail(PM_EINVAL, "too many frames");
    if (total == 0 || peaks == 0) return PM_OK;
    if (!x || !frequencies || !out) return pm_fail(PM_EINVAL, "null argument");
    PeakArgs a;
    a.x = x; a.frequencies = frequencies; a.frames = row_frames; a.out = out;
    a.B = rows; a.T = frames; a.S = states; a.peaks = peaks;
    hipLaunchKernelGGL(hm_peak_kernel,
                       dim3((total + HM_PEAK_THREADS - 1) / HM_PEAK_THREADS),
                       dim3(HM_PEAK_THREADS), 0, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

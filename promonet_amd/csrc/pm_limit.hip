// The loudness-editing stages of the C ABI (include/promonet_hip.h): the
// limiter and the shift. Kernels: pm_limit.h. Every argument is checked before
// the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_limit.h"

namespace {

// [p, p + rows * stride) of floats against [q, ...)
bool overlap(const float* p, long long p_stride, const float* q,
             long long q_stride, int rows, int samples) {
    return pm_overlap(p, ((size_t)(rows - 1) * p_stride + samples) * 4,
                      q, ((size_t)(rows - 1) * q_stride + samples) * 4);
}

bool unit(float v) { return v > 0.f && v < 1.f; }

}  // namespace

extern "C" int pm_limit_tile(int* chunk, int* tile) {
    if (chunk) *chunk = LM_CHUNK;
    if (tile) *tile = LM_TILE;
    return PM_OK;
}

extern "C" size_t pm_limit_workspace_bytes(int rows) {
    if (rows < 1) return 0;
    return pm_align256((size_t)rows * LM_STATS * sizeof(int));
}

extern "C" int pm_limit(const float* x, const int* lengths, float* out,
                        float* gain, int rows, int samples, long long x_stride,
                        long long out_stride, int delay, float attack,
                        float attack_complement, float release,
                        float threshold, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (rows < 0 || samples < 0) return pm_fail(PM_EINVAL, "negative size");
    if (delay < 1) return pm_fail(PM_EINVAL, "delay must be at least 1");
    if (!unit(attack) || !unit(attack_complement) || !unit(release))
        return pm_fail(PM_EINVAL, "the attack coefficient, its complement and "
                       "the release coefficient must lie inside (0, 1)");
    if (!(threshold > 0.f) || threshold > 3e38f)
        return pm_fail(PM_EINVAL, "the threshold must be positive and finite");
    if (x_stride < samples || out_stride < samples)
        return pm_fail(PM_EINVAL, "a row stride is below its row's length");
    if (rows == 0 || samples == 0) return PM_OK;
    if (!x || !out || !workspace) return pm_fail(PM_EINVAL, "null argument");
    if (overlap(x, x_stride, out, out_stride, rows, samples))
        return pm_fail(PM_EINVAL, "out must not alias x");
    if (workspace_bytes < pm_limit_workspace_bytes(rows))
        return pm_fail(PM_ENOMEM, "workspace too small");
    LimitArgs a;
    a.x = x; a.lengths = lengths; a.out = out; a.gain = gain;
    a.stats = (int*)workspace;
    a.x_stride = x_stride; a.out_stride = out_stride;
    a.samples = samples; a.delay = delay;
    a.a = attack; a.b = attack_complement; a.r = release; a.th = threshold;
    hipLaunchKernelGGL(pm_limit_kernel, dim3(rows), dim3(LM_THREADS), 0,
                       (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_loudness_shift(const float* x, const float* db,
                                 const int* lengths, const int* frame_lengths,
                                 float* out, int rows, int samples,
                                 long long x_stride, int frames,
                                 long long db_stride, long long out_stride,
                                 void* stream) {
    if (rows < 0 || samples < 0) return pm_fail(PM_EINVAL, "negative size");
    if (frames < 1) return pm_fail(PM_EINVAL, "frames must be at least 1");
    if (x_stride < samples || out_stride < samples)
        return pm_fail(PM_EINVAL, "a row stride is below its row's length");
    if (db_stride != 0 && db_stride < frames)
        return pm_fail(PM_EINVAL, "the stride of db is below `frames` (0 "
                       "shares one contour among the rows)");
    if (rows > 65535) return pm_fail(PM_EINVAL, "at most 65535 rows");
    if (rows == 0 || samples == 0) return PM_OK;
    if (!x || !db || !out) return pm_fail(PM_EINVAL, "null argument");
    ShiftArgs a;
    a.x = x; a.db = db; a.lengths = lengths; a.frame_lengths = frame_lengths;
    a.out = out; a.x_stride = x_stride; a.db_stride = db_stride;
    a.out_stride = out_stride; a.samples = samples; a.frames = frames;
    hipLaunchKernelGGL(pm_loudness_shift_kernel,
                       dim3((samples + LS_THREADS - 1) / LS_THREADS, rows),
                       dim3(LS_THREADS), 0, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// HiFi-GAN streaming of the C ABI (include/promonet_hip.h): the receptive
// field of the generator, and one overlap-save step - window kernel, the
// engine's forward on the window, emit kernel (pm_stream.h). Every argument is
// checked before the first HIP call, so the checks answer on a machine without
// a GPU.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pm_host.h"
#include "pm_stream.h"

namespace {

long long floor_div(long long a, long long b) {
    return a / b - (a % b != 0 && (a % b < 0) != (b < 0));
}
long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// The input frames the audio of frame 0 needs, by interval arithmetic
// backwards through the layers (hifigan.py:63-70): samples [0, hop) of the
// output, then per layer the input range a range of its output reads.
void context_of(const pm_hifigan_config& c, int* left, int* right) {
    long long hop = 1;
    for (int i = 0; i < c.num_stages; ++i) hop *= c.upsample_rates[i];
    long long a = 0, b = hop - 1;
    a -= 3; b += 3;                                  // output conv, k 7
    // the widest Block: per dilation d a conv (k, d) and a conv (k, 1)
    long long block = 0;
    for (int j = 0; j < c.num_resblocks; ++j) {
        const long long half = (c.resblock_kernel_sizes[j] - 1) / 2;
        long long reach = 0;
        for (int n = 0; n < c.num_dilations; ++n)
            reach += half * c.resblock_dilations[j][n] + half;
        block = std::max(block, reach);
    }
    for (int i = c.num_stages - 1; i >= 0; --i) {
        a -= block; b += block;
        // ConvTranspose1d(stride r, kernel k, padding q): out[n] reads x[m]
        // with 0 <= n + q - m r <= k - 1
        const long long r = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        const long long q = (k - r) / 2;
        a = ceil_div(a + q - k + 1, r);
        b = floor_div(b + q, r);
    }
    a -= 3; b += 3;                                  // input conv, k 7
    *left = (int)-a;
    *right = (int)b;
}

// engine workspace of the window | the window's audio (B, W * hop)
struct StreamPlan {
    char* engine; float* audio; size_t total;
    size_t engine_bytes;
};

StreamPlan make_plan(pm_hifigan_t h, int B, int W, void* base) {
    StreamPlan p;
    p.engine_bytes = pm_hifigan_workspace_bytes(h, B, W);
    PmCarve c(base);
    p.engine = c.take<char>(p.engine_bytes);
    p.audio = c.take<float>((size_t)B * W * pm_hifigan_hopsize(h));
    p.total = c.used;
    return p;
}

}  // namespace

extern "C" int pm_hifigan_context(pm_hifigan_t h, int* left, int* right) {
    if (!h || !left || !right) return pm_fail(PM_EINVAL, "null argument");
    context_of(*pm_hifigan_config_of(h), left, right);
    return PM_OK;
}

extern "C" size_t pm_hifigan_stream_workspace_bytes(
    pm_hifigan_t h, int batch, int window_frames) {
    if (!h || batch < 1 || window_frames < 1) return 0;
    return make_plan(h, batch, window_frames, nullptr).total;
}

extern "C" int pm_hifigan_stream(
    pm_hifigan_t h, const float* chunk, int chunk_cl, int chunk_frames,
    const float* prev_window, int prev_frames, int keep, float* next_window,
    const float* global_features, int global_batch, int emit_first,
    int emit_frames, float* out, int batch, void* workspace,
    size_t workspace_bytes, void* stream) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    if (batch < 1) return pm_fail(PM_EINVAL, "empty batch");
    if (chunk_frames < 0 || prev_frames < 0 || keep < 0 || emit_first < 0 ||
        emit_frames < 0)
        return pm_fail(PM_EINVAL, "negative frame count");
    // the schedule (hifigan.py: stream_schedule): the history is what the
    // previous window holds, at most the context of both sides; the emitted
    // frames lie inside the new window
    int left = 0, right = 0;
    context_of(*pm_hifigan_config_of(h), &left, &right);
    if (keep > prev_frames)
        return pm_fail(PM_EINVAL, "keep %d > prev_frames %d", keep,
                       prev_frames);
    if (keep > left + right)
        return pm_fail(PM_EINVAL, "keep %d > the context %d + %d", keep, left,
                       right);
    const long long W = (long long)keep + chunk_frames;
    if (W < 1) return pm_fail(PM_EINVAL, "empty window");
    if ((long long)emit_first + emit_frames > W)
        return pm_fail(PM_EINVAL, "emitted frames [%d, %d) outside the window "
                       "of %lld", emit_first, emit_first + emit_frames, W);
    const pm_hifigan_config& cfg = *pm_hifigan_config_of(h);
    const int Cpad = pm_hifigan_features_cl_channels(h);
    const long long hop = pm_hifigan_hopsize(h);
    if (W * std::max<long long>(Cpad, hop) * batch > 0x7fffffffll)
        return pm_fail(PM_EINVAL, "window too large");
    if (!next_window || (keep && !prev_window) || (chunk_frames && !chunk) ||
        (emit_frames && (!out || !global_features || !workspace)))
        return pm_fail(PM_EINVAL, "null argument");
    if (!pm_aligned16(next_window) || !pm_aligned16(prev_window) ||
        (chunk_cl && !pm_aligned16(chunk)))
        return pm_fail(PM_EINVAL, "window and channels-last chunk pointers "
                       "must be 16-byte aligned");
    const size_t row = (size_t)Cpad * sizeof(float);
    if (pm_overlap(next_window, (size_t)batch * W * row, prev_window,
                   (size_t)batch * prev_frames * row))
        return pm_fail(PM_EINVAL, "next_window must not alias prev_window");
    if (pm_overlap(next_window, (size_t)batch * W * row, chunk,
                   (size_t)batch * chunk_frames *
                       (chunk_cl ? row : cfg.num_features * sizeof(float))))
        return pm_fail(PM_EINVAL, "next_window must not alias chunk");
    StreamPlan p = {};
    if (emit_frames) {
        p = make_plan(h, batch, (int)W, workspace);
        if (workspace_bytes < p.total)
            return pm_fail(PM_ENOMEM, "workspace %zu < required %zu",
                           workspace_bytes, p.total);
    }
    hipStream_t s = (hipStream_t)stream;

    StreamWindowArgs a;
    a.prev = prev_window; a.chunk = chunk; a.next = next_window;
    a.prev_frames = prev_frames; a.keep = keep; a.c = chunk_frames;
    a.C = cfg.num_features; a.Cpad = Cpad; a.chunk_cl = chunk_cl != 0;
    a.quads = (long long)batch * W * (Cpad / 4);
    hipLaunchKernelGGL(
        pm_stream_window_kernel,
        dim3((unsigned)((a.quads + PM_STREAM_THREADS - 1) / PM_STREAM_THREADS)),
        dim3(PM_STREAM_THREADS), 0, s, a);
    PM_HIP_TRY(hipGetLastError());
    if (!emit_frames) return PM_OK;

    int rc = pm_hifigan_forward_window(
        h, next_window, global_features, global_batch, p.audio, batch, (int)W,
        p.engine, p.engine_bytes, s);
    if (rc != PM_OK) return rc;

    const long long first = emit_first * hop, n = emit_frames * hop;
    const bool vec = hop % 4 == 0 && pm_aligned16(out);
    const long long total = (long long)batch * n / (vec ? 4 : 1);
    const dim3 grid(
        (unsigned)((total + PM_STREAM_THREADS - 1) / PM_STREAM_THREADS));
    if (vec)
        hipLaunchKernelGGL(pm_stream_emit_kernel<4>, grid,
                           dim3(PM_STREAM_THREADS), 0, s, p.audio, out,
                           W * hop, first, n, total);
    else
        hipLaunchKernelGGL(pm_stream_emit_kernel<1>, grid,
                           dim3(PM_STREAM_THREADS), 0, s, p.audio, out,
                           W * hop, first, n, total);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

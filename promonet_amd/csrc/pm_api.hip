// C ABI of libpromonet_hip.so (see include/promonet_hip.h): the error state,
// the host helpers of pm_host.h that need it or a kernel of pm_misc.h, and the
// HiFi-GAN engine: weight folding / packing at load, workspace planning and
// the per-forward launch sequence. Host C++; every kernel it launches is
// hand-written HIP for gfx950 (pm_conv.h, pm_misc.h). The waveform front end
// is pm_audio.hip, the FARGAN engine pm_fargan.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pm_host.h"
#include "pm_launch.h"
#include "pm_misc.h"

#define PM_VERSION 100

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_error[512] = "";

int pm_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

#ifdef PM_TUNING
static unsigned long long* g_timeline = nullptr;   // pm_debug_timeline
unsigned long long* pm_timeline() { return g_timeline; }
#endif

hipError_t pm_ensure_dynamic_lds(const void* kern, int bytes) {
    static std::mutex guard;
    static std::map<std::pair<const void*, int>, int> granted;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(guard);
    int& have = granted[std::make_pair(kern, dev)];
    if (bytes > have) {
        e = hipFuncSetAttribute(
            kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        have = bytes;
    }
    return hipSuccess;
}

int pm_device_cus() {
    static std::mutex guard;
    static std::map<int, int> cus_of;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(guard);
    auto it = cus_of.find(dev);
    if (it != cus_of.end()) return it->second;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess)
        cus = 0;
    cus_of[dev] = cus;
    return cus;
}

// bytes per element of an LDS operand row / of a packed weight stream
static inline int esz(int dtype) {
    return dtype == PM_F32 || dtype == PM_F16X3 || dtype == PM_F16A2 ? 4 : 2;
}
static inline int wsz(int dtype) {
    return dtype == PM_F32 || dtype == PM_F16X3 ? 4 : 2;
}
// A stage's (or the engine's) operand type code -> the type of its Blocks and
// of its upsampler (promonet_hip.h: PM_F16A2, PM_F16UX)
static inline int block_dtype(int code) { return code == PM_F16UX ? PM_F16 : code; }
// (the PM_F16UX upsampler as PM_F16A2 instead: same step, 1 % more error)
static inline int up_dtype(int code) {
    return code == PM_F16A2 || code == PM_F16UX ? PM_F16X3 : code;
}

// ---------------------------------------------------------------------------
// dtype dispatch: f(ET()) with ET the Elem* type of the operand code `dtype`
// ---------------------------------------------------------------------------
template <class F> static hipError_t with_elem(int dtype, F&& f) {
    switch (dtype) {
        case PM_F32: return f(ElemF32());
        case PM_F16: return f(ElemF16());
        case PM_BF16: return f(ElemBF16());
        case PM_F16X3: return f(ElemF16X3());
        case PM_F16A2: return f(ElemF16A2());
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_pair(
    int dtype, int C, int K, const PairArgs& a0, hipStream_t s) {
    PairArgs a = a0;
#ifdef PM_TUNING
    a.timeline = g_timeline;
#endif
    return with_elem(dtype, [&](auto et) {
        typedef decltype(et) ET;
        return pm_launch_pair<ET>(C, K, pm_plan_pair<ET>(C, K, a.B, a.L), a, s);
    });
}

static hipError_t plan_stage(int dtype, const PmStage& st, int fusion, PmPlan* p) {
    return with_elem(dtype, [&](auto et) {
        *p = pm_plan_stage<decltype(et)>(st, fusion);
        return hipSuccess;
    });
}

static hipError_t launch_block3(
    int dtype, const PmLaunch& l, const PmStage& st, int j, hipStream_t s) {
    return with_elem(dtype, [&](auto et) {
        return pm_launch_block3<decltype(et)>(l, st, j, s);
    });
}

static hipError_t launch_mrf(
    int dtype, const PmLaunch& l, const PmStage& st, hipStream_t s) {
    return with_elem(dtype, [&](auto et) {
        return pm_launch_mrf<decltype(et)>(l, st, s);
    });
}

// An MRF stage description (pm_launch.h) with what its Blocks share
static PmStage stage_desc(int C, const float* x, float* out, int B, int L,
                          int mode, float scale, int nblocks, int niter) {
    PmStage d = {};
    d.C = C; d.x = x; d.out = out; d.B = B; d.L = L; d.mode = mode;
    d.scale = scale; d.nblocks = nblocks; d.niter = niter;
#ifdef PM_TUNING
    d.timeline = g_timeline;
#endif
    return d;
}

static hipError_t launch_single(
    int dtype, int kind, int ch, int cfg, const SingleArgs& a, hipStream_t s) {
    return with_elem(dtype, [&](auto et) {
        return pm_launch_single<decltype(et)>(kind, ch, cfg, a, s);
    });
}

static hipError_t launch_pack(int dtype, const PackArgs& a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.total + 255) / 256);
    return with_elem(dtype, [&](auto et) {
        hipLaunchKernelGGL(pm_pack_kernel<decltype(et)>, dim3(grid), dim3(256),
                           0, s, a);
        return hipGetLastError();
    });
}

// Geometry of one packed convolution
struct ConvGeom {
    int mode = 0;            // 0 conv, 1 conv-transpose
    int cout = 0, cin = 0, k = 0;
    int cout_pad = 0, cin_pad = 0;
    int M = 0;               // packed rows (cout_pad, or r * cout_pad)
    int ch = 64, kt = 0;
    int r = 0, p = 0;
    bool bias_step = false;  // MRF convs: the stream of every M tile ends
                             // with one bias step (pm_pack_bias_step_kernel)
    size_t weight_elems() const { return (size_t)M * cin_pad * kt; }
    size_t packed_elems() const {
        return weight_elems() + (bias_step ? (size_t)(M / 32) * 512 : 0);
    }
    // copies of the padded bias (one per phase of a conv-transpose)
    int bias_rep() const { return mode == 1 ? r : 1; }
};

// One packed conv: the engine owns w / bias, an op entry points them into the
// caller's workspace
struct Layer {
    ConvGeom geom;
    void* w = nullptr;        // packed (+ bias steps for MRF convs)
    float* bias = nullptr;    // padded (tiled per phase for conv-transpose)
    float* tmp_g = nullptr;   // weight-norm pair awaiting its partner
    float* tmp_v = nullptr;
    bool has_w = false, has_b = false;
    int cfg = 0;
    int dtype = PM_F16;       // MFMA operand type this layer is packed for
};

static hipError_t pack_weights(
    int dtype, const ConvGeom& g, const float* w, void* out, hipStream_t s) {
    PackArgs a;
    a.w = w; a.out = out; a.mode = g.mode;
    a.cout = g.cout; a.cin = g.cin; a.k = g.k;
    a.cout_pad = g.cout_pad; a.cin_pad = g.cin_pad;
    a.mtiles = g.M / 32; a.nch = g.cin_pad / g.ch; a.ch = g.ch; a.kt = g.kt;
    a.r = g.r; a.p = g.p;
    a.bias_step = g.bias_step ? 1 : 0;
    a.total = (long long)g.weight_elems();
    return launch_pack(dtype, a, s);
}

// pm_host.h: the framed DFT's basis as a packed exact-fp32 conv weight
hipError_t pm_dft_pack(const float* w, void* out, int cout, int cout_pad,
                       int cin, int k, hipStream_t s) {
    ConvGeom g;
    g.mode = 0; g.cout = cout; g.cin = cin; g.k = k;
    g.cout_pad = g.M = cout_pad; g.cin_pad = cin; g.kt = g.k; g.ch = 64;
    return pack_weights(PM_F32, g, w, out, s);
}

hipError_t pm_dft_conv(int epi, const PmDftConv& c, hipStream_t s) {
    SingleArgs a = {};
    a.x = c.x; a.out = c.out; a.w = c.w; a.bias = c.bias;
    a.gbias = nullptr; a.gbias_batch = 1;
    a.B = c.B; a.L = c.L; a.Lout = c.Lout; a.Cin = c.Cin; a.M = c.M;
    a.bins = c.bins; a.maxbits = c.maxbits; a.grad = c.grad; a.lrelu = 0;
    a.pad = c.pad; a.phase_r = 0; a.phase_c = 1;
    return pm_launch_stft(epi, a, s);
}

// Write the bias step of every M tile of a packed MRF conv stream
static hipError_t pack_bias_step(
    int dtype, const ConvGeom& g, const float* bias, void* out, hipStream_t s) {
    const int mtiles = g.M / 32;
    const long long per_mt = (long long)g.weight_elems() / mtiles;
    const dim3 grid((mtiles * 512 + 255) / 256), block(256);
    return with_elem(dtype, [&](auto et) {
        hipLaunchKernelGGL(pm_pack_bias_step_kernel<decltype(et)>, grid, block,
                           0, s, bias, out, g.cout, mtiles, per_mt);
        return hipGetLastError();
    });
}

static hipError_t pad_bias(
    const float* src, float* dst, int n, int n_pad, int rep, hipStream_t s) {
    const int total = n_pad * rep;
    hipLaunchKernelGGL(pm_pad_bias_kernel, dim3((total + 255) / 256),
                       dim3(256), 0, s, src, dst, n, n_pad, rep);
    return hipGetLastError();
}

// Pack torch-layout weights and bias into l.w / l.bias (set_weight / set_bias
// receive their halves in either order and call the pieces)
static hipError_t pack_layer(
    const Layer& l, const float* w, const float* bias, hipStream_t s) {
    const ConvGeom& g = l.geom;
    hipError_t e = pack_weights(l.dtype, g, w, l.w, s);
    if (e == hipSuccess)
        e = pad_bias(bias, l.bias, g.cout, g.cout_pad, g.bias_rep(), s);
    if (e == hipSuccess && g.bias_step)
        e = pack_bias_step(l.dtype, g, l.bias, l.w, s);
    return e;
}

static int single_cfg(int M, int ch, int wave64_ok) {
    if (M % 256 == 0 && ch == 64 && wave64_ok) return 0;
    if (M == 128 && ch == 64) return 3;   // whole M in one workgroup
    if (M % 64 == 0) return 1;
    return 2;
}

// ---------------------------------------------------------------------------
// The HiFi-GAN layers: the geometry (and kernel configuration) of each kind
// and its launch, stated once for the engine and the per-kernel entry points
// ---------------------------------------------------------------------------
// Input conv: Conv1d(c_in -> c_out, k 7, pad 3)
static Layer input_layer(int dtype, int c_in, int c_out) {
    Layer l; l.dtype = dtype;
    ConvGeom& g = l.geom;
    g.mode = 0; g.cout = c_out; g.cin = c_in; g.k = g.kt = 7;
    g.cout_pad = g.M = pm_pad32(c_out); g.cin_pad = pm_pad32(c_in);
    g.ch = (g.cin_pad % 64 == 0) ? 64 : 32;
    l.cfg = single_cfg(g.M, g.ch, 1);
    return l;
}

// Upsampler: ConvTranspose1d(c_in -> c_out, k 2 r, stride r) as a polyphase
// GEMM of r phases, two taps each. cfg 4, the wide upsampler
// (conv_upsample_kernel): 16-bit operands, C_in 256 / 512, 256-row M blocks
// whose tap window is uniform; its packing is one chunk of the whole K.
static Layer upsample_layer(int dtype, int c_in, int c_out, int r) {
    Layer l; l.dtype = dtype;
    ConvGeom& g = l.geom;
    g.mode = 1; g.cout = c_out; g.cin = c_in; g.k = 2 * r;
    g.cout_pad = pm_pad32(c_out); g.cin_pad = pm_pad32(c_in);
    g.M = r * g.cout_pad; g.kt = 2; g.r = r; g.p = r / 2;
    g.ch = (g.cin_pad % 64 == 0) ? 64 : 32;
    const bool uniform = ((r / 2) * g.cout_pad) % 64 == 0;
    l.cfg = single_cfg(g.M, g.ch, uniform);
    if (esz(dtype) == 2 && (g.cin_pad == 256 || g.cin_pad == 512) &&
        g.M % 256 == 0 && uniform) {
        l.cfg = 4; g.ch = g.cin_pad;
    }
    return l;
}

// One conv of an MRF Block: Conv1d(C -> C, k K), its bias as a packed step
static Layer mrf_layer(int dtype, int C, int K) {
    Layer l; l.dtype = dtype;
    ConvGeom& g = l.geom;
    g.mode = 0; g.cout = g.cin = C; g.k = g.kt = K;
    g.cout_pad = g.cin_pad = g.M = pm_pad32(C);
    g.ch = std::min(g.M, 64);   // (pm_launch.h: one packing)
    g.bias_step = true;
    return l;
}

// Can this upsampler stage a 16-bit copy of its input as it is
// (SingleArgs::x16)? Only conv_single_kernel does, on 16-bit operands.
static bool takes_x16(const Layer& up) {
    return esz(up.dtype) == 2 && up.cfg != 4;
}

// Speaker conditioning (gbatch, G) as a per-utterance bias (gbatch, pad32(c))
static hipError_t launch_speaker_bias(
    const float* global, const float* w, const float* b, float* gbias,
    int gbatch, int G, int c, hipStream_t s) {
    const int cp = pm_pad32(c);
    hipLaunchKernelGGL(pm_speaker_bias_kernel, dim3((cp + 3) / 4, gbatch),
                       dim3(256), 0, s, global, w, b, gbias, G, c, cp);
    return hipGetLastError();
}

static hipError_t launch_input_conv(
    const Layer& l, const float* x, float* out, const float* gbias, int gbatch,
    int B, int L, const int* lengths, hipStream_t s) {
    const ConvGeom& g = l.geom;
    SingleArgs a = {};
    a.x = x; a.out = out; a.w = l.w; a.bias = l.bias;
    a.gbias = gbias; a.gbias_batch = gbatch;
    a.B = B; a.L = L; a.Lout = L; a.Cin = g.cin_pad; a.M = g.M;
    a.lrelu = 0; a.pad = 3; a.phase_r = 0; a.phase_c = 1;
    a.lengths = lengths; a.len_scale = 1;
    return launch_single(l.dtype, 0, g.ch, l.cfg, a, s);
}

// x (fp32) or, where takes_x16, x16 (the operand values of lrelu(x)); `rate`
// input rows per frame of `lengths`
static hipError_t launch_upsample(
    const Layer& l, const float* x, const void* x16, float* out, int lrelu,
    int B, int L, const int* lengths, int rate, hipStream_t s) {
    const ConvGeom& g = l.geom;
    SingleArgs a = {};
    a.x = x; a.x16 = x16; a.out = out; a.w = l.w; a.bias = l.bias;
    a.gbias = nullptr; a.gbias_batch = 1;
    a.B = B; a.L = L; a.Lout = L; a.Cin = g.cin_pad; a.M = g.M;
    a.lrelu = lrelu; a.pad = 1;
    a.phase_c = g.cout_pad; a.phase_p = g.p; a.phase_r = g.r;
    a.lengths = lengths; a.len_scale = rate;
    // (long batches: the 256-column variant of cfg 3)
    int cfg = l.cfg;
    if (cfg == 3 && esz(l.dtype) == 2 && g.ch == 64 &&
        (long long)B * ((L + 255) / 256) >= 4 * 256)
        cfg = 5;
    return launch_single(l.dtype, 1, g.ch, cfg, a, s);
}

// Output layer on x (B, L, pad32(C)), w (1, C, 7): the 32-channel kernel for
// exactly 32 channels, the generic one otherwise
static hipError_t launch_out_conv(
    const float* x, const float* w, float* out, int B, int L, int C,
    const int* lengths, int rate, hipStream_t s) {
    constexpr int T32 = 128, TH = 256;   // (T32: 38 KB of LDS, four per CU)
    const int Cp = pm_pad32(C);
    if (C == 32)
        hipLaunchKernelGGL(pm_out_conv32_kernel<T32>,
                           dim3((L + T32 * 2 - 1) / (T32 * 2), B), dim3(T32),
                           (size_t)32 * PM_OUT32_RL(T32) * sizeof(float), s, x,
                           w, out, L, lengths, rate);
    else
        hipLaunchKernelGGL(pm_out_conv_kernel<TH>, dim3((L + TH - 1) / TH, B),
                           dim3(TH),
                           ((size_t)(TH + 6) * (Cp + 1) + 7 * Cp) * sizeof(float),
                           s, x, w, out, L, Cp, C, lengths, rate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
struct Stage {
    int cin = 0, cout = 0, cout_pad = 0, r = 0, k = 0;
    int dtype = PM_F16;       // operand type of the stage (upsampler + MRF)
    Layer up;
    Layer c1[PM_MAX_RESBLOCKS][PM_MAX_DILATIONS];
    Layer c2[PM_MAX_RESBLOCKS][PM_MAX_DILATIONS];
};

struct pm_hifigan_s {
    pm_hifigan_config cfg;
    int dtype = PM_F16;
    int cfp = 0, c0 = 0, c0p = 0, hop = 1;
    Layer in_conv;
    float* spk_w = nullptr; float* spk_b = nullptr;
    bool has_spk_w = false, has_spk_b = false;
    float* out_w = nullptr; bool has_out_w = false;
    int c_last = 0;
    std::vector<Stage> stages;
    bool finalized = false;
    // ---- optional per-launch timing with HIP events (bench.py roofline) ----
    bool profile = false;
    std::string profile_only;            // bracket this label's launches only
    std::vector<hipEvent_t> events;      // pool, grown on demand
    size_t events_used = 0;
    struct Mark { std::string label; double flops, bytes; size_t e0, e1; };
    std::vector<Mark> marks;             // launches since the last collect
    struct Acc { long long count = 0; double ms = 0, flops = 0, bytes = 0; };
    std::map<std::string, Acc> totals;
    std::string report;
};

static int prof_event(pm_hifigan_t h, hipStream_t s, size_t* index) {
    if (h->events_used == h->events.size()) {
        hipEvent_t e;
        PM_HIP_TRY(hipEventCreate(&e));
        h->events.push_back(e);
    }
    *index = h->events_used++;
    PM_HIP_TRY(hipEventRecord(h->events[*index], s));
    return PM_OK;
}

// Bracket the launch(es) issued by `body` with two events on the same stream
#define PROF(h, s, label_, flops_, bytes_, body)                             \
    do {                                                                     \
        size_t e0_ = 0, e1_ = 0;                                             \
        const bool on_ = (h)->profile &&                                     \
            ((h)->profile_only.empty() || (h)->profile_only == (label_));    \
        if (on_) { int r_ = prof_event(h, s, &e0_); if (r_) return r_; }     \
        body;                                                                \
        if (on_) {                                                           \
            int r_ = prof_event(h, s, &e1_); if (r_) return r_;              \
            (h)->marks.push_back({label_, (double)(flops_), (double)(bytes_), e0_, e1_}); \
        }                                                                    \
    } while (0)

static void free_layer(Layer& l) {
    if (l.w) hipFree(l.w);
    if (l.bias) hipFree(l.bias);
    if (l.tmp_g) hipFree(l.tmp_g);
    if (l.tmp_v) hipFree(l.tmp_v);
    l = Layer();
}

extern "C" int pm_version(void) { return PM_VERSION; }
extern "C" const char* pm_last_error(void) { return g_error; }

extern "C" int pm_hifigan_create(
    const pm_hifigan_config* c, pm_hifigan_t* out) {
    if (!c || !out) return pm_fail(PM_EINVAL, "null argument");
    if (c->compute_dtype < 0 || c->compute_dtype > PM_F16UX)
        return pm_fail(PM_EINVAL, "compute_dtype %d unknown", c->compute_dtype);
    if (c->num_stages < 1 || c->num_stages > PM_MAX_STAGES ||
        c->num_resblocks < 1 || c->num_resblocks > PM_MAX_RESBLOCKS ||
        c->num_dilations < 1 || c->num_dilations > PM_MAX_DILATIONS)
        return pm_fail(PM_EINVAL,
                       "stage / resblock / dilation count out of range");
    if (c->num_features < 1 || c->global_channels < 1 ||
        c->initial_channels < (1 << c->num_stages))
        return pm_fail(PM_EINVAL, "bad channel configuration");
    for (int j = 0; j < c->num_resblocks; ++j) {
        const int k = c->resblock_kernel_sizes[j];
        if (k != 3 && k != 7 && k != 11)
            return pm_fail(PM_EINVAL,
                           "resblock kernel size %d unsupported (3, 7, 11)", k);
        for (int n = 0; n < c->num_dilations; ++n) {
            const int d = c->resblock_dilations[j][n];
            if (d < 1 || d > 5)
                return pm_fail(PM_EINVAL, "dilation %d unsupported (1..5)", d);
        }
    }
    for (int i = 0; i < c->num_stages; ++i)
        if (c->stage_compute_dtype[i] < 0 ||
            c->stage_compute_dtype[i] > 1 + PM_F16UX)
            return pm_fail(PM_EINVAL, "stage_compute_dtype[%d] = %d unknown", i,
                           c->stage_compute_dtype[i]);
    auto* h = new pm_hifigan_s();
    h->cfg = *c;
    h->dtype = c->compute_dtype;
    h->cfp = pm_pad32(c->num_features);
    h->c0 = c->initial_channels;
    h->c0p = pm_pad32(h->c0);
    h->in_conv = input_layer(block_dtype(h->dtype), c->num_features, h->c0);
    h->hop = 1;
    h->stages.resize(c->num_stages);
    for (int i = 0; i < c->num_stages; ++i) {
        Stage& s = h->stages[i];
        s.r = c->upsample_rates[i];
        s.k = c->upsample_kernel_sizes[i];
        const int code = c->stage_compute_dtype[i]
            ? c->stage_compute_dtype[i] - 1 : h->dtype;
        s.dtype = block_dtype(code);
        if (s.r < 2 || (s.r & 1) || s.k != 2 * s.r) {
            delete h;
            return pm_fail(PM_EINVAL,
                           "upsample stage %d: rate %d kernel %d unsupported "
                           "(need even rate and kernel == 2 * rate)", i,
                           c->upsample_rates[i], c->upsample_kernel_sizes[i]);
        }
        s.cin = h->c0 >> i;
        s.cout = h->c0 >> (i + 1);
        s.cout_pad = pm_pad32(s.cout);
        if (s.cout_pad != 32 && s.cout_pad != 64 && s.cout_pad != 128 &&
            s.cout_pad != 256) {
            delete h;
            return pm_fail(PM_EINVAL,
                           "stage %d: %d channels unsupported (padded channel "
                           "count must be 32, 64, 128 or 256)", i, s.cout);
        }
        h->hop *= s.r;
        s.up = upsample_layer(up_dtype(code), s.cin, s.cout, s.r);
        for (int j = 0; j < c->num_resblocks; ++j)
            for (int n = 0; n < c->num_dilations; ++n)
                s.c1[j][n] = s.c2[j][n] =
                    mrf_layer(s.dtype, s.cout, c->resblock_kernel_sizes[j]);
    }
    h->c_last = h->stages.back().cout;
    if (pm_pad32(h->c_last) > 64) {
        delete h;
        return pm_fail(PM_EINVAL, "output conv supports <= 64 input channels");
    }
    *out = h;
    return PM_OK;
}

extern "C" int pm_hifigan_destroy(pm_hifigan_t h) {
    if (!h) return PM_OK;
    free_layer(h->in_conv);
    if (h->spk_w) hipFree(h->spk_w);
    if (h->spk_b) hipFree(h->spk_b);
    if (h->out_w) hipFree(h->out_w);
    for (auto e : h->events) hipEventDestroy(e);
    for (auto& s : h->stages) {
        free_layer(s.up);
        for (int j = 0; j < PM_MAX_RESBLOCKS; ++j)
            for (int n = 0; n < PM_MAX_DILATIONS; ++n) {
                free_layer(s.c1[j][n]);
                free_layer(s.c2[j][n]);
            }
    }
    delete h;
    return PM_OK;
}

static size_t numel(const int64_t* shape, int ndim) {
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    return n;
}

int pm_copy_dev(float** dst, const float* src, size_t n, hipStream_t s) {
    if (!*dst) PM_HIP_TRY(hipMalloc((void**)dst, n * sizeof(float)));
    PM_HIP_TRY(hipMemcpyAsync(*dst, src, n * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
    return PM_OK;
}

// Pack a folded torch-layout weight into the layer
static int set_weight(
    pm_hifigan_t h, Layer& l, const float* w, const int64_t* shape, int ndim,
    hipStream_t s, const char* name) {
    const ConvGeom& g = l.geom;
    const int64_t d0 = g.mode == 0 ? g.cout : g.cin;
    const int64_t d1 = g.mode == 0 ? g.cin : g.cout;
    if (ndim != 3 || shape[0] != d0 || shape[1] != d1 || shape[2] != g.k)
        return pm_fail(PM_EINVAL, "%s: expected shape (%lld, %lld, %d)", name,
                       (long long)d0, (long long)d1, g.k);
    const size_t bytes = g.packed_elems() * wsz(l.dtype);
    if (!l.w) PM_HIP_TRY(hipMalloc(&l.w, bytes));
    PM_HIP_TRY(pack_weights(l.dtype, g, w, l.w, s));
    l.has_w = true;
    if (g.bias_step && l.has_b)
        PM_HIP_TRY(pack_bias_step(l.dtype, g, l.bias, l.w, s));
    return PM_OK;
}

static int set_bias(
    pm_hifigan_t h, Layer& l, const float* b, const int64_t* shape, int ndim,
    hipStream_t s, const char* name) {
    const ConvGeom& g = l.geom;
    if (ndim != 1 || shape[0] != g.cout)
        return pm_fail(PM_EINVAL, "%s: expected shape (%d)", name, g.cout);
    const int rep = g.bias_rep();
    if (!l.bias)
        PM_HIP_TRY(hipMalloc((void**)&l.bias,
                             (size_t)g.cout_pad * rep * sizeof(float)));
    PM_HIP_TRY(pad_bias(b, l.bias, g.cout, g.cout_pad, rep, s));
    l.has_b = true;
    if (g.bias_step && l.has_w)
        PM_HIP_TRY(pack_bias_step(l.dtype, g, l.bias, l.w, s));
    return PM_OK;
}

static int set_norm_part(
    pm_hifigan_t h, Layer& l, bool is_g, const float* t, const int64_t* shape,
    int ndim, hipStream_t s, const char* name) {
    const ConvGeom& g = l.geom;
    const int64_t rows = g.mode == 0 ? g.cout : g.cin;
    const int64_t cols = (g.mode == 0 ? g.cin : g.cout) * (int64_t)g.k;
    if (is_g) {
        if (ndim != 3 || shape[0] != rows || shape[1] != 1 || shape[2] != 1)
            return pm_fail(PM_EINVAL, "%s: expected shape (%lld, 1, 1)", name,
                           (long long)rows);
        int rc = pm_copy_dev(&l.tmp_g, t, rows, s);
        if (rc) return rc;
    } else {
        if (ndim != 3 || (int64_t)numel(shape, ndim) != rows * cols ||
            shape[0] != rows)
            return pm_fail(PM_EINVAL, "%s: unexpected weight_v shape", name);
        int rc = pm_copy_dev(&l.tmp_v, t, rows * cols, s);
        if (rc) return rc;
    }
    if (l.tmp_g && l.tmp_v) {
        float* folded = nullptr;
        PM_HIP_TRY(hipMalloc((void**)&folded, rows * cols * sizeof(float)));
        hipLaunchKernelGGL(pm_fold_kernel, dim3((unsigned)rows), dim3(256), 0,
                           s, l.tmp_g, l.tmp_v, folded, (int)cols);
        PM_HIP_TRY(hipGetLastError());
        const int64_t wshape[3] = {
            rows, g.mode == 0 ? (int64_t)g.cin : (int64_t)g.cout, g.k};
        int rc = set_weight(h, l, folded, wshape, 3, s, name);
        PM_HIP_TRY(hipStreamSynchronize(s));
        hipFree(folded);
        hipFree(l.tmp_g); hipFree(l.tmp_v);
        l.tmp_g = l.tmp_v = nullptr;
        if (rc) return rc;
    }
    return PM_OK;
}

static int set_layer_tensor(
    pm_hifigan_t h, Layer& l, const char* leaf, const float* t,
    const int64_t* shape, int ndim, hipStream_t s, const char* name) {
    if (!strcmp(leaf, "weight")) return set_weight(h, l, t, shape, ndim, s, name);
    if (!strcmp(leaf, "bias")) return set_bias(h, l, t, shape, ndim, s, name);
    if (!strcmp(leaf, "weight_g"))
        return set_norm_part(h, l, true, t, shape, ndim, s, name);
    if (!strcmp(leaf, "weight_v"))
        return set_norm_part(h, l, false, t, shape, ndim, s, name);
    return pm_fail(PM_EINVAL, "%s: unknown tensor", name);
}

extern "C" int pm_hifigan_load_tensor(
    pm_hifigan_t h, const char* name, const float* dev, const int64_t* shape,
    int ndim, void* stream) {
    if (!h || !name || !dev || !shape)
        return pm_fail(PM_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int ns = (int)h->stages.size();
    int rc = PM_EINVAL;
    int i = 0, j = 0, n = 0, which = 0;
    char leaf[32] = "";
    if (!strncmp(name, "input_feature_conv.", 19)) {
        rc = set_layer_tensor(h, h->in_conv, name + 19, dev, shape, ndim, s, name);
    } else if (!strcmp(name, "input_speaker_conv.weight")) {
        if (ndim != 3 || shape[0] != h->c0 ||
            shape[1] != h->cfg.global_channels || shape[2] != 1)
            return pm_fail(PM_EINVAL, "%s: unexpected shape", name);
        rc = pm_copy_dev(&h->spk_w, dev, numel(shape, ndim), s);
        h->has_spk_w = rc == PM_OK;
    } else if (!strcmp(name, "input_speaker_conv.bias")) {
        if (ndim != 1 || shape[0] != h->c0)
            return pm_fail(PM_EINVAL, "%s: unexpected shape", name);
        rc = pm_copy_dev(&h->spk_b, dev, numel(shape, ndim), s);
        h->has_spk_b = rc == PM_OK;
    } else if (sscanf(name, "model.%d.model.2.model.%d.convs%d.%d.%31s", &i,
                      &j, &which, &n, leaf) == 5) {
        if (i < 0 || i >= ns || j < 0 || j >= h->cfg.num_resblocks || n < 0 ||
            n >= h->cfg.num_dilations || which < 1 || which > 2)
            return pm_fail(PM_EINVAL, "%s: index out of range", name);
        Layer& l = (which == 1 ? h->stages[i].c1 : h->stages[i].c2)[j][n];
        rc = set_layer_tensor(h, l, leaf, dev, shape, ndim, s, name);
    } else if (sscanf(name, "model.%d.model.1.%31s", &i, leaf) == 2) {
        if (i < 0 || i >= ns)
            return pm_fail(PM_EINVAL, "%s: stage out of range", name);
        rc = set_layer_tensor(h, h->stages[i].up, leaf, dev, shape, ndim, s, name);
    } else if (sscanf(name, "model.%d.%31s", &i, leaf) == 2 && i == ns + 1 &&
               !strcmp(leaf, "weight")) {
        if (ndim != 3 || shape[0] != 1 || shape[1] != h->c_last ||
            shape[2] != 7)
            return pm_fail(PM_EINVAL, "%s: expected shape (1, %d, 7)", name,
                           h->c_last);
        rc = pm_copy_dev(&h->out_w, dev, numel(shape, ndim), s);
        h->has_out_w = rc == PM_OK;
    } else {
        return pm_fail(PM_EINVAL, "%s: not a HiFiGAN state-dict key", name);
    }
    if (rc != PM_OK) return rc;
    PM_HIP_TRY(hipStreamSynchronize(s));
    h->finalized = false;
    return PM_OK;
}

extern "C" int pm_hifigan_finalize(pm_hifigan_t h, void* stream) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    auto check = [](const Layer& l, const std::string& what) -> int {
        if (!l.has_w)
            return pm_fail(PM_ESTATE,
                           "missing tensor: %s weight", what.c_str());
        if (!l.has_b)
            return pm_fail(PM_ESTATE, "missing tensor: %s bias", what.c_str());
        return PM_OK;
    };
    int rc;
    if ((rc = check(h->in_conv, "input_feature_conv"))) return rc;
    if (!h->has_spk_w || !h->has_spk_b)
        return pm_fail(PM_ESTATE, "missing tensor: input_speaker_conv");
    if (!h->has_out_w) return pm_fail(PM_ESTATE, "missing tensor: output conv");
    for (size_t i = 0; i < h->stages.size(); ++i) {
        Stage& s = h->stages[i];
        if ((rc = check(s.up, "model." + std::to_string(i) + ".model.1")))
            return rc;
        for (int j = 0; j < h->cfg.num_resblocks; ++j)
            for (int n = 0; n < h->cfg.num_dilations; ++n) {
                const std::string base = "model." + std::to_string(i) +
                    ".model.2.model." + std::to_string(j);
                if ((rc = check(s.c1[j][n], base + ".convs1." + std::to_string(n))))
                    return rc;
                if ((rc = check(s.c2[j][n], base + ".convs2." + std::to_string(n))))
                    return rc;
            }
    }
    PM_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    h->finalized = true;
    return PM_OK;
}

extern "C" int pm_hifigan_hopsize(pm_hifigan_t h) { return h ? h->hop : 0; }
extern "C" int pm_hifigan_features_cl_channels(pm_hifigan_t h) {
    return h ? h->cfp : 0;
}

// channels-last features | speaker bias | four activation buffers | the
// skewed walks' scratch (or none)
struct Plan {
    float *feat, *gbias, *buf[4];
    char* scratch;
    size_t scratch_bytes, total;
};

// Scratch of the skewed whole-Block walk: one workgroup per (utterance,
// segment), at most max(B, CUs) of them (pm_launch.h)
static size_t walk_scratch_bytes(int B) {
    const int cus = pm_device_cus();
    return (size_t)std::max(B, cus > 0 ? cus : 256) * PM_SKEW_WG_SCRATCH;
}

static Plan make_plan(pm_hifigan_t h, int B, int T, void* base) {
    Plan p;
    size_t mx = (size_t)T * h->c0p;
    size_t L = T;
    for (auto& s : h->stages) {
        L *= s.r;
        mx = std::max(mx, L * (size_t)s.cout_pad);
    }
    PmCarve c(base);
    p.feat = c.take<float>((size_t)B * T * h->cfp);
    p.gbias = c.take<float>((size_t)B * h->c0p);
    for (float*& b : p.buf) b = c.take<float>((size_t)B * mx);
    // (the skewed walks are only planned with >= 4 steps per segment,
    // max(1, CUs / B) segments per utterance: short calls - a streaming
    // frame, a single 2 s utterance - carry no scratch. The planner tests
    // each stage against its own geometry's step; the workspace, sized once
    // for all stages, takes the longest stage and the narrowest step the
    // production heuristics skew, 256 columns - C = 128, and the 4-byte
    // layouts at C = 64 -, so that no stage the planner would skew lacks it)
    {
        const int cus = pm_device_cus();
        const size_t nseg = std::max(1, (cus > 0 ? cus : 256) / B);
        p.scratch_bytes = pm_force().walk_nseg || pm_force().skew > 0 ||
                          L / 256 / nseg >= 4
            ? walk_scratch_bytes(B) : 0;   // (a forced walk / skew: tests)
    }
    p.scratch = p.scratch_bytes ? c.take<char>(p.scratch_bytes) : nullptr;
    p.total = c.used;
    return p;
}

extern "C" size_t pm_hifigan_workspace_bytes(pm_hifigan_t h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    return make_plan(h, B, T, nullptr).total;
}

static int forward_impl(
    pm_hifigan_t h, const float* features, bool features_cl, const float* g,
    int gbatch, float* out, int B, int T, void* ws, size_t ws_bytes,
    hipStream_t s, const int* lengths = nullptr) {
    if (!h || !features || !g || !out || !ws)
        return pm_fail(PM_EINVAL, "null argument");
    if (!h->finalized)
        return pm_fail(PM_ESTATE, "pm_hifigan_finalize not called");
    if (B < 1 || T < 1) return pm_fail(PM_EINVAL, "empty batch or sequence");
    if (gbatch != 1 && gbatch != B)
        return pm_fail(PM_EINVAL, "global_batch must be 1 or batch");
    const Plan p = make_plan(h, B, T, ws);
    if (ws_bytes < p.total)
        return pm_fail(PM_ENOMEM,
                       "workspace %zu < required %zu", ws_bytes, p.total);
    float* const* buf = p.buf;

    const float* feat_cl = features;
    if (!features_cl) {
        dim3 grid((T + 31) / 32, h->cfp / 32, B);
        PROF(h, s, "to_channels_last", 0,
             (double)B * T * (h->cfg.num_features + h->cfp) * 4, {
            hipLaunchKernelGGL(pm_to_channels_last_kernel, grid, dim3(256), 0,
                               s, features, p.feat, h->cfg.num_features, T,
                               h->cfp);
            PM_HIP_TRY(hipGetLastError());
        });
        feat_cl = p.feat;
    }
    // speaker conditioning as a per-utterance bias of the input conv
    PM_HIP_TRY(launch_speaker_bias(g, h->spk_w, h->spk_b, p.gbias, gbatch,
                                   h->cfg.global_channels, h->c0, s));
    PROF(h, s, "input_conv", 2.0 * h->c0 * h->cfg.num_features * 7 * B * T,
         (double)B * T * (h->cfg.num_features + h->c0) * 4, {
        PM_HIP_TRY(launch_input_conv(h->in_conv, feat_cl, buf[0], p.gbias,
                                     gbatch, B, T, lengths, s));
    });
    int xi = 0;        // index of the buffer holding the stage input
    // the stage input once more, as the 16-bit operand values of the next
    // upsampler (written by the previous stage's last Block launch when that
    // is a skewed walk - Block3Args::act16), or null
    const void* x16 = nullptr;
    int L = T;
    int rate = 1;      // samples per frame at the current stage
    const float scale = 1.f / (float)h->cfg.num_resblocks;
    for (auto& st : h->stages) {
        const int ui = (xi + 1) & 3, ai = (xi + 2) & 3, bi = (xi + 3) & 3;
        {
            char label[64];
            snprintf(label, sizeof(label), "convT_c%d_r%d", st.cin, st.r);
            PROF(h, s, label, 2.0 * st.cin * st.cout * st.k * B * L,
                 (double)B * L * (st.cin + (double)st.r * st.cout) * 4, {
                PM_HIP_TRY(launch_upsample(st.up, buf[xi], x16, buf[ui], 1, B,
                                           L, lengths, rate, s));
            });
            x16 = nullptr;
        }
        L *= st.r;
        rate *= st.r;
        const int si = xi;   // stage input is dead after the upsampler
        // the MRF: U -> S, planned once (pm_launch.h)
        const int nb = h->cfg.num_resblocks, ni = h->cfg.num_dilations;
        PmStage d = stage_desc(st.cout_pad, buf[ui], buf[si], B, L, 1, scale,
                               nb, ni);
        d.lengths = lengths; d.len_scale = rate;
        d.scratch = p.scratch;
        d.scratch_bytes = p.scratch_bytes;
        for (int j = 0; j < nb; ++j) {
            d.blk[j].K = h->cfg.resblock_kernel_sizes[j];
            for (int n = 0; n < ni; ++n) {
                d.blk[j].w1[n] = st.c1[j][n].w;
                d.blk[j].w2[n] = st.c2[j][n].w;
                d.blk[j].dil[n] = h->cfg.resblock_dilations[j][n];
            }
        }
        // The stage's last Block completes `out`, whose only reader is the
        // next stage's upsampler - which stages cvt(lrelu(out)): let the
        // kernel write exactly that (half the bytes out, half the bytes in,
        // no staging VALU) when the upsampler is the conv_single_kernel of a
        // 16-bit stage.
        const size_t next = &st - &h->stages[0] + 1;
        if (nb > 1 && next < h->stages.size() &&
            takes_x16(h->stages[next].up)) {
            d.act16 = buf[ai];      // (free: no pair iterations)
            d.act16_type = h->stages[next].up.dtype;
        }
        PmPlan plan;
        PM_HIP_TRY(plan_stage(st.dtype, d, pm_fusion_level(), &plan));
        if (plan.mrf) {
            double flops = 0;
            for (int j = 0; j < nb; ++j)
                flops += ni * 4.0 * st.cout * st.cout * d.blk[j].K * B * L;
            char label[64];
            snprintf(label, sizeof(label), "mrf_c%d", st.cout);
            PROF(h, s, label, flops, (double)B * L * st.cout * 4 * 2, {
                PM_HIP_TRY(launch_mrf(st.dtype, plan.block[0], d, s));
            });
        }
        for (int j = 0; !plan.mrf && j < nb; ++j) {
            const int K = d.blk[j].K;
            const double bytes = (double)B * L * st.cout * 4 * (j ? 3 : 2);
            char label[64];
            if (plan.block[j].kernel != PM_PAIRS) {
                // whole Block (all dilations) in one kernel: U -> S
                snprintf(label, sizeof(label), "block_c%d_k%d", st.cout, K);
                PROF(h, s, label, ni * 4.0 * st.cout * st.cout * K * B * L, bytes, {
                    PM_HIP_TRY(launch_block3(st.dtype, plan.block[j], d, j, s));
                });
                if (plan.block[j].act16) x16 = buf[ai];
                continue;
            }
            const float* src = buf[ui];
            for (int n = 0; n < ni; ++n) {
                const bool last = n == ni - 1;
                float* dst = last ? buf[si] : ((n & 1) ? buf[bi] : buf[ai]);
                PairArgs a = {};
                a.x = src; a.out = dst;
                a.w1 = d.blk[j].w1[n];
                a.w2 = d.blk[j].w2[n];
                a.B = B; a.L = L;
                a.dilation = d.blk[j].dil[n];
                a.mode = last ? (j == 0 ? 1 : 2) : 0;
                a.scale = scale;
                a.lengths = lengths; a.len_scale = rate;
                snprintf(label, sizeof(label), "pair_c%d_k%d", st.cout, K);
                PROF(h, s, label, 4.0 * st.cout * st.cout * K * B * L,
                     (double)B * L * st.cout * 4 * (a.mode == 2 ? 3 : 2), {
                    PM_HIP_TRY(launch_pair(st.dtype, st.cout_pad, K, a, s));
                });
                src = dst;
            }
        }
        xi = si;
    }
    PROF(h, s, "out_conv_tanh", 2.0 * h->c_last * 7 * B * L,
         (double)B * L * (h->c_last + 1) * 4, {
        PM_HIP_TRY(launch_out_conv(buf[xi], h->out_w, out, B, L, h->c_last,
                                   lengths, rate, s));
    });
    return PM_OK;
}

// ---- profiling API ---------------------------------------------------------
extern "C" int pm_hifigan_profile_enable(pm_hifigan_t h, int enable) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    h->profile = enable != 0;
    return PM_OK;
}

// Restrict the event pairs to the launches reported under `label` (null or
// "": all of them): a timed region then carries two events per step instead
// of two per launch.
extern "C" int pm_hifigan_profile_only(pm_hifigan_t h, const char* label) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    h->profile_only = label ? label : "";
    return PM_OK;
}

// Synchronise, fold the event pairs recorded since the last call into the
// per-label totals and recycle the events. Call between forwards at will.
extern "C" int pm_hifigan_profile_collect(pm_hifigan_t h) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    for (auto& m : h->marks) {
        PM_HIP_TRY(hipEventSynchronize(h->events[m.e1]));
        float ms = 0.f;
        PM_HIP_TRY(hipEventElapsedTime(&ms, h->events[m.e0], h->events[m.e1]));
        auto& acc = h->totals[m.label];
        acc.count += 1; acc.ms += ms; acc.flops += m.flops; acc.bytes += m.bytes;
    }
    h->marks.clear();
    h->events_used = 0;
    return PM_OK;
}

extern "C" int pm_hifigan_profile_reset(pm_hifigan_t h) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    int rc = pm_hifigan_profile_collect(h);
    h->totals.clear();
    return rc;
}

// Text report, one line per kernel label:
//   label launches total_ms algorithmic_flops algorithmic_bytes
extern "C" const char* pm_hifigan_profile_report(pm_hifigan_t h) {
    if (!h) return "";
    h->report.clear();
    char line[256];
    for (auto& kv : h->totals) {
        snprintf(line, sizeof(line), "%s %lld %.6f %.6e %.6e\n",
                 kv.first.c_str(), kv.second.count, kv.second.ms,
                 kv.second.flops, kv.second.bytes);
        h->report += line;
    }
    return h->report.c_str();
}

extern "C" int pm_hifigan_forward(
    pm_hifigan_t h, const float* features, const float* g, int gbatch,
    float* out, int B, int T, void* ws, size_t ws_bytes, void* stream) {
    return forward_impl(h, features, false, g, gbatch, out, B, T, ws, ws_bytes,
                        (hipStream_t)stream);
}

extern "C" int pm_hifigan_forward_cl(
    pm_hifigan_t h, const float* features_cl, const float* g, int gbatch,
    float* out, int B, int T, void* ws, size_t ws_bytes, void* stream) {
    return forward_impl(h, features_cl, true, g, gbatch, out, B, T, ws,
                        ws_bytes, (hipStream_t)stream);
}

// Ragged batch: utterance b is lengths[b] <= T frames long inside the padded
// (B, T, ...) tensors. Every kernel treats frames >= lengths[b] as outside
// the sequence (the convolutions' zero padding), so out[b, :, :256 lengths[b]]
// is bit-identical to synthesising utterance b alone; the tail is zeros.
extern "C" int pm_hifigan_forward_ragged(
    pm_hifigan_t h, const float* features, int features_cl, const float* g,
    int gbatch, const int* lengths, float* out, int B, int T, void* ws,
    size_t ws_bytes, void* stream) {
    if (!lengths) return pm_fail(PM_EINVAL, "null lengths");
    return forward_impl(h, features, features_cl != 0, g, gbatch, out, B, T,
                        ws, ws_bytes, (hipStream_t)stream, lengths);
}

// ---- the engine as pm_stream.hip sees it (pm_host.h) -----------------------
const pm_hifigan_config* pm_hifigan_config_of(pm_hifigan_t h) {
    return &h->cfg;
}

int pm_hifigan_forward_window(
    pm_hifigan_t h, const float* features_cl, const float* g, int gbatch,
    float* out, int B, int T, void* ws, size_t ws_bytes, hipStream_t s) {
    return forward_impl(h, features_cl, true, g, gbatch, out, B, T, ws,
                        ws_bytes, s);
}

// ---------------------------------------------------------------------------
// conditioning
// ---------------------------------------------------------------------------
extern "C" int pm_prepare_features(
    const float* loudness, const float* pitch, const float* periodicity,
    const float* ppg, const float* pitch_edges, const float* pitch_table,
    float* out_ref, float* out_cl, int B, int T, int F, int P, int NB, int E,
    int bands, int cl_channels, int sparse_method, float ppg_threshold,
    float fmin, float fmax, float min_db, float ref_db, float period_rate,
    void* stream) {
    if (!loudness || !pitch || !periodicity || !ppg || !pitch_edges ||
        !pitch_table || (!out_ref && !out_cl))
        return pm_fail(PM_EINVAL, "null argument");
    if (B < 1 || T < 1 || P < 2 || bands < 1 || bands > 16 || F < bands)
        return pm_fail(PM_EINVAL, "bad feature dimensions");
    if (sparse_method < PM_SPARSE_NONE || sparse_method > PM_SPARSE_TOPK)
        return pm_fail(PM_EINVAL, "sparse_method %d unknown", sparse_method);
    const int C = P + E + bands + 1 + (period_rate > 0.f ? 1 : 0);
    if (out_cl && cl_channels < C)
        return pm_fail(PM_EINVAL, "cl_channels %d < %d", cl_channels, C);
    FeatureArgs a;
    a.loudness = loudness; a.pitch = pitch; a.periodicity = periodicity;
    a.ppg = ppg; a.pitch_edges = pitch_edges; a.pitch_table = pitch_table;
    a.out_cl = out_cl; a.out_ref = out_ref;
    a.B = B; a.T = T; a.F = F; a.P = P; a.NB = NB; a.E = E; a.bands = bands;
    a.Cpad = cl_channels;
    const double step = (double)F / (double)bands;   // generator.py:174
    for (int b = 0; b <= bands; ++b) a.band_start[b] = (int)(b * step);
    a.sparse_method = sparse_method;
    a.rank_below = a.rank_above = 0; a.rank_weight = 0.f;
    a.threshold = ppg_threshold; a.topk = 0;
    if (sparse_method == PM_SPARSE_PERCENTILE) {
        if (!(ppg_threshold >= 0.f && ppg_threshold <= 1.f))
            return pm_fail(PM_EINVAL, "percentile threshold must be in [0, 1]");
        // torch.quantile(..., interpolation='linear') in the tensor's dtype
        const float rank = ppg_threshold * (float)(P - 1);
        a.rank_below = (int)floorf(rank);
        a.rank_above = (int)ceilf(rank);
        a.rank_weight = rank - floorf(rank);
    } else if (sparse_method == PM_SPARSE_TOPK) {
        a.topk = (int)ppg_threshold;
        if (a.topk < 1 || a.topk > P)
            return pm_fail(PM_EINVAL, "topk must be in [1, %d]", P);
    }
    a.fmin = fmin; a.fmax = fmax; a.min_db = min_db;
    a.db_range = ref_db - min_db;
    a.period_rate = period_rate;
    constexpr int FR = 64;     // frames per workgroup
    const int width = a.Cpad > C ? a.Cpad : C;
    const size_t smem = ((size_t)P * FR + (size_t)FR * (width + 1) + 6 * FR) *
                        sizeof(float);
    hipLaunchKernelGGL(pm_prepare_features_kernel<FR>,
                       dim3((T + FR - 1) / FR, B), dim3(256), smem,
                       (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_prepare_global_features(
    const int64_t* speakers, const float* sbr, const float* lr,
    const float* table, float* out, int B, int S, int num_speakers,
    void* stream) {
    if (!speakers || !table || !out) return pm_fail(PM_EINVAL, "null argument");
    if (B < 1 || S < 1 || num_speakers < 1)
        return pm_fail(PM_EINVAL, "bad dimensions");
    hipLaunchKernelGGL(pm_global_features_kernel, dim3(B), dim3(256), 0,
                       (hipStream_t)stream, (const long long*)speakers, sbr,
                       lr, table, out, B, S, num_speakers);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_prepare_global_features_linear(
    const float* emb, const float* weight, const float* bias,
    const float* sbr, const float* lr, float* out, int B, int E, int S,
    void* stream) {
    if (!emb || !weight || !bias || !out)
        return pm_fail(PM_EINVAL, "null argument");
    if (B < 1 || E < 1 || S < 1) return pm_fail(PM_EINVAL, "bad dimensions");
    hipLaunchKernelGGL(pm_global_features_linear_kernel,
                       dim3((S + 3) / 4, B), dim3(256), 0,
                       (hipStream_t)stream, emb, weight, bias, sbr, lr, out, B,
                       E, S);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// ---------------------------------------------------------------------------
// per-kernel entry points
// ---------------------------------------------------------------------------
// One Block iteration: two packed weight streams (fp32-sized, + bias steps)
// and two padded biases
struct IterationLayout { float *w1, *w2, *b1, *b2; size_t total; };
static IterationLayout iteration_layout(int c_in, int c_out, int k,
                                        void* base) {
    const size_t ci = pm_pad32(c_in), co = pm_pad32(c_out);
    PmCarve c(base);
    return {c.take<float>(ci * co * k + co * 16),
            c.take<float>(ci * co * k + co * 16), c.take<float>(co * 64),
            c.take<float>(co * 64), c.used};
}

extern "C" size_t pm_op_workspace_bytes(int c_in, int c_out, int k) {
    return iteration_layout(c_in, c_out, k, nullptr).total;
}

// Pack one Block iteration - conv1 and conv2 weights (C, C, K) and biases (C)
// - into the pm_op_workspace_bytes(C, C, K) at `base`; *p1 / *p2: the two
// packed streams, their bias steps included
static int pack_iteration(
    int dtype, int C, int K, const float* w1, const float* b1, const float* w2,
    const float* b2, char* base, hipStream_t s, const void** p1,
    const void** p2) {
    const IterationLayout l = iteration_layout(C, C, K, base);
    Layer conv = mrf_layer(dtype, C, K);
    conv.w = l.w1; conv.bias = l.b1;
    PM_HIP_TRY(pack_layer(conv, w1, b1, s));
    conv.w = l.w2; conv.bias = l.b2;
    PM_HIP_TRY(pack_layer(conv, w2, b2, s));
    *p1 = l.w1; *p2 = l.w2;
    return PM_OK;
}

static int block_iteration_cl_impl(
    int dtype, const float* x, float* out, const float* w1, const float* b1,
    const float* w2, const float* b2, const int* lengths, int B, int L, int C,
    int K, int d, int mode, float scale, void* ws, size_t ws_bytes,
    void* stream) {
    if (!x || !out || !w1 || !b1 || !w2 || !b2 || !ws)
        return pm_fail(PM_EINVAL, "null argument");
    const int Cp = pm_pad32(C);
    if (Cp != 32 && Cp != 64 && Cp != 128 && Cp != 256)
        return pm_fail(PM_EINVAL, "channels %d unsupported", C);
    if ((K != 3 && K != 7 && K != 11) || d < 1 || d > 5)
        return pm_fail(PM_EINVAL, "kernel %d / dilation %d unsupported", K, d);
    if (ws_bytes < pm_op_workspace_bytes(C, C, K))
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const void *p1, *p2;
    const int rc = pack_iteration(dtype, C, K, w1, b1, w2, b2, (char*)ws, s,
                                  &p1, &p2);
    if (rc) return rc;
    PairArgs a = {};
    a.x = x; a.out = out; a.w1 = p1; a.w2 = p2;
    a.B = B; a.L = L; a.dilation = d; a.mode = mode; a.scale = scale;
    a.lengths = lengths; a.len_scale = 1;
    PM_HIP_TRY(launch_pair(dtype, Cp, K, a, s));
    return PM_OK;
}

extern "C" int pm_block_iteration_cl(
    int dtype, const float* x, float* out, const float* w1, const float* b1,
    const float* w2, const float* b2, int B, int L, int C, int K, int d,
    int mode, float scale, void* ws, size_t ws_bytes, void* stream) {
    return block_iteration_cl_impl(dtype, x, out, w1, b1, w2, b2, nullptr, B,
                                   L, C, K, d, mode, scale, ws, ws_bytes,
                                   stream);
}

// pm_block_iteration_cl on a ragged batch, as a forward with `lengths`
// launches the layer: utterance b has lengths[b] rows (device int32, clamped
// to `length`); rows past them are neither read nor written.
extern "C" int pm_block_iteration_ragged_cl(
    int dtype, const float* x, float* out, const float* w1, const float* b1,
    const float* w2, const float* b2, const int* lengths, int B, int L, int C,
    int K, int d, int mode, float scale, void* ws, size_t ws_bytes,
    void* stream) {
    if (!lengths) return pm_fail(PM_EINVAL, "null argument");
    return block_iteration_cl_impl(dtype, x, out, w1, b1, w2, b2, lengths, B,
                                   L, C, K, d, mode, scale, ws, ws_bytes,
                                   stream);
}

// Debug (-DPM_TUNING builds): subsequent pair / whole-Block launches make
// wave 0 of workgroup i write 16 shader-clock stamps to timeline[16 i ..]
// (NULL switches it off). The shipped library has no such instrumentation
// and returns PM_ESTATE.
extern "C" int pm_debug_timeline(void* dev_buffer) {
#ifdef PM_TUNING
    g_timeline = (unsigned long long*)dev_buffer;
    return PM_OK;
#else
    (void)dev_buffer;
    return pm_fail(PM_ESTATE, "pm_debug_timeline needs a -DPM_TUNING build "
                              "(make TUNING=1)");
#endif
}

// What the last pm_block_cl / pm_block_act16_cl / pm_mrf_cl of this host
// thread launched (pm_debug_last_launch below): written after the launch,
// read by nothing that plans or launches.
struct PmLastLaunch { bool valid = false; PmLaunch launch; };
static PmLastLaunch& last_launch() {
    static thread_local PmLastLaunch l;
    return l;
}
static void record_launch(const PmLaunch& l) {
    last_launch().valid = true;
    last_launch().launch = l;
}

static int block_cl_impl(
    int dtype, const float* x, float* out, const float* const* w1,
    const float* const* b1, const float* const* w2, const float* const* b2,
    const int* dilations, int niter, int B, int L, int C, int K, int mode,
    float scale, void* ws, size_t ws_bytes, void* stream, void* act16,
    int act_dtype) {
    if (!x || !out || !w1 || !b1 || !w2 || !b2 || !dilations || !ws)
        return pm_fail(PM_EINVAL, "null argument");
    const int Cp = pm_pad32(C);
    if (Cp > 256)
        return pm_fail(PM_EINVAL, "channels %d unsupported (<= 256)", C);
    if ((K != 3 && K != 7 && K != 11) || niter < 1 || niter > 3)
        return pm_fail(PM_EINVAL,
                       "kernel %d / %d iterations unsupported", K, niter);
    const size_t per = iteration_layout(C, C, K, nullptr).total;
    if (ws_bytes < 3 * per)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    PmStage d = stage_desc(Cp, x, out, B, L, mode, scale, 1, niter);
    d.blk[0].K = K;
    for (int n = 0; n < niter; ++n) {
        const int rc = pack_iteration(dtype, C, K, w1[n], b1[n], w2[n], b2[n],
                                      (char*)ws + n * per, s, &d.blk[0].w1[n],
                                      &d.blk[0].w2[n]);
        if (rc) return rc;
        d.blk[0].dil[n] = dilations[n];
    }
    // (what the caller hands over beyond the packed weights serves the skewed
    // walk: pm_walk_scratch_bytes)
    if (ws_bytes > 3 * per) {
        d.scratch = (char*)ws + 3 * per;
        d.scratch_bytes = ws_bytes - 3 * per;
    }
    if (act16) { d.act16 = act16; d.act16_type = act_dtype; }
    PmPlan plan;
    PM_HIP_TRY(plan_stage(dtype, d, 1, &plan));
    if (plan.block[0].kernel == PM_PAIRS)
        return pm_fail(PM_EINVAL, "no whole-Block kernel for this shape");
    PM_HIP_TRY(launch_block3(dtype, plan.block[0], d, 0, s));
    record_launch(plan.block[0]);
    if (act16 && !plan.block[0].act16)
        return pm_fail(PM_ESTATE,
                       "the launch did not take the skewed walk: `out` "
                       "holds the fp32 result, the 16-bit operand copy was not "
                       "written");
    return PM_OK;
}

extern "C" int pm_block_cl(
    int dtype, const float* x, float* out, const float* const* w1,
    const float* const* b1, const float* const* w2, const float* const* b2,
    const int* dilations, int niter, int B, int L, int C, int K, int mode,
    float scale, void* ws, size_t ws_bytes, void* stream) {
    return block_cl_impl(dtype, x, out, w1, b1, w2, b2, dilations, niter, B, L,
                         C, K, mode, scale, ws, ws_bytes, stream, nullptr, 0);
}

// pm_block_cl whose result leaves as the NEXT upsampler's MFMA operand instead
// of fp32 (Block3Args::act16): act16 (B, L, c_pad) 16-bit = cvt(lrelu(result)),
// act_dtype PM_F16 or PM_BF16; `out` is read (mode 2) and not written. Only the
// skewed walk does this: PM_ESTATE (and the plain fp32 result in `out`) when the
// launcher took another kernel.
extern "C" int pm_block_act16_cl(
    int dtype, int act_dtype, const float* x, float* out, void* act16,
    const float* const* w1, const float* const* b1, const float* const* w2,
    const float* const* b2, const int* dilations, int niter, int B, int L,
    int C, int K, int mode, float scale, void* ws, size_t ws_bytes,
    void* stream) {
    if (!act16) return pm_fail(PM_EINVAL, "null argument");
    if (act_dtype != PM_F16 && act_dtype != PM_BF16)
        return pm_fail(PM_EINVAL, "act_dtype must be PM_F16 or PM_BF16");
    return block_cl_impl(dtype, x, out, w1, b1, w2, b2, dilations, niter, B, L,
                         C, K, mode, scale, ws, ws_bytes, stream, act16,
                         act_dtype);
}

// Whole MRF ResidualBlock (hifigan.py:141-145): out = (B_3(x) + B_7(x) +
// B_11(x)) / 3, the three Blocks k = 3, 7, 11 (niter dilations each) in ONE
// launch with their sum held in registers. Only where the whole-MRF kernel
// exists (32 channels); w1 / b1 / w2 / b2 are HOST arrays of 3 * niter device
// pointers, Block-major. workspace >= 3 * niter * pm_op_workspace_bytes(c, c, 11).
extern "C" int pm_mrf_cl(
    int dtype, const float* x, float* out, const float* const* w1,
    const float* const* b1, const float* const* w2, const float* const* b2,
    const int* dilations, int niter, int B, int L, int C, void* ws,
    size_t ws_bytes, void* stream) {
    if (!x || !out || !w1 || !b1 || !w2 || !b2 || !dilations || !ws)
        return pm_fail(PM_EINVAL, "null argument");
    const int Cp = pm_pad32(C);
    if (Cp != 32)
        return pm_fail(PM_EINVAL, "whole-MRF kernel exists for <= 32 channels");
    if (niter < 1 || niter > 3) return pm_fail(PM_EINVAL, "1..3 dilations");
    const size_t per = iteration_layout(C, C, 11, nullptr).total;
    if (ws_bytes < 3 * (size_t)niter * per)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    PmStage d = stage_desc(Cp, x, out, B, L, 1, 1.f / 3.f, 3, niter);
    for (int j = 0; j < 3; ++j) {
        d.blk[j].K = 4 * j + 3;         // 3, 7, 11
        for (int n = 0; n < niter; ++n) {
            const int i = j * niter + n;
            const int rc = pack_iteration(
                dtype, C, d.blk[j].K, w1[i], b1[i], w2[i], b2[i],
                (char*)ws + (size_t)i * per, s, &d.blk[j].w1[n], &d.blk[j].w2[n]);
            if (rc) return rc;
            d.blk[j].dil[n] = dilations[n];
        }
    }
    // (what the caller hands over beyond the packed weights serves the skewed
    // whole-MRF walk of the 4-byte operand layouts: pm_walk_scratch_bytes)
    if (ws_bytes > 3 * (size_t)niter * per) {
        d.scratch = (char*)ws + 3 * (size_t)niter * per;
        d.scratch_bytes = ws_bytes - 3 * (size_t)niter * per;
    }
    PmLaunch l;
    bool planned = false;
    PM_HIP_TRY(with_elem(dtype, [&](auto et) {
           planned = pm_plan_mrf<decltype(et)>(d, false, &l);
           return hipSuccess;
    }));
    if (!planned)
        return pm_fail(PM_EINVAL, "no whole-MRF kernel for this shape");
    PM_HIP_TRY(launch_mrf(dtype, l, d, s));
    record_launch(l);
    return PM_OK;
}

// Input layers (hifigan.py:19-30, 67-68): Conv1d(c_in -> c_out, k 7, pad 3) on
// channels-last features plus the speaker conditioning Conv1d(G -> c_out, k 1)
// of the (B|1, G) global features, added as a per-utterance bias.
//   x_cl (B, L, pad32(c_in)), w (c_out, c_in, 7), bias (c_out),
//   global (gbatch, G), ws_w (c_out, G), ws_b (c_out)  ->  (B, L, pad32(c_out))
// The weights and the bias lie where a Block iteration (c_in, c_out, 7) has
// its first stream and its first bias; the speaker bias (B, pad32(c_out))
// follows that whole iteration, the public pm_op_workspace_bytes
struct InputConvLayout { float *w, *bias, *gbias; size_t total; };
static InputConvLayout input_conv_layout(int c_in, int c_out, int B,
                                         void* base) {
    const IterationLayout it = iteration_layout(c_in, c_out, 7, base);
    PmCarve c(base ? (char*)base + it.total : nullptr);
    return {it.w1, it.b1, c.take<float>((size_t)B * pm_pad32(c_out)),
            it.total + c.used};
}

extern "C" int pm_input_conv_cl(
    int dtype, const float* x, float* out, const float* w, const float* bias,
    const float* global, const float* ws_w, const float* ws_b, int gbatch,
    int G, int B, int L, int c_in, int c_out, void* ws, size_t ws_bytes,
    void* stream) {
    if (!x || !out || !w || !bias || !global || !ws_w || !ws_b || !ws)
        return pm_fail(PM_EINVAL, "null argument");
    if (gbatch != 1 && gbatch != B)
        return pm_fail(PM_EINVAL, "global batch must be 1 or batch");
    const int cop = pm_pad32(c_out);
    if (cop % 64 && cop != 32)
        return pm_fail(PM_EINVAL, "output channels %d unsupported", c_out);
    const InputConvLayout l = input_conv_layout(c_in, c_out, B, ws);
    if (ws_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Layer conv = input_layer(dtype, c_in, c_out);
    conv.w = l.w; conv.bias = l.bias;
    PM_HIP_TRY(pack_layer(conv, w, bias, s));
    PM_HIP_TRY(launch_speaker_bias(global, ws_w, ws_b, l.gbias, gbatch, G,
                                   c_out, s));
    PM_HIP_TRY(launch_input_conv(conv, x, out, l.gbias, gbatch, B, L, nullptr,
                                 s));
    return PM_OK;
}

// Packed weights in two fp32-sized streams' room (no bias steps: less than a
// Block iteration's), then the bias, once per phase
struct TransposeLayout { float *w, *bias; size_t total; };
static TransposeLayout transpose_layout(int c_in, int c_out, int r,
                                        void* base) {
    const size_t ci = pm_pad32(c_in), co = pm_pad32(c_out);
    PmCarve c(base);
    float* w = c.take<float>(ci * co * 2 * r);
    c.take<float>(ci * co * 2 * r);
    return {w, c.take<float>(co * r), c.used};
}

static int conv_transpose_cl_impl(
    int dtype, const float* x, const void* x16, float* out, const float* w,
    const float* bias, int B, int L, const int* lengths, int c_in, int c_out,
    int r, int lrelu, void* ws, size_t ws_bytes, void* stream) {
    if ((!x && !x16) || !out || !w || !bias || !ws)
        return pm_fail(PM_EINVAL, "null argument");
    if (r < 2 || (r & 1)) return pm_fail(PM_EINVAL, "rate %d unsupported", r);
    if (ws_bytes < pm_op_workspace_bytes(c_in, c_out, 2 * r))
        return pm_fail(PM_ENOMEM, "workspace too small");
    const TransposeLayout l = transpose_layout(c_in, c_out, r, ws);
    if (l.total > pm_op_workspace_bytes(c_in, c_out, 2 * r))
        return pm_fail(PM_ESTATE, "the layout outgrew its public bound");
    hipStream_t s = (hipStream_t)stream;
    Layer up = upsample_layer(dtype, c_in, c_out, r);
    if (x16 && !takes_x16(up))
        return pm_fail(PM_EINVAL, "a 16-bit operand input needs a 16-bit "
                       "operand type and the narrow upsampler kernel");
    up.w = l.w; up.bias = l.bias;
    PM_HIP_TRY(pack_layer(up, w, bias, s));
    PM_HIP_TRY(launch_upsample(up, x, x16, out, lrelu, B, L, lengths, 1, s));
    return PM_OK;
}

extern "C" int pm_conv_transpose_cl(
    int dtype, const float* x, float* out, const float* w, const float* bias,
    int B, int L, int c_in, int c_out, int r, int lrelu, void* ws,
    size_t ws_bytes, void* stream) {
    if (!x) return pm_fail(PM_EINVAL, "null argument");
    return conv_transpose_cl_impl(dtype, x, nullptr, out, w, bias, B, L,
                                  nullptr, c_in, c_out, r, lrelu, ws, ws_bytes,
                                  stream);
}

// pm_conv_transpose_cl on a ragged batch, as a forward with `lengths` launches
// the layer: utterance b has lengths[b] input rows (device int32, clamped to
// `length`); its output rows past r * lengths[b] are not written.
extern "C" int pm_conv_transpose_ragged_cl(
    int dtype, const float* x, float* out, const float* w, const float* bias,
    const int* lengths, int B, int L, int c_in, int c_out, int r, int lrelu,
    void* ws, size_t ws_bytes, void* stream) {
    if (!x || !lengths) return pm_fail(PM_EINVAL, "null argument");
    return conv_transpose_cl_impl(dtype, x, nullptr, out, w, bias, B, L,
                                  lengths, c_in, c_out, r, lrelu, ws, ws_bytes,
                                  stream);
}

// pm_conv_transpose_cl on an input that already holds the operand values:
// x16_cl (B, L, c_in_pad) in the operand type `dtype` = cvt(lrelu(x)), as
// pm_block_act16_cl writes it - staged as it is (SingleArgs::x16).
extern "C" int pm_conv_transpose_x16_cl(
    int dtype, const void* x16, float* out, const float* w, const float* bias,
    int B, int L, int c_in, int c_out, int r, void* ws, size_t ws_bytes,
    void* stream) {
    if (!x16) return pm_fail(PM_EINVAL, "null argument");
    return conv_transpose_cl_impl(dtype, nullptr, x16, out, w, bias, B, L,
                                  nullptr, c_in, c_out, r, 1, ws, ws_bytes,
                                  stream);
}

extern "C" int pm_out_conv_tanh(
    const float* x, const float* w, float* out, int B, int L, int C,
    void* stream) {
    if (!x || !w || !out) return pm_fail(PM_EINVAL, "null argument");
    if (pm_pad32(C) > 64)
        return pm_fail(PM_EINVAL, "channels %d unsupported", C);
    PM_HIP_TRY(launch_out_conv(x, w, out, B, L, C, nullptr, 1,
                               (hipStream_t)stream));
    return PM_OK;
}

// Test hook: force the walked whole-Block / whole-MRF kernels (with
// `walk_nseg` segments per utterance) and the number of M groups of the wide
// upsampler, which the launchers otherwise pick from the grid size - so that
// unit-sized inputs reach those code paths. 0 restores the heuristics.
//
// The hooks are OFF unless the process was started with PROMONET_HIP_DEBUG=1
// (tests/conftest.py and the scripts under scripts/ set it): a production
// process cannot have its launch geometry changed under it. Their state is
// per host thread (pm_launch.h), so a test thread's override never reaches a
// forward running on another thread, and every API call reads it on the
// thread that launches.
static bool debug_hooks_enabled() {
    static const bool enabled = [] {
        const char* e = getenv("PROMONET_HIP_DEBUG");
        return e && e[0] == '1';
    }();
    return enabled;
}

extern "C" int pm_debug_force(int walk_nseg, int upsample_groups) {
    if (!debug_hooks_enabled())
        return pm_fail(PM_ESTATE, "debug hooks are disabled "
                       "(start the process with PROMONET_HIP_DEBUG=1)");
    if (walk_nseg < 0 || upsample_groups < 0)
        return pm_fail(PM_EINVAL, "negative value");
    pm_force().walk_nseg = walk_nseg;
    pm_force().upsample_groups = upsample_groups;
    return PM_OK;
}

// Sustained-rate probe of the matrix pipe (bench.py times it with HIP events
// on `stream`): `workgroups` x 4 waves x `iterations` x 16 MFMAs of 32 768 FLOP.
// operands: >= 32 768 bytes of finite values of the operand type (2 048 uint4
// are read). A measurement aid, not a test hook: always available, it changes
// no state of the library.
extern "C" int pm_mfma_probe(int dtype, int iterations, const void* operands,
                             float* sink, int workgroups, void* stream) {
    if (!operands || !sink) return pm_fail(PM_EINVAL, "null argument");
    if (iterations < 1 || workgroups < 1)
        return pm_fail(PM_EINVAL, "bad probe arguments");
    hipStream_t s = (hipStream_t)stream;
    const uint4* src = (const uint4*)operands;
    if (dtype == PM_F16)
        hipLaunchKernelGGL(pm_mfma_probe_kernel<1>, dim3(workgroups), dim3(256),
                           0, s, src, sink, iterations);
    else if (dtype == PM_BF16)
        hipLaunchKernelGGL(pm_mfma_probe_kernel<2>, dim3(workgroups), dim3(256),
                           0, s, src, sink, iterations);
    else
        return pm_fail(PM_EINVAL,
                       "probe operand type must be PM_F16 or PM_BF16");
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// Test hook: -1 keeps the launchers off the skewed whole-Block walk, 1 takes
// it wherever it fits, 0 restores the default (the shapes it measured faster
// on, when scratch was handed over).
extern "C" int pm_debug_skew(int mode) {
    if (!debug_hooks_enabled())
        return pm_fail(PM_ESTATE, "debug hooks are disabled "
                       "(start the process with PROMONET_HIP_DEBUG=1)");
    if (mode < -1 || mode > 1) return pm_fail(PM_EINVAL, "mode is -1, 0 or 1");
    pm_force().skew = mode;
    return PM_OK;
}

// Test hook: the PmLaunch the last pm_block_cl / pm_block_act16_cl / pm_mrf_cl
// of this host thread took - kernel (the PmKernel values: 1 skewed, 2 walked,
// 3 two-sided tiling), segments per utterance (0: no walk), the latency
// geometry, the 16-bit operand output. PM_ESTATE before any such launch.
// Reads what the launch recorded; changes nothing that is launched.
extern "C" int pm_debug_last_launch(int* kernel, int* nseg, int* narrow,
                                    int* act16) {
    if (!debug_hooks_enabled())
        return pm_fail(PM_ESTATE, "debug hooks are disabled "
                       "(start the process with PROMONET_HIP_DEBUG=1)");
    if (!kernel || !nseg || !narrow || !act16)
        return pm_fail(PM_EINVAL, "null argument");
    const PmLastLaunch& l = last_launch();
    if (!l.valid)
        return pm_fail(PM_ESTATE, "no whole-Block or whole-MRF launch on "
                       "this thread yet");
    *kernel = (int)l.launch.kernel;
    *nseg = l.launch.nseg;
    *narrow = l.launch.narrow;
    *act16 = l.launch.act16;
    return PM_OK;
}

// Scratch bytes the skewed whole-Block walk wants behind the workspace of
// pm_block_cl for a batch of B utterances (optional: without it the walked
// or stand-alone kernels run).
extern "C" size_t pm_walk_scratch_bytes(int B) {
    return B < 1 ? 0 : walk_scratch_bytes(B);
}

extern "C" int pm_fold_weight_norm(
    const float* g, const float* v, float* w, int rows, int cols,
    void* stream) {
    if (!g || !v || !w || rows < 1 || cols < 1)
        return pm_fail(PM_EINVAL, "bad argument");
    hipLaunchKernelGGL(pm_fold_kernel, dim3(rows), dim3(256), 0,
                       (hipStream_t)stream, g, v, w, cols);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_to_channels_last(
    const float* src, float* dst, int B, int C, int T, int c_pad,
    void* stream) {
    if (!src || !dst || c_pad % 32) return pm_fail(PM_EINVAL, "bad argument");
    dim3 grid((T + 31) / 32, c_pad / 32, B);
    hipLaunchKernelGGL(pm_to_channels_last_kernel, grid, dim3(256), 0,
                       (hipStream_t)stream, src, dst, C, T, c_pad);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}


// promonet.edit feature editing (edit/core.py:17-132, edit/grid.py:12-45)
extern "C" int pm_grid_sample(
    const float* seq, const float* grid, float* out, int rows, int n_in,
    int n_out, int mode, float scale, float offset, float lo, float hi,
    void* stream) {
    if (!seq || !out) return pm_fail(PM_EINVAL, "null argument");
    if (rows < 1 || n_in < 1 || n_out < 1 || mode < 0 || mode > 2)
        return pm_fail(PM_EINVAL, "bad grid-sample arguments");
    if (rows > 65535) return pm_fail(PM_EINVAL, "too many rows (max 65535)");
    hipLaunchKernelGGL(pm_grid_sample_kernel, dim3((n_out + 255) / 256, rows),
                       dim3(256), 0, (hipStream_t)stream, seq, grid, out, rows,
                       n_in, n_out, mode, scale, offset, lo, hi);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// Selective time-stretch grid (edit/core.py:57-110)
extern "C" int pm_stretch_grid(
    const float* ppg, int ppg_rows, const int* indices, int n_indices,
    float* selected, float* grid, int frames, int target_frames,
    void* stream) {
    if (!ppg || !indices || !selected || !grid)
        return pm_fail(PM_EINVAL, "null argument");
    if (ppg_rows < 1 || n_indices < 1 || frames < 1 || target_frames < 1)
        return pm_fail(PM_EINVAL, "bad stretch-grid arguments");
    StretchArgs a;
    a.ppg = ppg; a.indices = indices; a.selected = selected; a.grid = grid;
    a.n = n_indices; a.T = frames; a.target = target_frames; a.P = ppg_rows;
    const size_t bytes = (size_t)frames * sizeof(float);
    const size_t smem = bytes <= 64 * 1024 ? bytes : 0;
    auto kern = pm_stretch_grid_kernel;
    if (smem > 48 * 1024)
        PM_HIP_TRY(pm_ensure_dynamic_lds(reinterpret_cast<const void*>(kern),
                                         (int)smem));
    hipLaunchKernelGGL(kern, dim3(1), dim3(256), smem, (hipStream_t)stream, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

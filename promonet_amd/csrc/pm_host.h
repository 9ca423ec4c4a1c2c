// Host helpers shared by every .hip that implements part of the C ABI
// (include/promonet_hip.h). No kernels: what is declared here and not inline
// is defined once, in pm_api.hip, next to the state or the kernels it needs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "promonet_hip.h"

// Sets the message pm_last_error() returns on this thread; returns `code`
int pm_fail(int code, const char* fmt, ...)
    __attribute__((format(printf, 2, 3)));

#define PM_HIP_TRY(expr)                                                     \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess)                                                \
            return pm_fail(PM_EHIP, "%s failed: %s (%s:%d)", #expr,          \
                           hipGetErrorString(e_), __FILE__, __LINE__);       \
    } while (0)

// the most workgroups one grid dimension takes
static const long long PM_MAX_GRID = 0x7fffffffll;

static inline int pm_pad32(int c) { return (c + 31) / 32 * 32; }
static inline size_t pm_align256(size_t v) { return (v + 255) / 256 * 256; }
static inline bool pm_aligned16(const void* p) {
    return ((uintptr_t)p & 15) == 0;
}

static inline long long pm_ceil_div(long long a, long long b) {
    return (a + b - 1) / b;
}
// the workgroups of `block` threads that hold `threads`
static inline unsigned pm_groups(long long threads, int block) {
    return (unsigned)pm_ceil_div(threads, block);
}

// Returns NULL, or what is wrong with the slope of a leaky layer.
static inline const char* pm_check_slope(float slope) {
    // (on the bits, as one integer range: the files that call this are
    // compiled with -fno-honor-nans, which lets the compiler drop any test
    // that only NaN fails; the positive floats are ordered as their bits are,
    // 1.f being 0x3f800000)
    uint32_t bits;
    std::memcpy(&bits, &slope, sizeof bits);
    if (bits - 1u > 0x3f800000u - 1u)
        return "slope must be finite and in (0, 1]";
    return nullptr;
}

// The partials of a gW kernel over `pixels` flattened pixels, one a workgroup,
// and the pixels of each, a multiple of 16 (so that its four waves take whole
// steps of four): ceil(pixels / chunk) of them, `max_parts` at the most. A
// function of the sizes alone.
struct PmSplit { int parts, each; };
static inline PmSplit pm_pixel_split(long long pixels, int chunk,
                                     int max_parts) {
    long long want = pm_ceil_div(pixels, chunk);
    if (want > max_parts) want = max_parts;
    const int each = (int)((pm_ceil_div(pixels, want) + 15) / 16 * 16);
    return {(int)pm_ceil_div(pixels, each), each};
}

// The partials a tile of the gW kernels that are GEMMs over flattened pixels
// (pc_gw_kernel, gc_gw_kernel, fs_gw_kernel), and the K
// chunks of each: K = `pixels` runs in chunks of `pixels_per_chunk`, and a
// tile's chunks go to at most `workgroups` / `tiles` partials (one at the
// least) of `min_chunks` chunks or more (but the last). A function of the
// sizes alone.
struct PmChunkSplit { int parts, each, chunks; };
static inline PmChunkSplit pm_chunk_split(long long pixels,
                                          int pixels_per_chunk, int tiles,
                                          int workgroups, int min_chunks) {
    const int chunks = (int)pm_ceil_div(pixels, pixels_per_chunk);
    long long want = pm_ceil_div(chunks, min_chunks);
    const long long room = workgroups / tiles > 1 ? workgroups / tiles : 1;
    if (want > room) want = room;
    const int each = (int)pm_ceil_div(chunks, want);
    return {(int)pm_ceil_div(chunks, each), each, chunks};
}

// The checks of a conv layer's backward after its sizes: the pointers, then
// the workspace of `needed` bytes, which only the weight gradients use.
// `inputs`: no tensor that the entry reads is null.
static inline int pm_check_backward(const char* entry, bool inputs,
                                    const float* grad_weight,
                                    const float* grad_bias,
                                    const void* workspace,
                                    size_t workspace_bytes, size_t needed) {
    const bool weights = grad_weight || grad_bias;
    if (!inputs || (weights && (!grad_weight || !grad_bias || !workspace)))
        return pm_fail(PM_EINVAL, "%s: null argument", entry);
    if (weights && workspace_bytes < needed)
        return pm_fail(PM_ENOMEM, "%s: workspace too small", entry);
    return PM_OK;
}

// A caller-provided workspace is laid out by one function that carves its
// slots in order: on a null base the carve only counts (the *_bytes entries
// read `used`), on the caller's pointer it places (the launches). A layout
// returned as a braced list takes its slots in member order (the elements of
// a braced list are evaluated left to right), `used` last.
struct PmCarve {
    char* base; size_t used = 0;
    explicit PmCarve(void* b) : base((char*)b) {}
    // a 256-byte slot of `count` T; null when base is null
    template <class T> T* take(size_t count) {
        T* p = base ? (T*)(base + used) : nullptr;
        used += pm_align256(count * sizeof(T));
        return p;
    }
};

// The workspace of a conv layer's backward: the `parts` partials of gW | gb,
// `partial_floats` each
struct PmPartsLayout { float* parts; size_t total; };
static inline PmPartsLayout pm_parts_layout(void* base, size_t parts,
                                            size_t partial_floats) {
    PmCarve c(base);
    return {c.take<float>(parts * partial_floats), c.used};
}

// Do the byte ranges [a, a + an) and [b, b + bn) share a byte? A null or an
// empty range overlaps nothing.
static inline bool pm_overlap(
    const void* a, size_t an, const void* b, size_t bn) {
    const char* p = (const char*)a;
    const char* q = (const char*)b;
    return p && q && an && bn && p < q + bn && q < p + an;
}

// Opt a kernel into `bytes` of dynamic LDS (> 48 KB needs the attribute).
// The grant is a property of (kernel, DEVICE): cached per pair, so one process
// driving several GPUs sets it on each, and guarded so that concurrent
// launches from several host threads / streams are safe.
hipError_t pm_ensure_dynamic_lds(const void* kern, int bytes);

// Launch `kern` on `grid` workgroups of `threads` with `lds` bytes of dynamic
// LDS, granted first
template <class Kernel, class Args>
int pm_launch_dynamic(Kernel kern, unsigned grid, int threads, int lds,
                      hipStream_t s, const Args& a) {
    PM_HIP_TRY(pm_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, a);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// Compute units of the current device, queried once per device (the walked
// launches size their grids from it on every forward).
int pm_device_cus();

// *dst (allocated when null) = n floats of device memory copied from src
int pm_copy_dev(float** dst, const float* src, size_t n, hipStream_t s);

// The exact-fp32 convs of the framed DFT (pm_audio.hip), whose kernels are
// compiled with the other convs: pack a (cout, cin, k) basis, plain conv
// layout of 64-channel chunks, and run it over x (B, L, Cin) with epilogue
// `epi` (pm_launch_stft). bins / maxbits / grad: SingleArgs (pm_conv.h).
struct PmDftConv {
    const float* x; float* out; const void* w; const float* bias;
    int B, L, Lout, Cin, M, pad, bins;
    unsigned* maxbits; const float* grad;
};
hipError_t pm_dft_pack(const float* w, void* out, int cout, int cout_pad,
                       int cin, int k, hipStream_t s);
hipError_t pm_dft_conv(int epi, const PmDftConv& c, hipStream_t s);

// The adjoint of the short-time transform of a plan (pm_stockham.h), whose
// kernels are compiled with the losses (pm_loss.hip): G (B, bins, frames, 2)
// to the windowed frames (B, frames, N) in `frames`, then their overlap-add
// and the adjoint of the reflect margin; grad_x (B, T) = (or +=, `accumulate`)
// scale[0] * that, a null scale being 1.
struct ScPlan;
hipError_t pm_sc_adjoint_launch(const ScPlan& p, int batch, const float* G,
                                const float* window, const float* twiddle,
                                const float* scale, float* grad_x,
                                int accumulate, float* frames, hipStream_t s);

// The HiFi-GAN engine as the streaming entries see it (pm_stream.hip): its
// configuration, and pm_hifigan_forward_cl with the stream typed.
const pm_hifigan_config* pm_hifigan_config_of(pm_hifigan_t h);
int pm_hifigan_forward_window(pm_hifigan_t h, const float* features_cl,
                              const float* g, int gbatch, float* out, int B,
                              int T, void* ws, size_t ws_bytes, hipStream_t s);

#ifdef PM_TUNING
unsigned long long* pm_timeline();   // what pm_debug_timeline set, or null
#endif

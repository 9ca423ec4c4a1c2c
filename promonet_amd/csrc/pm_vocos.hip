// Vocos engine and unit entries of the C ABI (include/promonet_hip.h).
// Kernels: pm_vocos.h. Reference: promonet/model/vocos.py.
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "pm_host.h"
#include "pm_vocos.h"

namespace {

int round_up(int v, int m) { return (v + m - 1) / m * m; }

bool known_dtype(int dtype) {
    return dtype == PM_F32 || dtype == PM_F16 || dtype == PM_BF16;
}
size_t esz(int dtype) { return dtype == PM_F32 ? 4 : 2; }

template <class F> hipError_t with_elem(int dtype, F&& f) {
    switch (dtype) {
        case PM_F16: return f(ElemF16());
        case PM_BF16: return f(ElemBF16());
        default: return f(ElemF32());
    }
}

// fp32 (N, K, taps) -> operand type [round_up(N, 128)][taps][K]
hipError_t pack(int dtype, const float* w, void* out, int N, int K, int taps,
                hipStream_t s) {
    const int Np = round_up(N, PM_VOCOS_GEMM_COLS);
    const long long total = (long long)Np * taps * K;
    return with_elem(dtype, [&](auto et) {
        typedef decltype(et) ET;
        hipLaunchKernelGGL(vocos_pack_kernel<ET>,
                           dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           s, w, out, N, Np, K, taps);
        return hipGetLastError();
    });
}
size_t packed_bytes(int dtype, int N, int K, int taps) {
    return pm_align256((size_t)round_up(N, PM_VOCOS_GEMM_COLS) * taps * K *
                       esz(dtype));
}

hipError_t gemm(int dtype, int taps, bool cf, const VocosGemmArgs& a,
                hipStream_t s) {
    const dim3 grid((a.B * a.T + PM_VOCOS_GEMM_ROWS - 1) / PM_VOCOS_GEMM_ROWS,
                    round_up(a.N, PM_VOCOS_GEMM_COLS) / PM_VOCOS_GEMM_COLS);
    return with_elem(dtype, [&](auto et) {
        typedef decltype(et) ET;
        auto launch = [&](auto ragged) {
            constexpr bool RG = decltype(ragged)::value;
            if (taps == 7 && cf)
                hipLaunchKernelGGL((vocos_gemm_kernel<ET, 7, true, RG>), grid,
                                   dim3(256), 0, s, a);
            else if (taps == 7)
                hipLaunchKernelGGL((vocos_gemm_kernel<ET, 7, false, RG>), grid,
                                   dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL((vocos_gemm_kernel<ET, 1, false, RG>), grid,
                                   dim3(256), 0, s, a);
        };
        if (a.rg.map) launch(std::true_type());
        else launch(std::false_type());
        return hipGetLastError();
    });
}

// rows: B T; total: the packed row count on the device (ragged) or null
hipError_t layer_norm(float* x, const float* g, const float* b, int rows,
                      const int* total, hipStream_t s) {
    if (total)
        hipLaunchKernelGGL(vocos_ln_kernel<true>, dim3((rows + 3) / 4),
                           dim3(256), 0, s, x, g, b, rows, total);
    else
        hipLaunchKernelGGL(vocos_ln_kernel<false>, dim3((rows + 3) / 4),
                           dim3(256), 0, s, x, g, b, rows, total);
    return hipGetLastError();
}

hipError_t block(int dtype, const VocosBlockArgs& a, hipStream_t s) {
    return with_elem(dtype, [&](auto et) {
        typedef decltype(et) ET;
        typedef VocosTile<ET> Tile;
        auto kern = a.rg.map ? vocos_block_kernel<ET, true>
                             : vocos_block_kernel<ET, false>;
        hipError_t e = pm_ensure_dynamic_lds(
            reinterpret_cast<const void*>(kern), Tile::SMEM);
        if (e != hipSuccess) return e;
        const int rows = a.B * a.T;
        hipLaunchKernelGGL(kern, dim3((rows + Tile::MT - 1) / Tile::MT),
                           dim3(Tile::THREADS), Tile::SMEM, s, a);
        return hipGetLastError();
    });
}

// frames (B T, 1024) -> audio (B, 256 T); off: the ragged batch's (B + 1)
// first rows (mode 0 only) or null
hipError_t istft(int mode, const float* spec, const float* window,
                 float* frames, float* audio, int B, int T, const int* off,
                 hipStream_t s) {
    VocosIstftArgs a = {spec, window, frames, B, T, off ? off + B : nullptr};
    if (mode == 0 && off)
        hipLaunchKernelGGL((vocos_istft_frame_kernel<0, true>), dim3(B * T),
                           dim3(256), 0, s, a);
    else if (mode == 0)
        hipLaunchKernelGGL((vocos_istft_frame_kernel<0, false>), dim3(B * T),
                           dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((vocos_istft_frame_kernel<1, false>), dim3(B * T),
                           dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((T * PM_VOCOS_HOP + 255) / 256, B);
    if (off)
        hipLaunchKernelGGL(vocos_ola_kernel<true>, grid, dim3(256), 0, s,
                           frames, window, audio, T, off);
    else
        hipLaunchKernelGGL(vocos_ola_kernel<false>, grid, dim3(256), 0, s,
                           frames, window, audio, T, off);
    return hipGetLastError();
}

// the head's logits (B T, 1026) -> audio; frames aliases nothing it reads
hipError_t head(int dtype, const float* x, const void* w, const float* bias,
                const float* window, float* logits, float* frames,
                float* audio, int B, int T, const VocosRagged& rg,
                hipStream_t s) {
    VocosGemmArgs g = {};
    g.x = x; g.w = w; g.bias = bias; g.out = logits;
    g.B = B; g.T = T; g.K = PM_VOCOS_C; g.N = PM_VOCOS_HEAD_OUT;
    g.ldo = PM_VOCOS_HEAD_OUT; g.rg = rg;
    hipError_t e = gemm(dtype, 1, false, g, s);
    if (e != hipSuccess) return e;
    return istft(0, logits, window, frames, audio, B, T, rg.off, s);
}

// one ConvNeXt block's operand-type pointwise weights and depthwise taps
struct BlockWeights { char* w1; char* w2; float* dw; size_t total; };
BlockWeights block_weights(int dtype, int C, int H, void* base) {
    PmCarve c(base);
    return {c.take<char>((size_t)C * H * esz(dtype)),
            c.take<char>((size_t)C * H * esz(dtype)),
            c.take<float>((size_t)7 * C), c.used};
}

// pm_vocos_head: packed weight | logits (rows x 1026) | frames (rows x 1024)
struct HeadLayout { char* w; float* logits; float* frames; size_t total; };
HeadLayout head_layout(int dtype, int batch, int frames, void* base) {
    const size_t rows = (size_t)batch * frames;
    PmCarve c(base);
    return {c.take<char>(packed_bytes(dtype, PM_VOCOS_HEAD_OUT, PM_VOCOS_C, 1)),
            c.take<float>(rows * PM_VOCOS_HEAD_OUT),
            c.take<float>(rows * PM_VOCOS_NFFT), c.used};
}

}  // namespace

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
struct pm_vocos_s {
    int F, G, C, H, layers, dtype;
    struct Tensor {
        std::vector<int64_t> shape;
        float* data = nullptr;
    };
    std::map<std::string, Tensor> tensors;  // every state_dict entry, fp32
    void* packed = nullptr;                 // operand-type weights
    const void* conv_pre = nullptr;
    const void* embed = nullptr;
    const void* head = nullptr;
    std::vector<const void*> w1, w2;
    std::vector<const float*> dw;
    bool finalized = false;

    const float* at(const std::string& name) const {
        return tensors.at(name).data;
    }
};

static std::string layer_key(int i, const char* leaf) {
    return "backbone.convnext." + std::to_string(i) + "." + leaf;
}

extern "C" int pm_vocos_create(int num_features, int global_channels,
                               int channels, int hidden, int layers,
                               int n_fft, int hop, int dtype,
                               pm_vocos_t* out) {
    if (!out) return pm_fail(PM_EINVAL, "null argument");
    *out = nullptr;
    if (num_features < 16 || num_features % 16)
        return pm_fail(PM_EINVAL,
                       "features must be a positive multiple of 16, got %d",
                       num_features);
    if (global_channels < 1)
        return pm_fail(PM_EINVAL, "global channels must be positive, got %d",
                       global_channels);
    if (channels != PM_VOCOS_C)
        return pm_fail(PM_EINVAL,
                       "the kernels are built for %d channels, got %d",
                       PM_VOCOS_C, channels);
    if (hidden < PM_VOCOS_HC || hidden % PM_VOCOS_HC)
        return pm_fail(PM_EINVAL,
                       "pointwise channels must be a positive multiple of %d, "
                       "got %d", PM_VOCOS_HC, hidden);
    if (layers < 0 || layers > 64)
        return pm_fail(PM_EINVAL, "layers must be in [0, 64], got %d", layers);
    if (n_fft != PM_VOCOS_NFFT || hop != PM_VOCOS_HOP)
        return pm_fail(PM_EINVAL, "the iSTFT is built for n_fft %d, hop %d",
                       PM_VOCOS_NFFT, PM_VOCOS_HOP);
    if (!known_dtype(dtype))
        return pm_fail(PM_EINVAL, "dtype must be PM_F32, PM_F16 or PM_BF16");
    auto* h = new pm_vocos_s();
    h->F = num_features; h->G = global_channels; h->C = channels;
    h->H = hidden; h->layers = layers; h->dtype = dtype;
    const int64_t C = channels, H = hidden;
    auto add = [&](const std::string& name, std::vector<int64_t> shape) {
        h->tensors[name].shape = shape;
    };
    add("conv_pre.weight", {C, num_features, 7});
    add("conv_pre.bias", {C});
    add("cond.weight", {C, global_channels, 1});
    add("cond.bias", {C});
    add("backbone.embed.weight", {C, C, 7});
    add("backbone.embed.bias", {C});
    for (const char* n : {"backbone.norm.", "backbone.final_layer_norm."}) {
        add(std::string(n) + "weight", {C});
        add(std::string(n) + "bias", {C});
    }
    for (int i = 0; i < layers; ++i) {
        add(layer_key(i, "dwconv.weight"), {C, 1, 7});
        add(layer_key(i, "dwconv.bias"), {C});
        add(layer_key(i, "norm.weight"), {C});
        add(layer_key(i, "norm.bias"), {C});
        add(layer_key(i, "pwconv1.weight"), {H, C});
        add(layer_key(i, "pwconv1.bias"), {H});
        add(layer_key(i, "pwconv2.weight"), {C, H});
        add(layer_key(i, "pwconv2.bias"), {C});
        add(layer_key(i, "gamma"), {C});
    }
    add("head.out.weight", {n_fft + 2, C});
    add("head.out.bias", {n_fft + 2});
    add("head.istft.window", {n_fft});
    *out = h;
    return PM_OK;
}

extern "C" int pm_vocos_destroy(pm_vocos_t h) {
    if (!h) return PM_OK;
    for (auto& kv : h->tensors)
        if (kv.second.data) hipFree(kv.second.data);
    if (h->packed) hipFree(h->packed);
    delete h;
    return PM_OK;
}

extern "C" int pm_vocos_load_tensor(pm_vocos_t h, const char* name,
                                    const float* dev, const int64_t* shape,
                                    int ndim, void* stream) {
    if (!h || !name || !dev || !shape)
        return pm_fail(PM_EINVAL, "null argument");
    auto it = h->tensors.find(name);
    if (it == h->tensors.end())
        return pm_fail(PM_EINVAL, "unexpected tensor %s", name);
    auto& t = it->second;
    bool same = (size_t)ndim == t.shape.size();
    size_t numel = 1;
    for (size_t d = 0; d < t.shape.size(); ++d) {
        numel *= t.shape[d];
        if (same && shape[d] != t.shape[d]) same = false;
    }
    if (!same) return pm_fail(PM_EINVAL, "%s: unexpected shape", name);
    if (!t.data) PM_HIP_TRY(hipMalloc(&t.data, numel * 4));
    PM_HIP_TRY(hipMemcpyAsync(t.data, dev, numel * 4, hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
    h->finalized = false;
    return PM_OK;
}

extern "C" int pm_vocos_finalize(pm_vocos_t h, void* stream) {
    if (!h) return pm_fail(PM_EINVAL, "null argument");
    for (auto& kv : h->tensors)
        if (!kv.second.data)
            return pm_fail(PM_ESTATE, "%s was not loaded", kv.first.c_str());
    hipStream_t s = (hipStream_t)stream;
    const int d = h->dtype, C = h->C, H = h->H;
    const size_t pre = packed_bytes(d, C, h->F, 7);
    const size_t emb = packed_bytes(d, C, C, 7);
    const size_t hd = packed_bytes(d, PM_VOCOS_HEAD_OUT, C, 1);
    const size_t per = block_weights(d, C, H, nullptr).total;
    const size_t total = pre + emb + hd + per * h->layers;
    if (!h->packed) PM_HIP_TRY(hipMalloc(&h->packed, total));
    char* base = (char*)h->packed;
    PM_HIP_TRY(pack(d, h->at("conv_pre.weight"), base, C, h->F, 7, s));
    h->conv_pre = base;
    base += pre;
    PM_HIP_TRY(pack(d, h->at("backbone.embed.weight"), base, C, C, 7, s));
    h->embed = base;
    base += emb;
    PM_HIP_TRY(pack(d, h->at("head.out.weight"), base, PM_VOCOS_HEAD_OUT, C, 1,
                    s));
    h->head = base;
    base += hd;
    h->w1.clear(); h->w2.clear(); h->dw.clear();
    for (int i = 0; i < h->layers; ++i) {
        const BlockWeights bw = block_weights(d, C, H, base);
        PM_HIP_TRY(pack(d, h->at(layer_key(i, "pwconv1.weight")), bw.w1, H, C,
                        1, s));
        PM_HIP_TRY(pack(d, h->at(layer_key(i, "pwconv2.weight")), bw.w2, C, H,
                        1, s));
        hipLaunchKernelGGL(vocos_dw_pack_kernel, dim3((7 * C + 255) / 256),
                           dim3(256), 0, s, h->at(layer_key(i, "dwconv.weight")),
                           bw.dw, C);
        PM_HIP_TRY(hipGetLastError());
        h->w1.push_back(bw.w1);
        h->w2.push_back(bw.w2);
        h->dw.push_back(bw.dw);
        base += bw.total;
    }
    h->finalized = true;
    return PM_OK;
}

// residual ping-pong (2 x rows x C fp32) | head logits (rows x 1026) | cond
// output (B x C); ragged: | row map (rows x 16 bytes) | offsets (B + 1)
struct VocosLayout {
    float *x0, *x1, *logits, *cond, *frames;
    VocosRow* map; int* off;
    size_t total;
};
static VocosLayout vocos_layout(pm_vocos_t h, int batch, int frames,
                                bool ragged, void* base) {
    const size_t rows = (size_t)batch * frames;
    PmCarve c(base);
    VocosLayout l = {};
    l.x0 = c.take<float>(rows * h->C);
    l.x1 = c.take<float>(rows * h->C);
    l.logits = c.take<float>(rows * PM_VOCOS_HEAD_OUT);
    l.cond = c.take<float>((size_t)batch * h->C);
    // the iSTFT frames overwrite the residual buffers, both dead once the
    // head has its logits: 2 x rows x 512 == rows x 1024 floats
    l.frames = l.x0;
    if (ragged) {
        l.map = c.take<VocosRow>(rows);
        l.off = c.take<int>((size_t)batch + 1);
    }
    l.total = c.used;
    return l;
}

extern "C" size_t pm_vocos_workspace_bytes(pm_vocos_t h, int batch,
                                           int frames) {
    if (!h || batch < 1 || frames < 1) return 0;
    return vocos_layout(h, batch, frames, false, nullptr).total;
}

extern "C" size_t pm_vocos_ragged_workspace_bytes(pm_vocos_t h, int batch,
                                                  int frames) {
    if (!h || batch < 1 || frames < 1) return 0;
    return vocos_layout(h, batch, frames, true, nullptr).total;
}

// lengths null: the uniform batch; else the ragged one, rows packed
static int vocos_forward(pm_vocos_t h, const float* features,
                         const float* global_features, int global_batch,
                         const int* lengths, bool ragged, float* audio,
                         int batch, int frames, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (!h || !features || !audio || (ragged && !lengths))
        return pm_fail(PM_EINVAL, "null argument");
    if (!h->finalized)
        return pm_fail(PM_ESTATE, "pm_vocos_finalize not called");
    if (batch < 1 || frames < 1)
        return pm_fail(PM_EINVAL, "batch and frames must be positive");
    if (global_features && global_batch != 1 && global_batch != batch)
        return pm_fail(PM_EINVAL, "global batch must be 1 or batch");
    const VocosLayout l = vocos_layout(h, batch, frames, ragged, workspace);
    if (!workspace || workspace_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)batch * frames;
    const int C = h->C, d = h->dtype;
    const VocosRagged rg = {l.map, l.off};
    if (ragged) {
        hipLaunchKernelGGL(vocos_rowmap_kernel,
                           dim3((frames + 255) / 256, batch), dim3(256), 0, s,
                           lengths, l.off, l.map, batch, frames);
        PM_HIP_TRY(hipGetLastError());
    }
    const int* total = ragged ? rg.off + batch : nullptr;

    // conv_pre(x) + cond(g)                                vocos.py:41-49
    if (global_features) {
        hipLaunchKernelGGL(vocos_cond_kernel, dim3((C + 255) / 256,
                                                   global_batch),
                           dim3(256), 0, s, global_features,
                           h->at("cond.weight"), h->at("cond.bias"), l.cond,
                           h->G, C);
        PM_HIP_TRY(hipGetLastError());
    }
    VocosGemmArgs g = {};
    g.x = features; g.w = h->conv_pre; g.bias = h->at("conv_pre.bias");
    g.gbias = global_features ? l.cond : nullptr; g.gbatch = global_batch;
    g.out = l.x1; g.B = batch; g.T = frames; g.K = h->F; g.N = C; g.ldo = C;
    g.rg = rg;
    PM_HIP_TRY(gemm(d, 7, true, g, s));
    // backbone embed + norm                                vocos.py:96-98
    g = {};
    g.x = l.x1; g.w = h->embed; g.bias = h->at("backbone.embed.bias");
    g.out = l.x0; g.B = batch; g.T = frames; g.K = C; g.N = C; g.ldo = C;
    g.rg = rg;
    PM_HIP_TRY(gemm(d, 7, false, g, s));
    PM_HIP_TRY(layer_norm(l.x0, h->at("backbone.norm.weight"),
                          h->at("backbone.norm.bias"), (int)rows, total, s));
    float* cur = l.x0;
    float* nxt = l.x1;
    for (int i = 0; i < h->layers; ++i) {
        VocosBlockArgs a = {};
        a.x = cur; a.y = nxt; a.dw_w = h->dw[i];
        a.dw_b = h->at(layer_key(i, "dwconv.bias"));
        a.ln_w = h->at(layer_key(i, "norm.weight"));
        a.ln_b = h->at(layer_key(i, "norm.bias"));
        a.w1 = h->w1[i]; a.b1 = h->at(layer_key(i, "pwconv1.bias"));
        a.w2 = h->w2[i]; a.b2 = h->at(layer_key(i, "pwconv2.bias"));
        a.gamma = h->at(layer_key(i, "gamma"));
        a.B = batch; a.T = frames; a.H = h->H; a.rg = rg;
        PM_HIP_TRY(block(d, a, s));
        std::swap(cur, nxt);
    }
    PM_HIP_TRY(layer_norm(cur, h->at("backbone.final_layer_norm.weight"),
                          h->at("backbone.final_layer_norm.bias"), (int)rows,
                          total, s));
    // head: cur -> logits, then the frames overwrite the residual buffers
    PM_HIP_TRY(head(d, cur, h->head, h->at("head.out.bias"),
                    h->at("head.istft.window"), l.logits, l.frames, audio,
                    batch, frames, rg, s));
    return PM_OK;
}

extern "C" int pm_vocos_forward(pm_vocos_t h, const float* features,
                                const float* global_features, int global_batch,
                                float* audio, int batch, int frames,
                                void* workspace, size_t workspace_bytes,
                                void* stream) {
    return vocos_forward(h, features, global_features, global_batch, nullptr,
                         false, audio, batch, frames, workspace,
                         workspace_bytes, stream);
}

extern "C" int pm_vocos_forward_ragged(pm_vocos_t h, const float* features,
                                       const float* global_features,
                                       int global_batch, const int* lengths,
                                       float* audio, int batch, int frames,
                                       void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return vocos_forward(h, features, global_features, global_batch, lengths,
                         true, audio, batch, frames, workspace,
                         workspace_bytes, stream);
}

// ---------------------------------------------------------------------------
// unit entries
// ---------------------------------------------------------------------------
extern "C" size_t pm_convnext_block_workspace_bytes(int dtype, int channels,
                                                    int hidden) {
    if (!known_dtype(dtype) || channels < 1 || hidden < 1) return 0;
    return block_weights(dtype, channels, hidden, nullptr).total;
}

extern "C" int pm_convnext_block_cl(
    int dtype, const float* x, float* y, const float* dw_w, const float* dw_b,
    const float* ln_w, const float* ln_b, const float* w1, const float* b1,
    const float* w2, const float* b2, const float* gamma, int batch,
    int frames, int channels, int hidden, void* workspace,
    size_t workspace_bytes, void* stream) {
    if (!x || !y || !dw_w || !dw_b || !ln_w || !ln_b || !w1 || !b1 || !w2 ||
        !b2 || !gamma)
        return pm_fail(PM_EINVAL, "null argument");
    if (x == y) return pm_fail(PM_EINVAL, "the block cannot run in place");
    if (!known_dtype(dtype))
        return pm_fail(PM_EINVAL, "dtype must be PM_F32, PM_F16 or PM_BF16");
    if (channels != PM_VOCOS_C || hidden < PM_VOCOS_HC ||
        hidden % PM_VOCOS_HC)
        return pm_fail(PM_EINVAL,
                       "unsupported block %d x %d", channels, hidden);
    if (batch < 1 || frames < 1)
        return pm_fail(PM_EINVAL, "batch and frames must be positive");
    const BlockWeights bw = block_weights(dtype, channels, hidden, workspace);
    if (!workspace || workspace_bytes < bw.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    PM_HIP_TRY(pack(dtype, w1, bw.w1, hidden, channels, 1, s));
    PM_HIP_TRY(pack(dtype, w2, bw.w2, channels, hidden, 1, s));
    hipLaunchKernelGGL(vocos_dw_pack_kernel, dim3((7 * channels + 255) / 256),
                       dim3(256), 0, s, dw_w, bw.dw, channels);
    PM_HIP_TRY(hipGetLastError());
    VocosBlockArgs a = {};
    a.x = x; a.y = y; a.dw_w = bw.dw; a.dw_b = dw_b; a.ln_w = ln_w;
    a.ln_b = ln_b;
    a.w1 = bw.w1; a.b1 = b1; a.w2 = bw.w2; a.b2 = b2; a.gamma = gamma;
    a.B = batch; a.T = frames; a.H = hidden;
    PM_HIP_TRY(block(dtype, a, s));
    return PM_OK;
}

extern "C" size_t pm_vocos_gemm_workspace_bytes(int dtype, int taps,
                                                int in_channels,
                                                int out_channels) {
    if (!known_dtype(dtype) || (taps != 1 && taps != 7) || in_channels < 1 ||
        out_channels < 1)
        return 0;
    return packed_bytes(dtype, out_channels, in_channels, taps);
}

extern "C" int pm_vocos_gemm_cl(int dtype, int taps, int channels_first,
                                const float* x, const float* w,
                                const float* bias, const float* gbias,
                                int gbatch, float* out, int batch, int frames,
                                int in_channels, int out_channels,
                                void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!x || !w || !bias || !out) return pm_fail(PM_EINVAL, "null argument");
    if (!known_dtype(dtype))
        return pm_fail(PM_EINVAL, "dtype must be PM_F32, PM_F16 or PM_BF16");
    // (the instantiations of gemm(): k7 in both layouts, k1 channels-last)
    if (taps != 1 && taps != 7)
        return pm_fail(PM_EINVAL, "taps must be 1 or 7, got %d", taps);
    if (channels_first && taps != 7)
        return pm_fail(PM_EINVAL, "channels-first input needs taps 7");
    if (batch < 1 || frames < 1)
        return pm_fail(PM_EINVAL, "batch and frames must be positive");
    if (in_channels < 16 || in_channels % 16)
        return pm_fail(PM_EINVAL,
                       "input channels must be a positive multiple of 16, got %d",
                       in_channels);
    if (out_channels < 1)
        return pm_fail(PM_EINVAL, "output channels must be positive, got %d",
                       out_channels);
    if (gbias && gbatch != 1 && gbatch != batch)
        return pm_fail(PM_EINVAL, "global batch must be 1 or batch");
    if (!workspace || workspace_bytes < pm_vocos_gemm_workspace_bytes(
            dtype, taps, in_channels, out_channels))
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    PM_HIP_TRY(pack(dtype, w, workspace, out_channels, in_channels, taps, s));
    VocosGemmArgs g = {};
    g.x = x; g.w = workspace; g.bias = bias; g.gbias = gbias;
    g.gbatch = gbatch; g.out = out; g.B = batch; g.T = frames;
    g.K = in_channels; g.N = out_channels; g.ldo = out_channels;
    PM_HIP_TRY(gemm(dtype, taps, channels_first != 0, g, s));
    return PM_OK;
}

extern "C" size_t pm_vocos_head_workspace_bytes(int dtype, int batch,
                                                int frames) {
    if (!known_dtype(dtype) || batch < 1 || frames < 1) return 0;
    return head_layout(dtype, batch, frames, nullptr).total;
}

extern "C" int pm_vocos_head(int dtype, const float* x, const float* w,
                             const float* bias, const float* window,
                             float* audio, int batch, int frames,
                             void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (!x || !w || !bias || !window || !audio)
        return pm_fail(PM_EINVAL, "null argument");
    if (!known_dtype(dtype))
        return pm_fail(PM_EINVAL, "dtype must be PM_F32, PM_F16 or PM_BF16");
    if (batch < 1 || frames < 1)
        return pm_fail(PM_EINVAL, "batch and frames must be positive");
    const HeadLayout l = head_layout(dtype, batch, frames, workspace);
    if (!workspace || workspace_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    PM_HIP_TRY(pack(dtype, w, l.w, PM_VOCOS_HEAD_OUT, PM_VOCOS_C, 1, s));
    PM_HIP_TRY(head(dtype, x, l.w, bias, window, l.logits, l.frames, audio,
                    batch, frames, VocosRagged{nullptr, nullptr}, s));
    return PM_OK;
}

extern "C" size_t pm_istft_workspace_bytes(int batch, int frames) {
    if (batch < 1 || frames < 1) return 0;
    return pm_align256((size_t)batch * frames * PM_VOCOS_NFFT * 4);
}

extern "C" int pm_istft(const float* spectrum, const float* window,
                        float* audio, int batch, int frames, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!spectrum || !window || !audio)
        return pm_fail(PM_EINVAL, "null argument");
    if (batch < 1 || frames < 1)
        return pm_fail(PM_EINVAL, "batch and frames must be positive");
    if (!workspace ||
        workspace_bytes < pm_istft_workspace_bytes(batch, frames))
        return pm_fail(PM_ENOMEM, "workspace too small");
    PM_HIP_TRY(istft(1, spectrum, window, (float*)workspace, audio, batch,
                     frames, nullptr, (hipStream_t)stream));
    return PM_OK;
}

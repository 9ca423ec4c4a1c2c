// The FARGAN engine of the C ABI (include/promonet_hip.h; config/fargan.py):
// replaces promonet.model.FARGAN. Kernels: pm_fargan.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pm_host.h"
#include "pm_fargan.h"

struct FLayer {
    const char* key;     // state-dict prefix (without .weight / .weight_g ...)
    const char* leaf;    // leaf of a plain tensor ("weight", "weight_ih", ...)
    bool normed;         // weight-normed Linear: accepts weight_g + weight_v
    int rows, cols, rpad, kpad;
    int kw = 0;              // > 0: also packed K-split, 8 x (rpad x kw)
    bool insensitive = false;  // stored f16 under PM_FARGAN_MIXED (GRU, gates)
    size_t offset = 0;       // element offsets into the one weight buffer
    size_t offset_k = 0;
    float* tmp_g = nullptr;
    float* tmp_v = nullptr;
    bool has = false;
};

struct pm_fargan_s {
    void* weights = nullptr;   // every packed layer (FarganWeights layout)
    void* weights_i = nullptr; // PM_FARGAN_MIXED: the f16-stored layers (same
                               // element offsets; only their regions are used)
    int nfeat, G, dtype;
    int mode = 0;        // 0 auto, 1 one workgroup per utterance, 2 clusters
    std::vector<FLayer> layers;
    bool finalized = false;
};

#define FG_P "subframe_network."
static std::vector<FLayer> fargan_layers(int nin) {
    const int cpad = 376;
    std::vector<FLayer> l = {
        {"conditioning_network.0", "weight", false, nin, nin, 384, cpad},
        {"conditioning_network.2", "weight", false, nin, nin, 384, cpad},
        {"conditioning_network.4", "weight", false, 512, nin, 512, cpad},
        {FG_P "framewise_convolution.model.0", "weight", true, 256, 520, 256, 520},
        {FG_P "framewise_convolution.model.2.gate", "weight", true, 256, 256, 256, 256},
        {FG_P "gru1", "weight_ih", false, 768, 384, 768, 384},
        {FG_P "gru2", "weight_ih", false, 768, 384, 768, 384},
        {FG_P "gru3", "weight_ih", false, 768, 384, 768, 384},
        {FG_P "gru1", "weight_hh", false, 768, 256, 768, 256},
        {FG_P "gru2", "weight_hh", false, 768, 256, 768, 256},
        {FG_P "gru3", "weight_hh", false, 768, 256, 768, 256},
        {FG_P "gru1_glu.gate", "weight", true, 256, 256, 256, 256},
        {FG_P "gru2_glu.gate", "weight", true, 256, 256, 256, 256},
        {FG_P "gru3_glu.gate", "weight", true, 256, 256, 256, 256},
        {FG_P "skip_dense", "weight", false, 256, 1152, 256, 1152},
        {FG_P "skip_glu.gate", "weight", true, 256, 256, 256, 256},
        {FG_P "output_layer", "weight", false, 64, 256, 64, 256},
    };
    // layers that contract a member-owned slice in the cluster kernel
    l[1].kw = 48;                                   // conditioning_network.2
    l[4].kw = 32;                                   // framewise conv GLU gate
    l[11].kw = l[12].kw = l[13].kw = 32;            // GRU GLU gates
    l[16].kw = 32;                                  // output layer
    // FgTypes<FgMixed>::I (pm_fargan.h): the GRU cells and the GLU gates
    for (int i : {4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15}) l[i].insensitive = true;
    // offsets = FarganWeights<>: row-packed layers in table order, then the
    // K-split copies
    size_t at = 0;
    for (auto& layer : l) {
        layer.offset = at;
        at += (size_t)layer.rpad * layer.kpad;
    }
    for (auto& layer : l)
        if (layer.kw) {
            layer.offset_k = at;
            at += (size_t)FG_G * layer.rpad * layer.kw;
        }
    return l;
}

extern "C" int pm_fargan_create(
    int num_features, int global_channels, int weight_dtype,
    pm_fargan_t* out) {
    if (!out) return pm_fail(PM_EINVAL, "null argument");
    if (num_features + global_channels != 371 || num_features < 1)
        return pm_fail(PM_EINVAL,
                       "FARGAN kernel is built for 113 + 258 conditioning "
                       "channels (config/fargan.py)");
    if (weight_dtype != PM_F32 && weight_dtype != PM_F16 &&
        weight_dtype != PM_FARGAN_MIXED)
        return pm_fail(PM_EINVAL,
                       "weight dtype must be PM_F32, PM_F16 or PM_FARGAN_MIXED");
    auto* h = new pm_fargan_s();
    h->nfeat = num_features; h->G = global_channels; h->dtype = weight_dtype;
    h->layers = fargan_layers(num_features + global_channels);
    typedef FarganWeights<float> W;
    const auto& l = h->layers;
    if (l[0].offset != W::COND0 || l[1].offset != W::COND1 ||
        l[2].offset != W::COND2 || l[3].offset != W::FWCONV ||
        l[4].offset != W::FWGLU || l[5].offset != W::GRU_IH ||
        l[8].offset != W::GRU_HH || l[11].offset != W::GRU_GLU ||
        l[14].offset != W::SKIP || l[15].offset != W::SKIP_GLU ||
        l[16].offset != W::OUT || l[1].offset_k != W::K_COND1 ||
        l[4].offset_k != W::K_FWGLU || l[11].offset_k != W::K_GRU_GLU ||
        l[16].offset_k != W::K_OUT) {
        delete h;
        return pm_fail(PM_ESTATE,
                       "FARGAN layer table and FarganWeights disagree");
    }
    *out = h;      // the weight buffer is allocated with the first tensor
    return PM_OK;
}

extern "C" int pm_fargan_destroy(pm_fargan_t h) {
    if (!h) return PM_OK;
    if (h->weights) hipFree(h->weights);
    if (h->weights_i) hipFree(h->weights_i);
    for (auto& l : h->layers) {
        if (l.tmp_g) hipFree(l.tmp_g);
        if (l.tmp_v) hipFree(l.tmp_v);
    }
    delete h;
    return PM_OK;
}

template <class WT>
static hipError_t fargan_pack_t(
    void* buffer, FLayer& l, const float* w, hipStream_t s) {
    const int gru = l.rows == 768 ? 1 : 0;   // gate-interleaved GRU rows
    const size_t elems = (size_t)l.rpad * l.kpad;
    WT* base = (WT*)buffer;
    hipLaunchKernelGGL(pm_fargan_pack_kernel<WT>,
                       dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s,
                       w, base + l.offset, l.rows, l.cols, l.rpad, l.kpad, gru,
                       0);
    if (l.kw) {
        // K-split copy: member g's sub-matrix W[:, g kw : (g + 1) kw]
        const size_t sub = (size_t)l.rpad * l.kw;
        for (int g = 0; g < FG_G; ++g)
            hipLaunchKernelGGL(pm_fargan_pack_kernel<WT>,
                               dim3((unsigned)((sub + 255) / 256)), dim3(256),
                               0, s, w, base + l.offset_k + g * sub, l.rows,
                               l.cols, l.rpad, l.kw, 0, g * l.kw);
    }
    return hipGetLastError();
}

static int fargan_pack(pm_fargan_t h, FLayer& l, const float* w, hipStream_t s) {
    if (!h->weights)
        PM_HIP_TRY(hipMalloc(&h->weights, FarganWeights<float>::TOTAL *
                                              (h->dtype == PM_F16 ? 2 : 4)));
    if (h->dtype == PM_FARGAN_MIXED && !h->weights_i)
        PM_HIP_TRY(hipMalloc(&h->weights_i, FarganWeights<float>::TOTAL * 2));
    if (h->dtype == PM_FARGAN_MIXED && l.insensitive)
        PM_HIP_TRY(fargan_pack_t<_Float16>(h->weights_i, l, w, s));
    else if (h->dtype == PM_F16)
        PM_HIP_TRY(fargan_pack_t<_Float16>(h->weights, l, w, s));
    else
        PM_HIP_TRY(fargan_pack_t<float>(h->weights, l, w, s));
    l.has = true;
    return PM_OK;
}

extern "C" int pm_fargan_load_tensor(
    pm_fargan_t h, const char* name, const float* dev, const int64_t* shape,
    int ndim, void* stream) {
    if (!h || !name || !dev || !shape)
        return pm_fail(PM_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    for (auto& l : h->layers) {
        const size_t n = strlen(l.key);
        if (strncmp(name, l.key, n) || name[n] != '.') continue;
        const char* leaf = name + n + 1;
        if (!strcmp(leaf, l.leaf)) {
            if (ndim != 2 || shape[0] != l.rows || shape[1] != l.cols)
                return pm_fail(PM_EINVAL, "%s: expected shape (%d, %d)", name,
                               l.rows, l.cols);
            int rc = fargan_pack(h, l, dev, s);
            if (rc) return rc;
        } else if (l.normed && (!strcmp(leaf, "weight_g") ||
                                !strcmp(leaf, "weight_v"))) {
            const bool is_g = leaf[7] == 'g';
            if (is_g) {
                if (ndim != 2 || shape[0] != l.rows || shape[1] != 1)
                    return pm_fail(PM_EINVAL,
                                   "%s: expected (%d, 1)", name, l.rows);
                int rc = pm_copy_dev(&l.tmp_g, dev, l.rows, s);
                if (rc) return rc;
            } else {
                if (ndim != 2 || shape[0] != l.rows || shape[1] != l.cols)
                    return pm_fail(PM_EINVAL, "%s: expected (%d, %d)", name,
                                   l.rows, l.cols);
                int rc = pm_copy_dev(&l.tmp_v, dev, (size_t)l.rows * l.cols, s);
                if (rc) return rc;
            }
            if (l.tmp_g && l.tmp_v) {
                float* folded = nullptr;
                PM_HIP_TRY(hipMalloc((void**)&folded,
                                     (size_t)l.rows * l.cols * sizeof(float)));
                int rc = pm_fold_weight_norm(l.tmp_g, l.tmp_v, folded, l.rows,
                                             l.cols, s);
                if (rc) return rc;
                rc = fargan_pack(h, l, folded, s);
                PM_HIP_TRY(hipStreamSynchronize(s));
                hipFree(folded); hipFree(l.tmp_g); hipFree(l.tmp_v);
                l.tmp_g = l.tmp_v = nullptr;
                if (rc) return rc;
            }
        } else {
            continue;   // e.g. gru1.weight_hh is a different table row
        }
        PM_HIP_TRY(hipStreamSynchronize(s));
        h->finalized = false;
        return PM_OK;
    }
    return pm_fail(PM_EINVAL, "%s: not a FARGAN state-dict key", name);
}

extern "C" int pm_fargan_finalize(pm_fargan_t h, void* stream) {
    if (!h) return pm_fail(PM_EINVAL, "null handle");
    for (auto& l : h->layers)
        if (!l.has)
            return pm_fail(PM_ESTATE, "missing tensor: %s.%s", l.key, l.leaf);
    PM_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    h->finalized = true;
    return PM_OK;
}

// Kernel choice. Measured (MI355X, 10 s utterances, fp32 weights): clusters of
// 8 workgroups take 112 ms for 32 utterances (one per cluster), 162 ms for 64
// (two in lockstep per cluster), 242 ms for 128 and 485 ms for 256 (four in
// lockstep, two waves); one workgroup per utterance takes 721 ms per wave of
// 256 -> clusters at every batch size, PROVIDED every workgroup of the grid is
// resident at once: the members of a cluster wait for each other's granules.
// The grid is therefore sized from the device: one 768-thread workgroup per CU
// (its LDS / wave budget admits at least that on any gfx950 partition), i.e.
// at most multiProcessorCount / 8 clusters; a device with fewer than 8 CUs
// visible gets the one-workgroup-per-utterance kernel. What the query cannot
// see (another process sharing the GPU, a CU mask) is caught by the bounded
// spins: pm_fargan_check reports the timeout and the caller re-runs with
// pm_fargan_set_mode(h, 1). pm_fargan_set_mode() overrides the choice
// (a -DPM_TUNING build also reads PM_FARGAN=single|cluster).
static const int FG_MAX_CLUSTERS = 32;   // 32 x 8 workgroups = one per CU

static int fargan_resident_clusters() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess)
        return 0;
    const int n = cus / FG_G;
    return n < FG_MAX_CLUSTERS ? n : FG_MAX_CLUSTERS;
}

static bool fargan_use_cluster(pm_fargan_t h, int B) {
    int mode = h->mode;
#ifdef PM_TUNING
    static const int forced = [] {
        const char* e = getenv("PM_FARGAN");
        return !e ? 0 : (!strcmp(e, "single") ? 1 : (!strcmp(e, "cluster") ? 2 : 0));
    }();
    if (!mode) mode = forced;
#endif
    (void)B;
    if (mode == 1) return false;
    return fargan_resident_clusters() >= 1;
}

extern "C" int pm_fargan_set_mode(pm_fargan_t h, int mode) {
    if (!h || mode < 0 || mode > 2) return pm_fail(PM_EINVAL, "bad mode");
    h->mode = mode;
    return PM_OK;
}

// channels-last features | cluster state | its error word | conditioning
struct FarganLayout {
    float* features; unsigned* state; unsigned* error; float* cond;
    size_t total;
};
static const size_t FG_STATE_WORDS = (size_t)FG_MAX_CLUSTERS * FG_CSTATE;
static_assert(FG_STATE_WORDS % 64 == 0, "the error word follows the state");

static FarganLayout fargan_layout(pm_fargan_t h, int B, int T, void* base) {
    PmCarve c(base);
    // cond: (B * T, 512) conditioning vectors of pm_fargan_cond_kernel,
    // fp32-stored conditioning weights only (f16 storage keeps them inside
    // the cluster kernel)
    return {c.take<float>((size_t)B * T * pm_pad32(h->nfeat + 1)),
            c.take<unsigned>(FG_STATE_WORDS), c.take<unsigned>(1),
            h->dtype != PM_F16 ? c.take<float>((size_t)B * T * 512) : nullptr,
            c.used};
}

extern "C" size_t pm_fargan_workspace_bytes(pm_fargan_t h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    return fargan_layout(h, B, T, nullptr).total;
}

// st.states_out != null: the stateful instantiations (pm_fargan_forward_stateful)
// cl: the workspace of the cluster kernels, or null for one workgroup per
// utterance
template <class WT>
static int fargan_launch(
    pm_fargan_t h, const FarganArgs& a, hipStream_t s, const FarganLayout* cl,
    const FarganState& st) {
    const bool stateful = st.states_out != nullptr;
    FarganWeights<WT> w;
    w.base = (const typename FarganWeights<WT>::S*)h->weights;
    w.base_i = (const typename FarganWeights<WT>::I*)(
        h->weights_i ? h->weights_i : h->weights);
    if (cl) {
        // counters / payload / error word are re-initialised on every call
        // (the state's slot and, straight behind it, the error word's)
        PM_HIP_TRY(hipMemsetAsync(
            cl->state, 0, (FG_STATE_WORDS + 64) * sizeof(unsigned), s));
        FarganClusterArgs ca;
        ca.f = a;
        ca.state = cl->state;
        ca.error = cl->error;
        ca.precond = nullptr;
        if constexpr (std::is_same<typename FarganWeights<WT>::S, float>::value) {
            // the conditioning network of every frame, ahead of the walk
            FarganCondArgs cn;
            cn.features_cl = a.features_cl; cn.global = a.global;
            cn.cond = cl->cond;
            cn.B = a.B; cn.T = a.T; cn.cstride = a.cstride; cn.nfeat = a.nfeat;
            cn.G = a.G; cn.global_batch = a.global_batch;
            const size_t cond_lds =
                (size_t)FG_CN * (FG_CPITCH + FG_OPITCH) * sizeof(float);
            hipError_t ce = pm_ensure_dynamic_lds(
                reinterpret_cast<const void*>(pm_fargan_cond_kernel),
                (int)cond_lds);
            PM_HIP_TRY(ce);
            const long long frames = (long long)a.B * a.T;
            hipLaunchKernelGGL(
                pm_fargan_cond_kernel,
                dim3((unsigned)((frames + FG_CN - 1) / FG_CN)), dim3(256),
                cond_lds, s, cn, w.base + FarganWeights<WT>::COND0,
                w.base + FarganWeights<WT>::COND1,
                w.base + FarganWeights<WT>::COND2);
            PM_HIP_TRY(hipGetLastError());
            ca.precond = cn.cond;
        }
#ifdef PM_TUNING
        ca.timeline = pm_timeline();
#endif
        // U utterances per cluster in lockstep: 1 while one cluster per
        // utterance fits the resident grid (32 clusters = 256 CUs), then 2,
        // then 4; beyond that the clusters walk the batch in waves
        const int resident = fargan_resident_clusters();
        if (resident < 1)
            return pm_fail(PM_ESTATE,
                           "FARGAN cluster kernel needs >= %d CUs", FG_G);
        const int U = a.B <= resident ? 1 : a.B <= 2 * resident ? 2 : FG_UMAX;
        const int groups = (a.B + U - 1) / U;
        ca.nclusters = groups < resident ? groups : resident;
        const dim3 grid(ca.nclusters * FG_G), block(FG_CT);
        // (+ the LDS-resident short slices of a one-utterance cluster)
        const size_t smem = (size_t)U * sizeof(FgLds) +
                            (U == 1 ? FgResident<WT, 1>::BYTES : 0);
        auto launch = [&](auto kern, const auto& args) -> hipError_t {
            hipError_t e = pm_ensure_dynamic_lds(
                reinterpret_cast<const void*>(kern), (int)smem);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, grid, block, smem, s, args, w);
            return hipGetLastError();
        };
        auto pick = [&](const auto& args) -> hipError_t {
            typedef std::decay_t<decltype(args)> CA;
            return U == 1 ? launch(pm_fargan_cluster_kernel<WT, 1, CA>, args)
                 : U == 2 ? launch(pm_fargan_cluster_kernel<WT, 2, CA>, args)
                          : launch(pm_fargan_cluster_kernel<WT, FG_UMAX, CA>, args);
        };
        FgStateful<FarganClusterArgs> sca;
        static_cast<FarganClusterArgs&>(sca) = ca;
        static_cast<FarganState&>(sca) = st;
        PM_HIP_TRY(stateful ? pick(sca) : pick(ca));
        return PM_OK;
    }
    if (stateful) {
        FgStateful<FarganArgs> sa;
        static_cast<FarganArgs&>(sa) = a;
        static_cast<FarganState&>(sa) = st;
        auto kern = pm_fargan_kernel<WT, FgStateful<FarganArgs>>;
        hipLaunchKernelGGL(kern, dim3(a.B), dim3(FG_THREADS), 0, s, sa, w);
    } else {
        hipLaunchKernelGGL(pm_fargan_kernel<WT>, dim3(a.B), dim3(FG_THREADS), 0, s,
                           a, w);
    }
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

// Synchronises `stream` and reports whether a cluster exchange of the last
// forward on `workspace` gave up (bounded spin): PM_OK or PM_EHIP.
extern "C" int pm_fargan_check(
    pm_fargan_t h, int B, int T, void* ws, void* stream) {
    if (!h || !ws) return pm_fail(PM_EINVAL, "null argument");
    if (!fargan_use_cluster(h, B)) return PM_OK;
    unsigned flag = 0;
    PM_HIP_TRY(hipMemcpyAsync(
        &flag, fargan_layout(h, B, T, ws).error, 4, hipMemcpyDeviceToHost,
        (hipStream_t)stream));
    PM_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (flag) return pm_fail(PM_ETIMEOUT, "FARGAN cluster exchange timed out");
    return PM_OK;
}

// FARGAN.forward (model/fargan.py:21-59): features (B, nfeat + 1, T) with the
// pitch period as last channel (or channels-last (B, T, pad32(nfeat + 1)) when
// features_cl != 0), global (Bg, G), previous (Bp, 512) or NULL -> (B, 1, 256 T)
static int fargan_forward_impl(
    pm_fargan_t h, const float* features, int features_cl, const float* g,
    int gbatch, const float* previous, int pbatch, const int* lengths,
    float* out, int B, int T, void* ws, size_t ws_bytes, void* stream,
    const FarganState& st = FarganState()) {
    if (!h || !features || !g || !out)
        return pm_fail(PM_EINVAL, "null argument");
    if (!h->finalized)
        return pm_fail(PM_ESTATE, "pm_fargan_finalize not called");
    if (B < 1 || T < 1) return pm_fail(PM_EINVAL, "empty batch or sequence");
    if ((gbatch != 1 && gbatch != B) || (previous && pbatch != 1 && pbatch != B))
        return pm_fail(PM_EINVAL, "broadcast batch must be 1 or batch");
    hipStream_t s = (hipStream_t)stream;
    const int cpad = pm_pad32(h->nfeat + 1);
    const float* fcl = features;
    const FarganLayout l = fargan_layout(h, B, T, ws);
    if (!ws || ws_bytes < l.total)
        return pm_fail(PM_ENOMEM, "workspace too small");
    const FarganLayout* cl = fargan_use_cluster(h, B) ? &l : nullptr;
    if (!features_cl) {
        int rc = pm_to_channels_last(features, l.features, B, h->nfeat + 1, T,
                                     cpad, s);
        if (rc) return rc;
        fcl = l.features;
    }
    FarganArgs a;
    a.features_cl = fcl; a.global = g; a.previous = previous; a.out = out;
    a.B = B; a.T = T; a.cstride = cpad; a.nfeat = h->nfeat; a.G = h->G;
    a.global_batch = gbatch; a.previous_batch = pbatch;
    a.lengths = lengths;
    return h->dtype == PM_F32 ? fargan_launch<float>(h, a, s, cl, st)
         : h->dtype == PM_F16 ? fargan_launch<_Float16>(h, a, s, cl, st)
                              : fargan_launch<FgMixed>(h, a, s, cl, st);
}

extern "C" int pm_fargan_forward(
    pm_fargan_t h, const float* features, int features_cl, const float* g,
    int gbatch, const float* previous, int pbatch, float* out, int B, int T,
    void* ws, size_t ws_bytes, void* stream) {
    return fargan_forward_impl(h, features, features_cl, g, gbatch, previous,
                               pbatch, nullptr, out, B, T, ws, ws_bytes, stream);
}

// Ragged batch: utterance b is lengths[b] <= T frames long inside the padded
// tensors. FARGAN is causal (frame t reads features <= t only), so the valid
// prefix equals the stand-alone synthesis bit for bit; the tail is zeros.
extern "C" int pm_fargan_forward_ragged(
    pm_fargan_t h, const float* features, int features_cl, const float* g,
    int gbatch, const float* previous, int pbatch, const int* lengths,
    float* out, int B, int T, void* ws, size_t ws_bytes, void* stream) {
    if (!lengths) return pm_fail(PM_EINVAL, "null lengths");
    return fargan_forward_impl(h, features, features_cl, g, gbatch, previous,
                               pbatch, lengths, out, B, T, ws, ws_bytes, stream);
}

static_assert(FG_STATE == PM_FARGAN_STATE_FLOATS, "FARGAN state row");

// FARGAN.step (model/fargan.py:65-131) for `frames` consecutive frames, from
// the recurrent state `states` / `previous` (NULL: zeros) to the state after
// the last frame. The kernels are the forward's with a state prologue and
// epilogue, so consecutive calls carrying the state equal one forward over
// the concatenated frames, bit for bit. The outputs may not overlap an input
// (nor the workspace, nor each other): a relaunch after a timed-out cluster
// exchange reads the inputs again.
extern "C" int pm_fargan_forward_stateful(
    pm_fargan_t h, const float* features, int features_cl, const float* g,
    int gbatch, const float* previous, int pbatch, const float* states,
    float* out, float* previous_out, float* states_out, int B, int T,
    void* ws, size_t ws_bytes, void* stream) {
    if (!h || !features || !g || !out || !previous_out || !states_out)
        return pm_fail(PM_EINVAL, "null argument");
    if (B < 1 || T < 1) return pm_fail(PM_EINVAL, "empty batch or sequence");
    if ((gbatch != 1 && gbatch != B) || (previous && pbatch != 1 && pbatch != B))
        return pm_fail(PM_EINVAL, "broadcast batch must be 1 or batch");
    const size_t F = sizeof(float);
    const int channels = features_cl ? pm_pad32(h->nfeat + 1) : h->nfeat + 1;
    struct Span { const void* p; size_t n; };
    const Span in[] = {
        {features, (size_t)B * T * channels * F}, {g, (size_t)gbatch * h->G * F},
        {previous, (size_t)pbatch * FG_PREV * F}, {states, (size_t)B * FG_STATE * F},
        {ws, ws_bytes}};
    const Span outs[] = {
        {out, (size_t)B * T * FG_HOP * F}, {previous_out, (size_t)B * FG_PREV * F},
        {states_out, (size_t)B * FG_STATE * F}};
    for (int o = 0; o < 3; ++o) {
        for (const Span& i : in)
            if (pm_overlap(outs[o].p, outs[o].n, i.p, i.n))
                return pm_fail(PM_EINVAL,
                               "an output overlaps an input or the workspace");
        for (int q = o + 1; q < 3; ++q)
            if (pm_overlap(outs[o].p, outs[o].n, outs[q].p, outs[q].n))
                return pm_fail(PM_EINVAL, "outputs overlap");
    }
    FarganState st;
    st.states = states; st.states_out = states_out; st.previous_out = previous_out;
    return fargan_forward_impl(h, features, features_cl, g, gbatch, previous,
                               pbatch, nullptr, out, B, T, ws, ws_bytes, stream,
                               st);
}

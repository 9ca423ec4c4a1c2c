// Host side of the MFMA convolutions: the tile geometry per layer shape, the
// planner that chooses which kernel runs each MRF stage (pm_plan_*), and the
// launchers that launch what it chose (pm_launch_*). The launchers are
// explicitly instantiated once per operand type in pm_conv_*.hip so that the
// types compile in parallel.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "pm_conv.h"
#include "pm_host.h"

// Test hooks (pm_debug_force): the walked kernels and the multi-block path of
// the wide upsampler are chosen from the grid size, which unit-sized inputs
// never reach. walk_nseg > 0: take the walked variant wherever it exists, with
// that many segments per utterance; upsample_groups > 0: that many M groups
// per column tile. 0 = the production heuristics.
// skew: -1 = never the skewed walk, 0 = where it measured faster, 1 = wherever
// it fits.
struct PmForce { int walk_nseg = 0; int upsample_groups = 0; int skew = 0; };
// scratch the skewed walk takes per workgroup, at most
#define PM_SKEW_WG_SCRATCH (256 << 10)
// (per host thread: see pm_debug_force in pm_api.hip)
inline PmForce& pm_force() { static thread_local PmForce f; return f; }

// Latency (narrow-tile) variants can be switched off for A/B runs in a
// -DPM_TUNING build only; the shipped library reads no environment.
inline bool pm_narrow_allowed() {
#ifdef PM_TUNING
    static const bool allowed = !getenv("PM_NO_NARROW");
    return allowed;
#else
    return true;
#endif
}

// Fusion level: 2 = whole-MRF launches where they exist, 1 = one kernel per
// Block, 0 = one kernel per Block iteration. The shipped library always runs
// level 2; a -DPM_TUNING build reads PM_FUSION=pair|block for A/B runs.
inline int pm_fusion_level() {
#ifdef PM_TUNING
    static const int level = [] {
        const char* e = getenv("PM_FUSION");
        return (e && !strcmp(e, "pair")) ? 0 : (e && !strcmp(e, "block")) ? 1 : 2;
    }();
    return level;
#else
    return 2;
#endif
}

// LDS a walked or skewed workgroup may take
#define PM_LDS_BYTES (160 * 1024)

// 1: the wide upsampler stores rows through LDS (launch_upsample_cfg; the
// r = 2 upsamplers: PM_SINGLE_ROWS, pm_conv.h); 0: direct stores, for A/B builds
#ifndef PM_UPSAMPLE_ROWS
#define PM_UPSAMPLE_ROWS 1
#endif

// ---- fused pair geometry per (operand type, C) ---------------------------
template <class ET, int C> struct PairCfg;
// 16-bit operands: every wave owns a 32 (co) x 128 (time) register tile, so
// one A fragment (weights, streamed L2 -> VGPR) feeds 4 MFMAs: the vector
// memory path, not the matrix pipe, was the limiter at 2 loads per 4 MFMAs
// (rocprof r01: MFMA busy 43 %). C = 128 takes 256-column tiles
// (LDS 160,480 B at k 11, d 5).
// CH: input channels staged per LDS chunk (one barrier per chunk). Measured:
// CH = 128 (half the barriers, LDS tiles aliased) is 4 % slower than 64.
// 192 columns per weight fetch (LDS tiles aliased to fit): the pair kernels
// run at the power wall with the L2 94 % busy streaming weights, so fewer L2
// bytes per MFMA is what buys clock (measured -7 % on k 7 / k 11).
// (r02: 64 x 128 wave tiles on 256-column workgroup tiles with CH = 32 are
// 3-5 % slower at every k - profiles/r02/ab_tile_variants.txt)
template <> struct PairCfg<ElemF16, 256> { enum { WM = 8, WN = 1, NTW = 6, CH = 64, ALIAS = 1 }; };
// C = 128 alternatives measured and dropped: 384-column tiles with CH = 32
// (neutral), two 4-wave 128-column workgroups per CU (neutral: L2 weight
// traffic doubles), one fat wave per SIMD with 64 x 128 tiles (+1...+4 %).
// r02: 4-wave workgroups of 64 x 128 wave tiles, two per CU (CH = 32, tiles
// aliased) spill the staging registers and run 8-15 % slower; the same tiling
// fed by LDS-DMA from a 16-bit copy of lrelu(x) (no staging registers, no
// spills) is still 3-6 % slower, 8 waves on 512 columns 7-13 % slower
// (profiles/r02/ab_pair_dma_*.txt).
template <> struct PairCfg<ElemF16, 128> { enum { WM = 4, WN = 2, NTW = 4, CH = 64, ALIAS = 0 }; };
template <> struct PairCfg<ElemF16, 64>  { enum { WM = 2, WN = 2, NTW = 2, CH = 64, ALIAS = 0 }; };
template <> struct PairCfg<ElemF16, 32>  { enum { WM = 1, WN = 4, NTW = 1, CH = 32, ALIAS = 0 }; };
template <int C> struct PairCfg<ElemBF16, C> : PairCfg<ElemF16, C> {};
// exact fp32 operands: LDS rows are twice as wide -> 64-column tiles
// (round 4: 128-column tiles with the conv1 -> conv2 tile overlaying the x
// chunks instead of 64-column ones: 8 % of the columns recomputed instead of
// 16 % at k 11 and half the weight bytes per column - config 2 22.1 -> 20.4 ms;
// 192 columns at C = 128, where they fit: 19.7 ms - profiles/r04/ab_x3_skew.txt)
template <> struct PairCfg<ElemF32, 256> { enum { WM = 4, WN = 2, NTW = 2, CH = 64, ALIAS = 1 }; };
template <> struct PairCfg<ElemF32, 128> { enum { WM = 4, WN = 2, NTW = 3, CH = 64, ALIAS = 1 }; };
template <> struct PairCfg<ElemF32, 64>  { enum { WM = 2, WN = 2, NTW = 1, CH = 64, ALIAS = 0 }; };
template <> struct PairCfg<ElemF32, 32>  { enum { WM = 1, WN = 4, NTW = 1, CH = 32, ALIAS = 0 }; };
// split f16 (hi + lo, three MFMAs per step): 4 bytes per element like fp32,
// the same tiles
template <int C> struct PairCfg<ElemF16X3, C> : PairCfg<ElemF32, C> {};
// activations split, weights single f16: the same LDS tiles
template <int C> struct PairCfg<ElemF16A2, C> : PairCfg<ElemF32, C> {};

// Latency variant: when the wide tiling yields fewer workgroups than the chip
// has CUs (single utterances: 8 tiles at C = 256 for 2 s of audio), 64-column
// (C = 256) / 128-column (C = 128) tiles put 3x / 2x as many CUs to work on a
// third / half of the per-tile critical path. More halo recompute and weight
// traffic per column, so only below PM_NARROW_BELOW workgroups.
template <class ET, int C> struct PairCfgNarrow : PairCfg<ET, C> {};
// (CH must equal the wide variant's: both read the same packed weights)
template <> struct PairCfgNarrow<ElemF16, 256> { enum { WM = 8, WN = 1, NTW = 2, CH = PairCfg<ElemF16, 256>::CH, ALIAS = 1 }; };
template <> struct PairCfgNarrow<ElemF16, 128> { enum { WM = 4, WN = 2, NTW = 2, CH = PairCfg<ElemF16, 128>::CH, ALIAS = 0 }; };
// (fp32: the 64-column tiles of rounds 1-3 as the latency variant)
template <> struct PairCfgNarrow<ElemF32, 256> { enum { WM = 4, WN = 2, NTW = 1, CH = 64, ALIAS = 0 }; };
template <> struct PairCfgNarrow<ElemF32, 128> { enum { WM = 4, WN = 2, NTW = 1, CH = 64, ALIAS = 0 }; };
template <> struct PairCfgNarrow<ElemF16X3, 256> : PairCfgNarrow<ElemF32, 256> {};
template <> struct PairCfgNarrow<ElemF16X3, 128> : PairCfgNarrow<ElemF32, 128> {};
template <> struct PairCfgNarrow<ElemF16A2, 256> : PairCfgNarrow<ElemF32, 256> {};
template <> struct PairCfgNarrow<ElemF16A2, 128> : PairCfgNarrow<ElemF32, 128> {};
template <> struct PairCfgNarrow<ElemBF16, 256> : PairCfgNarrow<ElemF16, 256> {};
template <> struct PairCfgNarrow<ElemBF16, 128> : PairCfgNarrow<ElemF16, 128> {};
#define PM_NARROW_BELOW 150   // 3x the tiles must still fit ~2 rounds of 256 CUs

// The MRF conv weights are packed once, in chunks of min(C, 64) input channels
// (the whole-Block kernels' chunk, block3_body): every pair geometry streams
// the same packing, so the fusion level never changes it.
template <class ET, int C> constexpr bool pm_one_packing_c() {
    return PairCfg<ET, C>::CH == (C < 64 ? C : 64) &&
           PairCfgNarrow<ET, C>::CH == PairCfg<ET, C>::CH;
}
template <class ET> constexpr bool pm_one_packing() {
    return pm_one_packing_c<ET, 32>() &&
           pm_one_packing_c<ET, 64>() &&
           pm_one_packing_c<ET, 128>() &&
           pm_one_packing_c<ET, 256>();
}
static_assert(pm_one_packing<ElemF32>() &&
              pm_one_packing<ElemF16>() &&
              pm_one_packing<ElemBF16>() &&
              pm_one_packing<ElemF16X3>() &&
              pm_one_packing<ElemF16A2>(),
              "pair and whole-Block kernels read one weight packing");

// ---- whole-Block fusion ---------------------------------------------------
// Geometry per (operand type, C, K). WM == 0: no whole-Block instantiation
// (the caller runs one pair kernel per iteration instead). Measured: halving
// the columns PER WAVE so that two workgroups share a CU is slower (C = 64
// k 3: 1.65 vs 1.22 ms - the fixed cost per barrier phase dominates), so a
// wave always keeps the widest register tile.
template <class ET, int C, int K> struct Block3Cfg { enum { WM = 0, WN = 1, NTW = 1 }; };
// Small k (halo <= 36 columns): two 4-wave workgroups per CU with the same
// per-wave work beat one 8-wave workgroup (their phases interleave): -14 %
// at C = 32 k 3, -5 % at C = 32 k 7, -13 % at C = 64 k 3. With a larger halo
// (k 11, or k 7 at C = 64) the extra recompute eats the gain; at C = 128 it is
// 28 % slower.
template <> struct Block3Cfg<ElemF16, 32, 3>   { enum { WM = 1, WN = 4, NTW = 3 }; };
template <> struct Block3Cfg<ElemF16, 32, 7>   { enum { WM = 1, WN = 4, NTW = 3 }; };
// (8 waves at C = 32 k 3 / 7 for the skewed walk: +25 %, profiles/r06/ab_skew16.txt)
template <> struct Block3Cfg<ElemF16, 32, 11>  { enum { WM = 1, WN = 8, NTW = 3 }; };
template <> struct Block3Cfg<ElemF16, 64, 3>   { enum { WM = 2, WN = 2, NTW = 4 }; };
template <> struct Block3Cfg<ElemF16, 64, 7>   { enum { WM = 2, WN = 4, NTW = 4 }; };
template <> struct Block3Cfg<ElemF16, 64, 11>  { enum { WM = 2, WN = 4, NTW = 4 }; };
// (3 tiles per wave at C = 128 k 3: not faster, profiles/r06/ab_k3_tiles.txt)
template <> struct Block3Cfg<ElemF16, 128, 3>  { enum { WM = 4, WN = 2, NTW = 4 }; };
// C = 128, k 7: walked only (conv_block3_walk_kernel; stand-alone, the 36-column
// halo on both sides of a 256-column tile made it 28 % slower than three pair
// launches - walked it is 10.6 % faster, profiles/r02/ab_block128_k7_walk.txt)
template <> struct Block3Cfg<ElemF16, 128, 7>  { enum { WM = 4, WN = 2, NTW = 4 }; };
// C = 128, k 11: skewed walk only (conv_block3_skew_kernel)
template <> struct Block3Cfg<ElemF16, 128, 11> { enum { WM = 4, WN = 2, NTW = 4 }; };
// C = 256, k 3: walked only, 128-column tiles (12 of them halo): 0.67 -> 0.53 ms
// against three pair launches (profiles/r02/ab_block256_walk.txt)
template <> struct Block3Cfg<ElemF16, 256, 3>  { enum { WM = 8, WN = 1, NTW = 4 }; };
// C = 256, k 7: skewed walk only
template <> struct Block3Cfg<ElemF16, 256, 7>  { enum { WM = 8, WN = 1, NTW = 4 }; };
// (k 7 the same way: 36 of 128 columns halo, 1.45 vs 1.19 ms - stays on the pair kernel)
// (k 11 the same way - it fits 160 KB once `t` loses its right margin too - is
// 7 % slower than three pair launches: 31 % more MFMA work)
template <int C, int K> struct Block3Cfg<ElemBF16, C, K> : Block3Cfg<ElemF16, C, K> {};
template <> struct Block3Cfg<ElemF32, 32, 3>   { enum { WM = 1, WN = 8, NTW = 2 }; };
template <> struct Block3Cfg<ElemF32, 32, 7>   { enum { WM = 1, WN = 8, NTW = 2 }; };
template <> struct Block3Cfg<ElemF32, 32, 11>  { enum { WM = 1, WN = 8, NTW = 2 }; };
template <> struct Block3Cfg<ElemF32, 64, 3>   { enum { WM = 2, WN = 4, NTW = 2 }; };
template <> struct Block3Cfg<ElemF32, 64, 7>   { enum { WM = 2, WN = 4, NTW = 2 }; };
template <> struct Block3Cfg<ElemF32, 64, 11>  { enum { WM = 2, WN = 4, NTW = 2 }; };
template <int C, int K> struct Block3Cfg<ElemF16X3, C, K> : Block3Cfg<ElemF32, C, K> {};
template <int C, int K> struct Block3Cfg<ElemF16A2, C, K> : Block3Cfg<ElemF32, C, K> {};

// Latency variants (see PairCfgNarrow): half the waves, same per-wave tile.
template <class ET, int C, int K> struct Block3CfgNarrow : Block3Cfg<ET, C, K> {};
template <> struct Block3CfgNarrow<ElemF16, 32, 11> { enum { WM = 1, WN = 4, NTW = 3 }; };
template <> struct Block3CfgNarrow<ElemF16, 64, 7>  { enum { WM = 2, WN = 2, NTW = 4 }; };
template <> struct Block3CfgNarrow<ElemF16, 64, 11> { enum { WM = 2, WN = 2, NTW = 4 }; };
template <> struct Block3CfgNarrow<ElemF16, 128, 3> { enum { WM = 4, WN = 1, NTW = 4 }; };
template <int C, int K> struct Block3CfgNarrow<ElemBF16, C, K> : Block3CfgNarrow<ElemF16, C, K> {};

// ---- which kernels exist per geometry ---------------------------------------
// The 4-byte operand layouts (exact fp32, split f16, split activations) run
// their C = 32 / 64 Blocks on the skewed walk where it fits: at 16 times / three
// times the MFMA time per step, what the skew removes - the two-sided
// tilings' halo recompute - shows (split f16: three skewed Block launches
// 6.07 ms against 6.99 ms for the fused whole-MRF tiling,
// profiles/r04/ab_x3_skew.txt; fp32: profiles/r05/ab_x3skew_f32.txt). The
// 16-bit types stay on the walked / whole-MRF kernels at C = 32 (skewed: +25 %,
// profiles/r06/ab_skew16.txt).
template <class ET, int C>
constexpr bool pm_skew_4byte() { return ET::ESZ == 4 && (C == 32 || C == 64); }

// Whole-Block kernels instantiated for geometry G (Block3Cfg or its narrow
// variant): the skewed walk (no recompute at all), the walked tiling (no
// left-halo recompute: where its carry area fits the LDS) and the two-sided
// tiling. C = 128 k >= 7 and C = 256 exist walked / skewed only (stand-alone
// they lose to three pair launches, see Block3Cfg).
template <class ET, int C, int K, class G> struct Block3Kernels {
    static constexpr int NW = G::WM * G::WN;
    static constexpr bool SKEW = G::WM != 0 && NW == 8 && G::NTW >= 2 &&
                                 (ET::ESZ == 2 || pm_skew_4byte<ET, C>());
    static constexpr bool WALK = G::WM != 0 && NW == 8 && ET::ESZ == 2 &&
                                 !(C == 128 && K == 11) && !(C == 256 && K == 7);
    static constexpr bool TILED = G::WM != 0 && !(C == 128 && K >= 7) && C != 256;
};
// Whole-MRF kernels (C = 32, the k 11 geometry G for all three Blocks): the
// skewed walk for the 4-byte layouts, the walked tiling for the 16-bit ones
// (split f16 walked: 8.4 ms against 7.0 ms for the two-sided tiling - the
// carry areas only fit beside one tile per wave, round 4), the two-sided
// tiling for both.
template <class ET, class G> struct MrfKernels {
    static constexpr int NW = G::WM * G::WN;
    static constexpr bool ANY = G::WM != 0 && Block3Cfg<ET, 32, 3>::WM != 0 &&
                                Block3Cfg<ET, 32, 7>::WM != 0;
    static constexpr bool SKEW = ANY && ET::ESZ == 4 && NW == 8 && G::NTW >= 2;
    static constexpr bool WALK = ANY && ET::ESZ == 2 && NW == 8;
};

// ---- the planner ------------------------------------------------------------
// One MRF stage - or, for pm_block_cl, one Block. Everything but the weights
// and dilations is shared by its Blocks; the first Block stores per `mode`
// (Block3Args::mode), the ones after it add.
struct PmBlock {
    int K;
    const void* w1[PM_MAX_DILATIONS];   // packed weights + bias step
    const void* w2[PM_MAX_DILATIONS];
    int dil[PM_MAX_DILATIONS];
};
struct PmStage {
    int C;                    // padded channels
    const float* x;
    float* out;
    int B, L;
    const int* lengths;       // (B) valid frames per utterance or null
    int len_scale;
    int mode;
    float scale;
    char* scratch;            // device scratch for the skewed walks, or null
    size_t scratch_bytes;
    void* act16;              // the last Block's result as the next
    int act16_type;           // upsampler's operand (Block3Args::act16), or null
    int nblocks, niter;
    PmBlock blk[PM_MAX_RESBLOCKS];
    PM_TIMELINE_FIELD         // debug stamps (tuning builds)
};

enum PmKernel { PM_PAIRS, PM_SKEW, PM_WALK, PM_TILED };
struct PmLaunch {
    PmKernel kernel = PM_PAIRS;   // PM_PAIRS: one pair launch per iteration
    bool narrow = false;          // the latency geometry (Block3CfgNarrow)
    int halo = 0;                 // the tiling's halo columns
    int nseg = 0;                 // segments per utterance (walks)
    bool act16 = false;           // writes PmStage::act16 instead of `out`
};
struct PmPlan {
    bool mrf = false;             // one whole-MRF launch: block[0]
    PmLaunch block[PM_MAX_RESBLOCKS];
};

inline int pm_halo(int K, int niter, const int* dil) {
    int halo = 0;
    for (int i = 0; i < niter; ++i) halo += (dil[i] + 1) * ((K - 1) / 2);
    return halo;
}
// the skewed walk's carries: dilations <= 5 and H2 (d + 1) <= 30
inline bool pm_skew_dilations(int K, int niter, const int* dil) {
    for (int i = 0; i < niter; ++i)
        if (dil[i] < 1 || dil[i] > 5 || ((K - 1) / 2) * (dil[i] + 1) > 30)
            return false;
    return true;
}
// Segments per utterance of a walk: one workgroup per (utterance, segment),
// as many as fill the chip (or the test hook's count); 0: no walk (CU count
// unknown).
inline int pm_walk_segments(int B) {
    if (pm_force().walk_nseg) return pm_force().walk_nseg;
    const int cus = pm_device_cus();
    return cus > 0 ? std::max(1, cus / B) : 0;
}
// The latency geometry (nc_narrow columns instead of nc_wide) where the wide
// tiling gives the chip fewer than PM_NARROW_BELOW workgroups. (A forced walk
// - tests - keeps the 8-wave geometry the walks exist for.)
inline bool pm_take_narrow(int nc_wide, int nc_narrow, int halo, int B, int L) {
    const int TL = nc_wide - 2 * halo, TLn = nc_narrow - 2 * halo;
    return pm_narrow_allowed() && !pm_force().walk_nseg && TL > 0 &&
           TLn >= 32 && (long long)((L + TL - 1) / TL) * B < PM_NARROW_BELOW;
}

template <class ET, int C>
static bool plan_pair_c(int K, int B, int L) {
    typedef PairCfg<ET, C> W;
    typedef PairCfgNarrow<ET, C> N;
    if constexpr ((int)N::NTW != (int)W::NTW || (int)N::WN != (int)W::WN) {
        const int TL = W::WN * W::NTW * 32 - (K - 1);
        return pm_narrow_allowed() &&
               (long long)((L + TL - 1) / TL) * B < PM_NARROW_BELOW;
    }
    return false;
}
// Pair launch (one Block iteration): whether it takes PairCfgNarrow
template <class ET> bool pm_plan_pair(int C, int K, int B, int L) {
    switch (C) {
        case 256: return plan_pair_c<ET, 256>(K, B, L);
        case 128: return plan_pair_c<ET, 128>(K, B, L);
    }
    return false;
}

template <class ET, int C, int K, class G>
static bool plan_block_cfg(const PmStage& s, int j, PmLaunch* l) {
    typedef Block3Kernels<ET, C, K, G> KS;
    if constexpr (G::WM == 0) {
        return false;
    } else {
    constexpr int NC = G::WN * G::NTW * 32;
    const int* dil = s.blk[j].dil;
    l->halo = pm_halo(K, s.niter, dil);
    if (NC - 2 * l->halo < 32) return false;
    const PmForce& f = pm_force();
    const int nseg = pm_walk_segments(s.B);
    if constexpr (KS::SKEW) {
        // Measured at batch 32 x 10 s (profiles/r03/ab_skew.txt): -14 % at C = 128
        // k 11 (against three pair launches), -10 % at C = 128 k 7, -7 % at
        // C = 64 k 11, -1.3 % at C = 64 k 7 (against the walked kernels); where
        // the walked halo is small (k 3: 12 columns) its carries and the
        // hand-over cost 5 % more than the recompute they save, on the
        // 128-column tiles of C = 256 k 7 it is even with three pair launches.
        typedef SkewGeom<ET, C, K, G::WM, G::WN, G::NTW> GE;
        static_assert(GE::SCRATCH <= PM_SKEW_WG_SCRATCH, "scratch bound");
        constexpr bool WINS = ((C == 128 || C == 64) && K >= 7) ||
                              pm_skew_4byte<ET, C>();
        // (for grids that fill the chip several times over)
        if (GE::SMEM <= PM_LDS_BYTES && s.scratch && nseg > 0 &&
            (f.skew > 0 || (f.skew == 0 && WINS)) &&
            pm_skew_dilations(K, s.niter, dil) &&
            (f.walk_nseg || (s.L / NC) / nseg >= 4) &&
            (size_t)s.B * nseg * GE::SCRATCH <= s.scratch_bytes) {
            l->kernel = PM_SKEW;
            l->nseg = nseg;
            l->act16 = s.act16 && j == s.nblocks - 1;
            return true;
        }
    }
    if constexpr (KS::WALK) {
        const int smem = block3_walk_smem_bytes<ET, C, K, G::WM, G::WN, G::NTW>() +
                         block3_carry_bytes<ET, C>(l->halo);
        if (smem <= PM_LDS_BYTES && nseg > 0 &&
            (f.walk_nseg || (s.L / (NC - l->halo)) / nseg >= 6)) {
            l->kernel = PM_WALK;
            l->nseg = nseg;
            return true;
        }
    }
    if constexpr (KS::TILED) {
        l->kernel = PM_TILED;
        return true;
    }
    return false;
    }
}

template <class ET, int C, int K>
static PmLaunch plan_block_ck(const PmStage& s, int j) {
    typedef Block3Cfg<ET, C, K> W;
    typedef Block3CfgNarrow<ET, C, K> N;
    PmLaunch l;
    if constexpr ((int)W::WM != 0 && (int)N::WN != (int)W::WN) {
        if (pm_take_narrow(W::WN * W::NTW * 32, N::WN * N::NTW * 32,
                           pm_halo(K, s.niter, s.blk[j].dil), s.B, s.L)) {
            l.narrow = true;
            return plan_block_cfg<ET, C, K, N>(s, j, &l) ? l : PmLaunch();
        }
    }
    return plan_block_cfg<ET, C, K, W>(s, j, &l) ? l : PmLaunch();
}

// Block j of the stage: a whole-Block launch, or PM_PAIRS where no whole-Block
// kernel takes the shape
template <class ET> PmLaunch pm_plan_block(const PmStage& s, int j) {
    if (s.niter < 1 || s.niter > 3) return PmLaunch();
    for (int i = 0; i < s.niter; ++i)
        if (s.blk[j].dil[i] < 1 || s.blk[j].dil[i] > 5) return PmLaunch();
    const int K = s.blk[j].K;
#define PM_PLAN_C(C_)                                                        \
    case C_:                                                                 \
        if (K == 3) return plan_block_ck<ET, C_, 3>(s, j);                   \
        if (K == 7) return plan_block_ck<ET, C_, 7>(s, j);                   \
        if (K == 11) return plan_block_ck<ET, C_, 11>(s, j);                 \
        break;
    switch (s.C) { PM_PLAN_C(32) PM_PLAN_C(64) PM_PLAN_C(128) PM_PLAN_C(256) }
#undef PM_PLAN_C
    return PmLaunch();
}

template <class ET, class G>
static bool plan_mrf_cfg(const PmStage& s, bool blocks_ok, PmLaunch* l) {
    typedef MrfKernels<ET, G> KS;
    if constexpr (!KS::ANY) {
        return false;
    } else {
    constexpr int NC = G::WN * G::NTW * 32;
    constexpr int KS3[3] = {3, 7, 11};
    l->halo = 0;
    for (int j = 0; j < 3; ++j)
        l->halo = std::max(l->halo, pm_halo(KS3[j], s.niter, s.blk[j].dil));
    if (NC - 2 * l->halo < 32) return false;
    const PmForce& f = pm_force();
    const int nseg = pm_walk_segments(s.B);
    if constexpr (KS::SKEW) {
        typedef MrfSkewGeom<ET, 32, G::WM, G::WN, G::NTW> MG;
        static_assert(MG::SCRATCH <= PM_SKEW_WG_SCRATCH, "scratch bound");
        bool fits = MG::SMEM <= PM_LDS_BYTES && s.scratch && nseg > 0 &&
                    f.skew >= 0 && s.niter == 3;
        for (int j = 0; j < 3; ++j)
            fits = fits && pm_skew_dilations(KS3[j], 3, s.blk[j].dil);
        if (fits && (f.walk_nseg || (s.L / NC) / nseg >= 4) &&
            (size_t)s.B * nseg * MG::SCRATCH <= s.scratch_bytes) {
            l->kernel = PM_SKEW;
            l->nseg = nseg;
            return true;
        }
        // A batch long enough for the skewed walk never takes the two-sided
        // tiling below (pm_skew_4byte): Block by Block instead - unless the
        // test hook has switched the skewed walk off altogether, which makes
        // the tiling, whose sum order is the skewed whole-MRF walk's, the
        // stand-alone counterpart the tests compare bit for bit.
        const int cus = pm_device_cus();
        if (blocks_ok && f.skew >= 0 && s.scratch && cus > 0 &&
            (s.L / NC) / std::max(1, cus / s.B) >= 4)
            return false;
    }
    if constexpr (KS::WALK) {
        // (enough tiles per segment to amortise its two-sided first tile)
        if (nseg > 0 && s.niter == 3 &&
            (f.walk_nseg || (s.L / (NC - l->halo)) / nseg >= 8)) {
            l->kernel = PM_WALK;
            l->nseg = nseg;
            return true;
        }
    }
    l->kernel = PM_TILED;
    return true;
    }
}

// The whole stage (Blocks k = 3, 7, 11) in one launch - C = 32 only: C = 64
// has no registers left for the sum (trunk + accumulator are 128 VGPRs), its
// whole-MRF variant read-modify-writes `out` through L2, the lines do not
// survive there (rocprof: 2.6 GB written per launch instead of 0.9) and it
// only ties with three Block launches. blocks_ok: the caller can run the
// stage Block by Block instead. False: no whole-MRF launch.
template <class ET> bool pm_plan_mrf(const PmStage& s, bool blocks_ok, PmLaunch* l) {
    *l = PmLaunch();
    if (s.C != 32 || s.nblocks != 3 || s.niter < 1 || s.niter > 3 ||
        s.blk[0].K != 3 || s.blk[1].K != 7 || s.blk[2].K != 11)
        return false;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < s.niter; ++i)
            if (s.blk[j].dil[i] < 1 || s.blk[j].dil[i] > 5) return false;
    typedef Block3Cfg<ET, 32, 11> W;
    typedef Block3CfgNarrow<ET, 32, 11> N;
    if constexpr ((int)W::WM != 0 && (int)N::WN != (int)W::WN) {
        if (pm_take_narrow(W::WN * W::NTW * 32, N::WN * N::NTW * 32,
                           pm_halo(11, s.niter, s.blk[2].dil), s.B, s.L)) {
            l->narrow = true;
            return plan_mrf_cfg<ET, N>(s, blocks_ok, l);
        }
    }
    return plan_mrf_cfg<ET, W>(s, blocks_ok, l);
}

// The stage at fusion level `fusion` (pm_fusion_level)
template <class ET> PmPlan pm_plan_stage(const PmStage& s, int fusion) {
    PmPlan p;
    if (fusion >= 2 && pm_plan_mrf<ET>(s, true, &p.block[0])) {
        p.mrf = true;
        return p;
    }
    for (int j = 0; j < s.nblocks; ++j)
        p.block[j] = fusion >= 1 ? pm_plan_block<ET>(s, j) : PmLaunch();
    return p;
}

// ---- launchers --------------------------------------------------------------
template <class ET> hipError_t pm_launch_pair(
    int C, int K, bool narrow, const PairArgs& args, hipStream_t stream);
// Block j of the stage as planned (not PM_PAIRS)
template <class ET> hipError_t pm_launch_block3(
    const PmLaunch& plan, const PmStage& s, int j, hipStream_t stream);
// The stage as one whole-MRF launch, as planned
template <class ET> hipError_t pm_launch_mrf(
    const PmLaunch& plan, const PmStage& s, hipStream_t stream);

// kind 0: plain conv with KT = KSPAN = 7 (input conv); kind 1: polyphase
// ConvTranspose (KT = 2, KSPAN = 3). cfg: 0 = 256 x 128 tile, 1 = 64 x 128,
// 3 = 128 x 128 (measured: a 512 x 128 tile is 20 % slower than cfg 0),
// 2 = 32 x 128.
template <class ET> hipError_t pm_launch_single(
    int kind, int ch, int cfg, const SingleArgs& args, hipStream_t stream);
hipError_t pm_launch_stft(int epi, const SingleArgs& args, hipStream_t stream);

#ifdef PM_INSTANTIATE

template <class Kern, class Args>
static hipError_t launch_with_lds(Kern kern, int grid, int threads, int smem,
                                  hipStream_t stream, const Args& args) {
    hipError_t e = pm_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), smem, stream, args);
    return hipGetLastError();
}

template <class ET, int C, int K, class G>
static hipError_t launch_pair_cfg(const PairArgs& a0, hipStream_t stream) {
    constexpr int WM = G::WM, WN = G::WN, NTW = G::NTW, CH = G::CH;
    constexpr int ALIAS = G::ALIAS;
    constexpr int TL = WN * NTW * 32 - (K - 1);
    PairArgs a = a0;
    a.ntiles = (a.L + TL - 1) / TL;
    return launch_with_lds(
        conv_pair_kernel<ET, C, K, WM, WN, NTW, CH, ALIAS>, a.ntiles * a.B,
        WM * WN * 64,
        pair_smem_bytes<ET, C, K, WM, WN, NTW, CH, ALIAS>(a.dilation), stream, a);
}

template <class ET, int C>
static hipError_t launch_pair_c(int K, bool narrow, const PairArgs& a, hipStream_t s) {
    typedef PairCfg<ET, C> W;
    typedef PairCfgNarrow<ET, C> N;
    switch (K) {
        case 3: return narrow ? launch_pair_cfg<ET, C, 3, N>(a, s) : launch_pair_cfg<ET, C, 3, W>(a, s);
        case 7: return narrow ? launch_pair_cfg<ET, C, 7, N>(a, s) : launch_pair_cfg<ET, C, 7, W>(a, s);
        case 11: return narrow ? launch_pair_cfg<ET, C, 11, N>(a, s) : launch_pair_cfg<ET, C, 11, W>(a, s);
    }
    return hipErrorInvalidValue;
}

template <class ET>
hipError_t pm_launch_pair(int C, int K, bool narrow, const PairArgs& a, hipStream_t s) {
    switch (C) {
        case 256: return launch_pair_c<ET, 256>(K, narrow, a, s);
        case 128: return launch_pair_c<ET, 128>(K, narrow, a, s);
        case 64: return launch_pair_c<ET, 64>(K, narrow, a, s);
        case 32: return launch_pair_c<ET, 32>(K, narrow, a, s);
    }
    return hipErrorInvalidValue;
}

// Block j's arguments, tiled with `halo` columns on NC-column tiles
static Block3Args block3_args(const PmStage& s, int j, int NC, int halo) {
    Block3Args a = {};
    a.x = s.x; a.out = s.out; a.niter = s.niter;
    for (int n = 0; n < s.niter; ++n) {
        a.w1[n] = s.blk[j].w1[n];
        a.w2[n] = s.blk[j].w2[n];
        a.dil[n] = s.blk[j].dil[n];
    }
    a.B = s.B; a.L = s.L; a.mode = j == 0 ? s.mode : 2; a.scale = s.scale;
    a.halo = halo; a.TL = NC - 2 * halo; a.ntiles = (s.L + a.TL - 1) / a.TL;
    a.lengths = s.lengths; a.len_scale = s.len_scale;
#ifdef PM_TUNING
    a.timeline = s.timeline;
#endif
    return a;
}

template <class ET, int C, int K, class G>
static hipError_t launch_block3_cfg(const PmLaunch& l, const PmStage& s, int j,
                                    hipStream_t stream) {
    typedef Block3Kernels<ET, C, K, G> KS;
    constexpr int WM = G::WM, WN = G::WN, NTW = G::NTW, NT = WM * WN * 64;
    Block3Args a = block3_args(s, j, WN * NTW * 32, l.halo);
    if constexpr (KS::SKEW) if (l.kernel == PM_SKEW) {
        typedef SkewGeom<ET, C, K, WM, WN, NTW> GE;
        if (l.act16) { a.act16 = s.act16; a.act16_type = s.act16_type; }
        Block3SkewArgs p;
        p.a = a; p.nseg = l.nseg; p.wg_scratch = GE::SCRATCH;
        p.scratch = s.scratch;
        return launch_with_lds(conv_block3_skew_kernel<ET, C, K, WM, WN, NTW>,
                               a.B * l.nseg, NT, GE::SMEM, stream, p);
    }
    if constexpr (KS::WALK) if (l.kernel == PM_WALK) {
        Block3WalkArgs p;
        p.a = a; p.nseg = l.nseg;
        return launch_with_lds(
            conv_block3_walk_kernel<ET, C, K, WM, WN, NTW>, a.B * l.nseg, NT,
            block3_walk_smem_bytes<ET, C, K, WM, WN, NTW>() +
                block3_carry_bytes<ET, C>(a.halo),
            stream, p);
    }
    if constexpr (KS::TILED) if (l.kernel == PM_TILED)
        return launch_with_lds(conv_block3_kernel<ET, C, K, WM, WN, NTW>,
                               a.ntiles * a.B, NT,
                               block3_smem_bytes<ET, C, K, WM, WN, NTW>(), stream, a);
    return hipErrorInvalidValue;
}

template <class ET, int C, int K>
static hipError_t launch_block3_ck(const PmLaunch& l, const PmStage& s, int j,
                                   hipStream_t stream) {
    return l.narrow
        ? launch_block3_cfg<ET, C, K, Block3CfgNarrow<ET, C, K>>(l, s, j, stream)
        : launch_block3_cfg<ET, C, K, Block3Cfg<ET, C, K>>(l, s, j, stream);
}

template <class ET>
hipError_t pm_launch_block3(const PmLaunch& l, const PmStage& s, int j,
                            hipStream_t stream) {
    const int K = s.blk[j].K;
#define PM_LAUNCH_C(C_)                                                      \
    case C_:                                                                 \
        if (K == 3) return launch_block3_ck<ET, C_, 3>(l, s, j, stream);     \
        if (K == 7) return launch_block3_ck<ET, C_, 7>(l, s, j, stream);     \
        if (K == 11) return launch_block3_ck<ET, C_, 11>(l, s, j, stream);   \
        break;
    switch (s.C) { PM_LAUNCH_C(32) PM_LAUNCH_C(64) PM_LAUNCH_C(128) PM_LAUNCH_C(256) }
#undef PM_LAUNCH_C
    return hipErrorInvalidValue;
}

// What the skewed and the walked whole-MRF arguments share
template <class A>
static void mrf_walk_args(A& p, const PmStage& s, const PmLaunch& l) {
    p.x = s.x; p.out = s.out;
    for (int j = 0; j < 3; ++j)
        for (int n = 0; n < 3; ++n) {
            p.w1[j][n] = s.blk[j].w1[n];
            p.w2[j][n] = s.blk[j].w2[n];
            p.dil[j][n] = s.blk[j].dil[n];
        }
    p.B = s.B; p.L = s.L; p.halo = l.halo; p.scale = s.scale;
    p.lengths = s.lengths; p.len_scale = s.len_scale;
    p.nseg = l.nseg;
}

template <class ET, class G>
static hipError_t launch_mrf_cfg(const PmLaunch& l, const PmStage& s,
                                 hipStream_t stream) {
    typedef MrfKernels<ET, G> KS;
    constexpr int C = 32, WM = G::WM, WN = G::WN, NTW = G::NTW;
    constexpr int NT = WM * WN * 64;
    if constexpr (KS::SKEW) if (l.kernel == PM_SKEW) {
        typedef MrfSkewGeom<ET, C, WM, WN, NTW> MG;
        MrfSkewArgs p = {};
        mrf_walk_args(p, s, l);
        p.wg_scratch = MG::SCRATCH;
        p.scratch = s.scratch;
#ifdef PM_TUNING
        p.timeline = s.timeline;
#endif
        return launch_with_lds(conv_mrf_skew_kernel<ET, C, WM, WN, NTW>,
                               s.B * l.nseg, NT, MG::SMEM, stream, p);
    }
    if constexpr (KS::WALK) if (l.kernel == PM_WALK) {
        MrfWalkArgs p = {};
        mrf_walk_args(p, s, l);
        return launch_with_lds(
            conv_mrf_walk_kernel<ET, C, WM, WN, NTW>, s.B * l.nseg, NT,
            block3_walk_smem_bytes<ET, C, 11, WM, WN, NTW>() +
                3 * block3_carry_bytes<ET, C>(l.halo),
            stream, p);
    }
    if constexpr (KS::ANY) if (l.kernel == PM_TILED) {
        MrfArgs m;
        for (int j = 0; j < 3; ++j) {
            m.k[j] = block3_args(s, j, WN * NTW * 32, l.halo);
#ifdef PM_TUNING
            m.k[j].timeline = nullptr;
#endif
        }
        return launch_with_lds(conv_mrf_kernel<ET, C, WM, WN, NTW, true>,
                               m.k[0].ntiles * s.B, NT,
                               block3_smem_bytes<ET, C, 11, WM, WN, NTW>(), stream, m);
    }
    return hipErrorInvalidValue;
}

template <class ET>
hipError_t pm_launch_mrf(const PmLaunch& l, const PmStage& s, hipStream_t stream) {
    if (s.C != 32) return hipErrorInvalidValue;
    return l.narrow
        ? launch_mrf_cfg<ET, Block3CfgNarrow<ET, 32, 11>>(l, s, stream)
        : launch_mrf_cfg<ET, Block3Cfg<ET, 32, 11>>(l, s, stream);
}

// ---- single conv ----------------------------------------------------------
template <class ET, int KT, int KSPAN, int CH, int WM, int WN, int MTW, int NTW,
          int EPI = 0>
static hipError_t launch_single_cfg(const SingleArgs& a0, hipStream_t stream) {
    constexpr int N1 = WN * NTW * 32;
    constexpr int MB = WM * MTW * 32;
    SingleArgs a = a0;
    a.ntiles = (a.Lout + N1 - 1) / N1;
    a.nmblocks = a.M / MB;
    auto kern = conv_single_kernel<ET, KT, KSPAN, CH, WM, WN, MTW, NTW, EPI>;
    constexpr int smem = 2 * (N1 + KSPAN - 1) * (CH * ET::ESZ + 16);
    if (smem > 48 * 1024) {
        hipError_t e = pm_ensure_dynamic_lds(
            reinterpret_cast<const void*>(kern), smem);
        if (e != hipSuccess) return e;
    }
    const int grid = a.ntiles * a.nmblocks * a.B;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WM * WN * 64), smem, stream, a);
    return hipGetLastError();
}

template <class ET, int KT, int KSPAN>
static hipError_t launch_single_k(
    int ch, int cfg, const SingleArgs& a, hipStream_t s) {
    if (ch == 64) {
        switch (cfg) {
            case 0: return launch_single_cfg<ET, KT, KSPAN, 64, 4, 2, 2, 2>(a, s);
            case 1: return launch_single_cfg<ET, KT, KSPAN, 64, 2, 2, 1, 2>(a, s);
            case 2: return launch_single_cfg<ET, KT, KSPAN, 64, 1, 4, 1, 1>(a, s);
            // all 128 rows of a 2x upsampler in one workgroup: x is read once
            case 3: return launch_single_cfg<ET, KT, KSPAN, 64, 4, 2, 1, 2>(a, s);
            // the C_in = 128 r = 2 upsampler on long batches: 256 input columns
            // a workgroup instead of 128 - half as many workgroups, a weight
            // fragment feeds four MFMAs instead of two: 0.364 -> 0.342 ms (the
            // same widening of cfg 1 for C_in = 64 measured neutral and is not
            // kept: profiles/r05/ab_wide_upsampler.txt)
            case 5:
                if constexpr (KT == 2)
                    return launch_single_cfg<ET, KT, KSPAN, 64, 4, 2, 1, 4>(a, s);
                break;
        }
    } else if (ch == 32) {
        switch (cfg) {
            case 1: return launch_single_cfg<ET, KT, KSPAN, 32, 2, 2, 1, 2>(a, s);
            case 2: return launch_single_cfg<ET, KT, KSPAN, 32, 1, 4, 1, 1>(a, s);
        }
    }
    return hipErrorInvalidValue;
}

// cfg 4: the wide upsampler with the whole K staged once (ch = C_in = 256 /
// 512, 16-bit operands, weights packed as one chunk)
template <class ET, int CIN>
static hipError_t launch_upsample_cfg(const SingleArgs& a0, hipStream_t stream) {
    if constexpr (ET::ESZ != 2) {
        return hipErrorNotSupported;
    } else {
    constexpr int WM = 4, WN = 2, MTW = 2, NTW = 2;
    constexpr int N1 = WN * NTW * 32, MB = WM * MTW * 32;
    SingleArgs a = a0;
    if (a.Cin != CIN || a.M % MB) return hipErrorInvalidValue;
    a.ntiles = (a.Lout + N1 - 1) / N1;
    // M groups per column tile: as few as still give the chip ~2 workgroups
    // per CU (every group stages the x tile again)
    const int mblocks = a.M / MB;
    int groups = 1;
    while (groups < mblocks && (long long)a.ntiles * a.B * groups < 512)
        groups *= 2;
    if (pm_force().upsample_groups > 0) groups = pm_force().upsample_groups;
    if (groups > mblocks) groups = mblocks;
    while (mblocks % groups) groups /= 2;
    a.nmblocks = groups;
    constexpr int xtile = (N1 + 2) * (CIN * ET::ESZ + 16);
    const dim3 grid(a.ntiles * a.nmblocks * a.B), block(WM * WN * 64);
    // Row stores (conv_upsample_kernel, ROWS > 0): every wave turns its
    // tiles round in LDS behind the x tile, 32 columns at a time (8 KB a
    // wave) where there is room - C_in = 256: 67 + 64 of 160 KB - and 8
    // columns (2 KB) at C_in = 512 (132 + 16 KB). A forced group count keeps
    // the direct stores, so that both stay under test.
    // Measured, bf16, batch 32 x 10 s (profiles/upsample_store/NOTES.md):
    // direct stores 0.359 ms (C_in 256) / 0.161 ms (512); row stores 0.298 /
    // 0.141, with half the write requests from the CUs to the L2; row stores
    // non-temporal (shipped) 0.276 / 0.137. Staging x for fewer groups at
    // C_in = 512 (2 instead of 4) measured neutral, 0.142, and is not kept.
    // Row stores with a workgroup barrier (whole 1 KB runs of a row) were
    // not built: the 256-byte runs already make every request a whole line.
    // (-DPM_UPSAMPLE_ROWS=0: the A/B build with direct stores)
    constexpr int CP =
        xtile + WM * WN * RowStores<MTW, 32>::WAVE <= PM_LDS_BYTES ? 32 : 8;
    if constexpr (PM_UPSAMPLE_ROWS &&
                  xtile + WM * WN * RowStores<MTW, CP>::WAVE <= PM_LDS_BYTES) {
        if (pm_force().upsample_groups == 0) {
            auto rows = conv_upsample_kernel<ET, CIN, WM, WN, MTW, NTW, CP>;
            constexpr int smem = xtile + WM * WN * RowStores<MTW, CP>::WAVE;
            hipError_t e = pm_ensure_dynamic_lds(
                reinterpret_cast<const void*>(rows), smem);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(rows, grid, block, smem, stream, a);
            return hipGetLastError();
        }
    }
    auto kern = conv_upsample_kernel<ET, CIN, WM, WN, MTW, NTW>;
    hipError_t e = pm_ensure_dynamic_lds(
        reinterpret_cast<const void*>(kern), xtile);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, xtile, stream, a);
    return hipGetLastError();
    }
}

template <class ET>
hipError_t pm_launch_single(
    int kind, int ch, int cfg, const SingleArgs& a, hipStream_t s) {
    if (kind == 1 && cfg == 4) {
        if (ch == 256) return launch_upsample_cfg<ET, 256>(a, s);
        if (ch == 512) return launch_upsample_cfg<ET, 512>(a, s);
        return hipErrorInvalidValue;
    }
    if (kind == 0) return launch_single_k<ET, 7, 7>(ch, cfg, a, s);
    if (kind == 1) return launch_single_k<ET, 2, 3>(ch, cfg, a, s);
    return hipErrorInvalidValue;
}

// Framed DFT (STFT) as a 4-tap conv over the hop-reshaped padded audio:
// exact-fp32 MFMA only (the forward transforms run as FFTs, pm_fft.h; this is
// the backward and the brute-force cross-check). epi 1: magnitude, 3: the DFT
// cotangent grad / magnitude * (re, im) (backward, first half), 0: the
// overlap-add conv of that cotangent against the transposed basis (backward,
// second half: C_in = 1088 -> 256 samples of one hop, 4 taps).
#ifdef PM_INSTANTIATE_STFT
hipError_t pm_launch_stft(int epi, const SingleArgs& a, hipStream_t s) {
    if (epi == 1)
        return launch_single_cfg<ElemF32, 4, 4, 64, 2, 2, 1, 2, 1>(a, s);
    if (epi == 3)
        return launch_single_cfg<ElemF32, 4, 4, 64, 2, 2, 1, 2, 3>(a, s);
    if (epi == 0)
        return launch_single_cfg<ElemF32, 4, 4, 64, 2, 2, 1, 2, 0>(a, s);
    return hipErrorInvalidValue;
}
#endif

#endif  // PM_INSTANTIATE

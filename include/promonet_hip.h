/* promonet_hip.h - C ABI of libpromonet_hip.so
 *
 * MI355X (gfx950 / CDNA4) implementation of promonet's synthesis hot path.
 * The reference (maxrmorrison/promonet @ 2024_08_07) is 100 % Python on
 * PyTorch and has NO FFI / plugin interface of its own; the seams this
 * library attaches to are Python module methods. Each entry point cites the
 * reference code it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - C linkage, plain pointers and sizes, no torch types.
 *   - Every pointer named *dev* / every tensor argument is a DEVICE pointer
 *     owned by the caller (e.g. torch.Tensor.data_ptr()); never mutated
 *     unless documented as an output.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream). All
 *     compute entry points are asynchronous on that stream.
 *   - Return value: PM_OK (0) or a negative PM_E* code; pm_last_error()
 *     returns a thread-local human-readable message for the last failure.
 *   - No allocation inside the forward path: the caller passes a workspace
 *     whose size comes from pm_hifigan_workspace_bytes(). Weight storage is
 *     allocated at load time (pm_hifigan_load_tensor / pm_hifigan_finalize).
 *   - fp32 tensors are dense row-major in the reference's (PyTorch) layout:
 *     activations (B, C, T), conv weights (C_out, C_in, k), transposed-conv
 *     weights (C_in, C_out, k). Arguments suffixed `_cl` are the library's
 *     internal channels-last layout (B, T, C_pad), C_pad = round_up(C, 32).
 */
#ifndef PROMONET_HIP_H
#define PROMONET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_EINVAL (-1)      /* bad argument / unsupported configuration */
#define PM_ESTATE (-2)      /* call order (e.g. forward before finalize)  */
#define PM_EHIP (-3)        /* a HIP runtime call failed                   */
#define PM_ENOMEM (-4)      /* workspace too small / allocation failed     */
#define PM_ETIMEOUT (-5)    /* a bounded inter-workgroup wait gave up      */

/* MFMA operand type (accumulation is always fp32; activations between
 * kernels are always fp32 in HBM) */
#define PM_F32 0            /* v_mfma_f32_32x32x2_f32   - exact fp32       */
#define PM_F16 1            /* v_mfma_f32_32x32x16_f16                     */
#define PM_BF16 2           /* v_mfma_f32_32x32x16_bf16                    */
#define PM_F16X3 3          /* f16 operands split hi + lo, three MFMAs per
                             * step: ~21 bits per factor (trained-scale
                             * accuracy for the last stage)  */
#define PM_F16A2 4          /* f16 operands, the ACTIVATIONS split hi + lo
                             * (two MFMAs per step, f16 weight stream). As
                             * the type of a STAGE: its Blocks; the stage's
                             * upsampler - one rounding of a wide sum - runs
                             * PM_F16X3                                    */
#define PM_F16UX 5          /* stage / engine type only: f16 Blocks behind a
                             * PM_F16X3 upsampler                          */

#define PM_MAX_STAGES 8
#define PM_MAX_RESBLOCKS 4
#define PM_MAX_DILATIONS 4

typedef struct pm_hifigan_s* pm_hifigan_t;

/* Mirrors the constants the reference reads at import time:
 * promonet/config/defaults.py:216,250-262 and config/static.py:42-53.   */
typedef struct pm_hifigan_config {
    int num_features;                 /* NUM_FEATURES (113)                */
    int global_channels;              /* GLOBAL_CHANNELS (258)             */
    int initial_channels;             /* HIFIGAN_UPSAMPLE_INITIAL_SIZE     */
    int num_stages;                   /* len(HIFIGAN_UPSAMPLE_RATES)       */
    int upsample_rates[PM_MAX_STAGES];
    int upsample_kernel_sizes[PM_MAX_STAGES];
    int num_resblocks;                /* len(HIFIGAN_RESBLOCK_KERNEL_SIZES)*/
    int resblock_kernel_sizes[PM_MAX_RESBLOCKS];
    int num_dilations;
    int resblock_dilations[PM_MAX_RESBLOCKS][PM_MAX_DILATIONS];
    int compute_dtype;                /* PM_F32 ... PM_F16UX                 */
    /* Per-stage override of the MFMA operand type (upsampler + MRF of stage
     * i): 0 = compute_dtype, else 1 + PM_F32 ... PM_F16UX. E.g. bf16
     * for the wide stages and f16 for the last two, whose rounding reaches
     * the output most directly.                                           */
    int stage_compute_dtype[PM_MAX_STAGES];
} pm_hifigan_config;

int pm_version(void);
const char* pm_last_error(void);

/* ---- HiFi-GAN vocoder engine: replaces promonet.model.HiFiGAN ----------
 * (promonet/model/hifigan.py:13-77; constructed at generator.py:22-25)   */
int pm_hifigan_create(const pm_hifigan_config* config, pm_hifigan_t* out);
int pm_hifigan_destroy(pm_hifigan_t h);

/* Load one tensor of HiFiGAN.state_dict() by its reference key, e.g.
 *   input_feature_conv.weight (512,113,7)   input_speaker_conv.bias (512)
 *   model.0.model.1.weight_g (512,1,1)      model.0.model.1.weight_v (512,256,16)
 *   model.0.model.2.model.1.convs2.0.bias   model.5.weight (1,32,7)
 * Weight-normed layers accept either the (weight_g, weight_v) pair of the
 * checkpoint (folded here: w = g v / ||v||, replacing the per-forward
 * torch.nn.utils.weight_norm hook of model/core.py:43-45) or an already
 * folded `.weight`. Replaces torchutil.checkpoint.load -> load_state_dict
 * at promonet/synthesize/core.py:245. Synchronous w.r.t. `stream`.       */
int pm_hifigan_load_tensor(pm_hifigan_t h, const char* name,
                           const float* dev, const int64_t* shape, int ndim,
                           void* stream);
/* Verify every tensor is present; must precede forward.                  */
int pm_hifigan_finalize(pm_hifigan_t h, void* stream);

size_t pm_hifigan_workspace_bytes(pm_hifigan_t h, int batch, int frames);
int pm_hifigan_hopsize(pm_hifigan_t h);
int pm_hifigan_features_cl_channels(pm_hifigan_t h);

/* HiFiGAN.forward(x, g, p) (hifigan.py:63-70):
 *   features (B, num_features, T) fp32, global_features (Bg, global_channels)
 *   with Bg == 1 (broadcast) or B; out (B, 1, T * hop) fp32.              */
int pm_hifigan_forward(pm_hifigan_t h, const float* features,
                       const float* global_features, int global_batch,
                       float* out, int batch, int frames, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Same with the features already channels-last (B, T, C_pad) - what
 * pm_prepare_features writes.                                             */
int pm_hifigan_forward_cl(pm_hifigan_t h, const float* features_cl,
                          const float* global_features, int global_batch,
                          float* out, int batch, int frames, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Ragged batch (no reference counterpart: the reference synthesises one
 * utterance per call, synthesize/core.py:158-201): lengths (B) int32 device
 * array of valid frames <= frames; frames past an utterance's end are never
 * read, so each utterance equals its stand-alone synthesis; the output tail
 * is zero. features_cl != 0: features are channels-last (B, T, C_pad).     */
int pm_hifigan_forward_ragged(pm_hifigan_t h, const float* features,
                              int features_cl, const float* global_features,
                              int global_batch, const int* lengths,
                              float* out, int batch, int frames,
                              void* workspace, size_t workspace_bytes,
                              void* stream);

/* Streaming by overlap-save (no reference counterpart: the reference
 * synthesises whole utterances, and its packed_inference, generator.py:
 * 313-343, treats every chunk as one). The generator is convolutional: the
 * audio of a frame depends on `left` frames before it and `right` frames
 * after it, derived from the configuration by interval arithmetic - (13, 13)
 * at the defaults.                                                         */
int pm_hifigan_context(pm_hifigan_t h, int* left, int* right);
/* One streaming step, on `stream`, without allocation or host sync:
 *   next_window (B, keep + chunk_frames, C_pad) = [the last `keep` frames of
 *   prev_window (B, prev_frames, C_pad) | chunk], where chunk is (B,
 *   chunk_frames, C_pad) with chunk_cl != 0 and (B, num_features,
 *   chunk_frames) otherwise; next_window must alias neither input (the caller
 *   swaps two buffers). Then, unless emit_frames == 0, the forward of
 *   pm_hifigan_forward_cl on next_window, and
 *   out (B, 1, emit_frames * hop) = its audio from frame emit_first on.
 * The caller's schedule chooses keep <= min(prev_frames, left + right) and
 * the emitted frames, inside the window, so that every emitted frame has its
 * context in the window or lies that close to a true end of the utterance;
 * the concatenated output then equals one forward over the concatenated
 * chunks bit for bit. chunk_frames == 0 closes a stream: the window is the
 * history alone. prev_window may be NULL with keep == 0, chunk with
 * chunk_frames == 0; global_features, out and workspace with emit_frames == 0.
 * workspace: pm_hifigan_stream_workspace_bytes(h, batch, keep + chunk_frames). */
int pm_hifigan_stream(pm_hifigan_t h, const float* chunk, int chunk_cl,
                      int chunk_frames, const float* prev_window,
                      int prev_frames, int keep, float* next_window,
                      const float* global_features, int global_batch,
                      int emit_first, int emit_frames, float* out, int batch,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t pm_hifigan_stream_workspace_bytes(pm_hifigan_t h, int batch,
                                         int window_frames);

/* Optional per-launch timing (HIP events recorded on `stream` around every
 * kernel the forward launches; no reference counterpart - the reference only
 * has wall-clock torchutil timers, synthesize/core.py:222,250). collect()
 * synchronises and folds the recorded pairs into per-label totals; report()
 * returns "label launches total_ms algorithmic_flops algorithmic_bytes" lines.
 * profile_only(label) restricts the events to that label's launches (NULL or
 * "": every launch), so that a timed region pays for two events per step.  */
int pm_hifigan_profile_enable(pm_hifigan_t h, int enable);
int pm_hifigan_profile_only(pm_hifigan_t h, const char* label);
int pm_hifigan_profile_collect(pm_hifigan_t h);
int pm_hifigan_profile_reset(pm_hifigan_t h);
const char* pm_hifigan_profile_report(pm_hifigan_t h);

/* ---- conditioning: replaces Generator.prepare_features ------------------
 * (promonet/model/generator.py:137-197) incl. the third-party ppgs.sparsify
 * it calls (:140-147).
 *   loudness (B, F, T) dB with F == bands or any F >= bands (513)
 *   pitch (B, T) Hz, periodicity (B, T), ppg (B, P, T)
 *   pitch_edges (NB) = Generator.pitch_distribution, pitch_table (NB, E)
 *   out_ref (B, P+E+bands+1, T) and/or out_cl (B, T, C_pad); either may be
 *   NULL. period_rate > 0 appends the channel period_rate / clip(hz), the
 *   pitch period in samples FARGAN reads (generator.py:191-195).
 *   sparse_method = promonet.SPARSE_PPG_METHOD: PM_SPARSE_NONE (ppg passed
 *   through), _PERCENTILE (ppg_threshold = quantile in [0, 1], the default
 *   0.85), _CONSTANT (ppg_threshold = the cut itself), _TOPK (ppg_threshold
 *   = k, the number of entries kept per frame).                            */
#define PM_SPARSE_NONE 0
#define PM_SPARSE_PERCENTILE 1
#define PM_SPARSE_CONSTANT 2
#define PM_SPARSE_TOPK 3
int pm_prepare_features(const float* loudness, const float* pitch,
                        const float* periodicity, const float* ppg,
                        const float* pitch_edges, const float* pitch_table,
                        float* out_ref, float* out_cl, int batch, int frames,
                        int loudness_rows, int ppg_channels, int pitch_bins,
                        int embedding_size, int bands, int cl_channels,
                        int sparse_method, float ppg_threshold, float fmin,
                        float fmax, float min_db, float ref_db,
                        float period_rate, void* stream);

/* BaseGenerator.prepare_global_features (generator.py:49-70): speaker
 * embedding lookup + the augmentation ratios -> (B, S + 2). Either ratio
 * pointer may be NULL (AUGMENT_PITCH / AUGMENT_LOUDNESS off: the row is
 * narrower). speaker_table is (num_speakers, S); an id outside
 * [0, num_speakers) reads nothing and produces a NaN row.                 */
int pm_prepare_global_features(const int64_t* speakers,
                               const float* spectral_balance_ratios,
                               const float* loudness_ratios,
                               const float* speaker_table, float* out,
                               int batch, int speaker_channels,
                               int num_speakers, void* stream);
/* ZERO_SHOT variant (generator.py:35-38, synthesize/core.py:253-254): the
 * speaker is a (B, E) x-vector, the embedding a Linear(E -> S) with weight
 * (S, E) and bias (S).                                                     */
int pm_prepare_global_features_linear(const float* speaker_embeddings,
                                      const float* weight, const float* bias,
                                      const float* spectral_balance_ratios,
                                      const float* loudness_ratios,
                                      float* out, int batch,
                                      int embedding_channels,
                                      int speaker_channels, void* stream);

/* ---- per-kernel entry points (unit parity tests; weights in torch layout,
 * packed into `workspace` on every call) --------------------------------- */
size_t pm_op_workspace_bytes(int c_in, int c_out, int k);
/* One Block iteration (hifigan.py:204-210), channels-last fp32 in/out:
 *   y = x + conv2(lrelu(conv1(lrelu(x)))); mode 0: out = y,
 *   1: out = y * scale, 2: out += y * scale                               */
int pm_block_iteration_cl(int dtype, const float* x_cl, float* out_cl,
                          const float* w1, const float* b1, const float* w2,
                          const float* b2, int batch, int length,
                          int channels, int kernel_size, int dilation,
                          int mode, float scale, void* workspace,
                          size_t workspace_bytes, void* stream);
/* pm_block_iteration_cl on a ragged batch, as a forward with `lengths` launches
 * the layer: lengths (B) int32 on the device, rows per utterance (clamped to
 * `length`). Rows of x past lengths[b] read as zero, and the rows of out_cl
 * past lengths[b] are neither read nor written. */
int pm_block_iteration_ragged_cl(int dtype, const float* x_cl, float* out_cl,
                                 const float* w1, const float* b1,
                                 const float* w2, const float* b2,
                                 const int* lengths, int batch, int length,
                                 int channels, int kernel_size, int dilation,
                                 int mode, float scale, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* A whole Block (hifigan.py:198-210), all `niter` <= 3 dilations fused in
 * one kernel: 16-bit operands for channels <= 64 at every k, 128 at k 3 and -
 * walked / skewed variants, taken for long inputs or through pm_debug_force -
 * 128 at k 7 / 11 and 256 at k 3 / 7; fp32 operands for channels <= 64
 * (PM_EINVAL "no whole-Block kernel" otherwise: use pm_block_iteration_cl);
 * w1/b1/w2/b2 are HOST arrays of `niter` device pointers;
 * workspace >= 3 * pm_op_workspace_bytes(c, c, k) [+ pm_walk_scratch_bytes] */
int pm_block_cl(int dtype, const float* x_cl, float* out_cl,
                const float* const* w1, const float* const* b1,
                const float* const* w2, const float* const* b2,
                const int* dilations, int niter, int batch, int length,
                int channels, int kernel_size, int mode, float scale,
                void* workspace, size_t workspace_bytes, void* stream);
/* pm_block_cl whose result leaves as the next upsampler's MFMA operand
 * (hifigan.py:100-106 stages lrelu(stage output) for its ConvTranspose1d):
 * act16_cl (B, L, c_pad) 16-bit = cvt(lrelu(result)) in `act_dtype` (PM_F16 |
 * PM_BF16) instead of the fp32 tensor; out_cl is read (mode 2) and left as it
 * is. Only the skewed walk does it (long inputs, scratch behind the workspace,
 * or pm_debug_skew(1)): PM_ESTATE, and the fp32 result in out_cl, otherwise. */
int pm_block_act16_cl(int dtype, int act_dtype, const float* x_cl,
                      float* out_cl, void* act16_cl, const float* const* w1,
                      const float* const* b1, const float* const* w2,
                      const float* const* b2, const int* dilations, int niter,
                      int batch, int length, int channels, int kernel_size,
                      int mode, float scale, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The whole MRF ResidualBlock of one stage (hifigan.py:141-145):
 * out = (Block_3(x) + Block_7(x) + Block_11(x)) / 3 in one launch, the sum
 * held in registers (32 channels). w1/b1/w2/b2: HOST arrays of 3 * niter
 * device pointers, Block-major (k = 3 first);
 * workspace >= 3 * niter * pm_op_workspace_bytes(c, c, 11); with
 * pm_walk_scratch_bytes(batch) more behind it the 4-byte operand layouts
 * (PM_F32, PM_F16X3, PM_F16A2) take the skewed whole-MRF walk on long batches
 * (three skewed Blocks per window, nothing recomputed)                      */
int pm_mrf_cl(int dtype, const float* x_cl, float* out_cl,
              const float* const* w1, const float* const* b1,
              const float* const* w2, const float* const* b2,
              const int* dilations, int niter, int batch, int length,
              int channels, void* workspace, size_t workspace_bytes,
              void* stream);
/* Input layers (hifigan.py:19-30, 67-68): Conv1d(c_in, c_out, 7, padding 3)
 * of the channels-last features + the k = 1 speaker conv of the (B|1, G)
 * global features as a per-utterance bias. workspace >=
 * pm_op_workspace_bytes(c_in, c_out, 7) + 256-aligned batch * pad32(c_out) * 4 */
int pm_input_conv_cl(int dtype, const float* x_cl, float* out_cl,
                     const float* weight, const float* bias,
                     const float* global_features,
                     const float* speaker_weight, const float* speaker_bias,
                     int global_batch, int global_channels, int batch,
                     int length, int c_in, int c_out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* lrelu(optional) -> ConvTranspose1d(c_in, c_out, k = 2 r, stride r,
 * padding r / 2) (hifigan.py:97-106), channels-last: (B, L, c_in_pad) ->
 * (B, L * r, c_out_pad). Launched as the engine launches the layer: with
 * 16-bit operands, an upsampler of r * c_out_pad = 128 rows (c_in 128 -> 64,
 * r = 2) takes its 256-column variant once batch * ceil(length / 256) >= 1024 */
int pm_conv_transpose_cl(int dtype, const float* x_cl, float* out_cl,
                         const float* w, const float* bias, int batch,
                         int length, int c_in, int c_out, int rate, int lrelu,
                         void* workspace, size_t workspace_bytes,
                         void* stream);
/* pm_conv_transpose_cl on a ragged batch, as a forward with `lengths` launches
 * the layer: lengths (B) int32 on the device, input rows per utterance
 * (clamped to `length`). Rows of x past lengths[b] read as zero, and the rows
 * of out_cl past rate * lengths[b] are not written. */
int pm_conv_transpose_ragged_cl(int dtype, const float* x_cl, float* out_cl,
                                const float* w, const float* bias,
                                const int* lengths, int batch, int length,
                                int c_in, int c_out, int rate, int lrelu,
                                void* workspace, size_t workspace_bytes,
                                void* stream);
/* pm_conv_transpose_cl on an input that already holds the operand values:
 * x16_cl (B, L, c_in_pad) in the operand type `dtype` (PM_F16 | PM_BF16) =
 * cvt(lrelu(x)) as pm_block_act16_cl writes it; narrow (r = 2 ...) upsamplers */
int pm_conv_transpose_x16_cl(int dtype, const void* x16_cl, float* out_cl,
                             const float* w, const float* bias, int batch,
                             int length, int c_in, int c_out, int rate,
                             void* workspace, size_t workspace_bytes,
                             void* stream);
/* LeakyReLU -> Conv1d(C, 1, 7, pad 3, no bias) -> tanh (hifigan.py:55-60):
 * (B, L, c_pad) channels-last -> (B, L). Launched as the engine launches
 * the layer: exactly 32 channels run the 32-channel kernel, any other count
 * (<= 64) the generic one                                                   */
int pm_out_conv_tanh(const float* x_cl, const float* w, float* out,
                     int batch, int length, int channels, void* stream);
/* Debug instrumentation: per-workgroup phase timestamps (s_memtime) of the
 * following fused-conv launches; buffer of 8 uint64 per workgroup or NULL  */
int pm_debug_timeline(void* dev_buffer);
/* Test hook: the walked (carry-through-LDS) variants of pm_block_cl /
 * pm_mrf_cl / the engine and the multi-block path of the wide upsampler are
 * chosen from the grid size; walk_nseg > 0 forces the walked variant with
 * that many segments per utterance, upsample_groups > 0 that many M groups
 * per column tile; 0, 0 restores the heuristics. State per HOST THREAD;
 * PM_ESTATE unless the process runs with PROMONET_HIP_DEBUG=1.              */
int pm_debug_force(int walk_nseg, int upsample_groups);
/* Test hook: -1 keeps every launcher off the skewed whole-Block walk
 * (conv_block3_skew_kernel), 1 takes it wherever it fits, 0 restores the
 * default (the shapes it measured faster on). Per host thread, and only
 * with PROMONET_HIP_DEBUG=1, like pm_debug_force.                           */
int pm_debug_skew(int mode);
/* Test hook: what the last pm_block_cl / pm_block_act16_cl / pm_mrf_cl of
 * this HOST THREAD launched - kernel: 1 the skewed walk, 2 the walked tiling,
 * 3 the two-sided tiling; nseg: segments per utterance (0: no walk); narrow:
 * the latency geometry; act16: the result left as 16-bit operands. PM_ESTATE
 * before any such launch and unless the process runs with
 * PROMONET_HIP_DEBUG=1. Host side only: it changes nothing that is launched. */
int pm_debug_last_launch(int* kernel, int* nseg, int* narrow, int* act16);
/* Measurement aid (bench.py): a register-resident loop of v_mfma_f32_32x32x16
 * (dtype PM_F16 | PM_BF16) - `workgroups` x 4 waves x `iterations` x 16 MFMAs
 * of 32 768 FLOP each - whose HIP-event time gives the matrix pipe's SUSTAINED
 * rate on this device under its power cap. operands: >= 32 768 bytes of finite
 * values of that type; sink: 4 bytes (never written). Always available (no
 * PROMONET_HIP_DEBUG needed): it changes no state of the library.           */
int pm_mfma_probe(int dtype, int iterations, const void* operands,
                  float* sink, int workgroups, void* stream);
/* Scratch the skewed whole-Block walk wants BEHIND the 3 x
 * pm_op_workspace_bytes() of pm_block_cl's workspace for `batch` utterances
 * (optional: without it the walked / stand-alone kernels run). The engine's
 * own scratch is part of pm_hifigan_workspace_bytes().                      */
size_t pm_walk_scratch_bytes(int batch);
/* torch.nn.utils.weight_norm fold: w = g * v / ||v||, rows x cols        */
int pm_fold_weight_norm(const float* g, const float* v, float* w, int rows,
                        int cols, void* stream);
/* (B, C, T) -> (B, T, c_pad) zero padded, and back                        */
int pm_to_channels_last(const float* src, float* dst, int batch, int channels,
                        int frames, int c_pad, void* stream);

/* ---- feature editing: promonet.edit (edit/core.py:17-132) -----------------
 * 1-D grid sampling (edit/grid.py:12-45) of `rows` sequences (rows, n_in) at
 * the fractional frame positions grid (n_out) (NULL = identity), with the
 * per-feature post-op fused: mode 0 linear, 1 linear in log2 then 2 ** y
 * (pitch, core.py:114), 2 nearest; then y = clip(y * scale + offset, lo, hi)
 * (pitch shift + clip core.py:121-125, loudness offset :128-129).          */
int pm_grid_sample(const float* seq, const float* grid, float* out, int rows,
                   int n_in, int n_out, int mode, float scale, float offset,
                   float lo, float hi, void* stream);
/* Selective time-stretch grid (edit/core.py:57-110, stretch_unvoiced /
 * stretch_silence off): ppg (ppg_rows, frames), `indices` (n) = rows of the
 * phonemes that ARE stretched (device int32; a row outside [0, ppg_rows) is
 * not read and turns the grid into NaN); writes selected (frames) = their
 * summed probability and grid (target_frames), the reference's sequential
 * fp32 recurrence whose step follows that probability. No selected mass (or
 * more unselected mass than target frames) yields a non-finite / decreasing
 * grid exactly as the reference's arithmetic does: callers check.           */
int pm_stretch_grid(const float* ppg, int ppg_rows, const int* indices,
                    int n_indices, float* selected, float* grid, int frames,
                    int target_frames, void* stream);

/* ---- FARGAN vocoder engine: replaces promonet.model.FARGAN ---------------
 * (promonet/model/fargan.py, selected by config/fargan.py MODEL = 'fargan').
 * One persistent workgroup per utterance; weight_dtype PM_F32, PM_F16 or
 * PM_FARGAN_MIXED is the STORAGE type of the streamed weights (math is fp32).
 * PM_FARGAN_MIXED keeps the conditioning network, the framewise conv, the
 * skip dense and the output layer (fargan.py:139-160, :349-372, :317-333) in
 * fp32 and stores the three GRU cells and every GLU gate (:212-223, :375-388)
 * - 80 % of the per-step weight stream - as f16.                            */
#define PM_FARGAN_MIXED 16
typedef struct pm_fargan_s* pm_fargan_t;
int pm_fargan_create(int num_features, int global_channels, int weight_dtype,
                     pm_fargan_t* out);
int pm_fargan_destroy(pm_fargan_t h);
/* FARGAN.state_dict() keys, e.g. conditioning_network.0.weight (371,371),
 * subframe_network.gru1.weight_ih (768,384),
 * subframe_network.skip_glu.gate.weight_g (256,1) / weight_v (256,256)     */
int pm_fargan_load_tensor(pm_fargan_t h, const char* name, const float* dev,
                          const int64_t* shape, int ndim, void* stream);
int pm_fargan_finalize(pm_fargan_t h, void* stream);
size_t pm_fargan_workspace_bytes(pm_fargan_t h, int batch, int frames);
/* FARGAN.forward(features, global_features, previous_samples)
 * (fargan.py:21-59): features (B, 114, T) - last channel = pitch period in
 * samples - or channels-last (B, T, 128) when features_cl != 0; global
 * (Bg, 258); previous (Bp, 512) or NULL (zeros); out (B, 1, 256 T).         */
int pm_fargan_forward(pm_fargan_t h, const float* features, int features_cl,
                      const float* global_features, int global_batch,
                      const float* previous_samples, int previous_batch,
                      float* out, int batch, int frames, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Ragged batch (lengths (B) int32 frames on the device): the model is causal,
 * so out[b, :256 lengths[b]] equals utterance b synthesised alone, bit for
 * bit; the tail is zeros.                                                  */
int pm_fargan_forward_ragged(pm_fargan_t h, const float* features,
                             int features_channels_last,
                             const float* global_features, int global_batch,
                             const float* previous_samples, int previous_batch,
                             const int* lengths, float* out, int batch,
                             int frames, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Streaming: the reference's FARGAN.step loop (fargan.py:65-131) over
 * `frames` >= 1 frames, starting from the given recurrent state. states
 * (B, PM_FARGAN_STATE_FLOATS) fp32 rows = the reference's `states` tuple
 * concatenated: [gru1 h 256 | gru2 h 256 | gru3 h 256 | sub-frame input 260]
 * (fargan.py:406-415), or NULL = zeros; previous (Bp, 512) in time order or
 * NULL = zeros. Writes the audio (B, 1, 256 T) and the state after the last
 * frame: previous_out (B, 512), states_out (B, PM_FARGAN_STATE_FLOATS).
 * Consecutive calls carrying that state equal one pm_fargan_forward over the
 * concatenated frames bit for bit. Workspace, kernel selection and
 * pm_fargan_check as for pm_fargan_forward. PM_EINVAL when an output overlaps
 * an input, the workspace or another output. There is no ragged form: the
 * lockstep replay of a ragged batch would advance a short utterance's state
 * past its end.                                                             */
#define PM_FARGAN_STATE_FLOATS 1028
int pm_fargan_forward_stateful(pm_fargan_t h, const float* features,
                               int features_channels_last,
                               const float* global_features, int global_batch,
                               const float* previous_samples,
                               int previous_batch, const float* states,
                               float* out, float* previous_out,
                               float* states_out, int batch, int frames,
                               void* workspace, size_t workspace_bytes,
                               void* stream);

/* Kernel selection: 0 auto (clusters of 8 workgroups per utterance up to 160
 * utterances per launch, else one persistent workgroup per utterance),
 * 1 force the latter, 2 force clusters.                                     */
int pm_fargan_set_mode(pm_fargan_t h, int mode);
/* Debug / safety: synchronise and report whether an inter-workgroup exchange
 * of the last forward on `workspace` timed out: PM_ETIMEOUT (never expected
 * on a GPU this process has to itself; the audio of that forward is invalid
 * and the caller re-runs, e.g. after pm_fargan_set_mode(h, 1)).             */
int pm_fargan_check(pm_fargan_t h, int batch, int frames, void* workspace,
                    void* stream);

/* ---- preprocessing: promonet/preprocess/spectrogram.py, loudness.py ---- */
/* spectrogram.from_audio (spectrogram.py:15-60): reflect-pad 384, hann-1024
 * hop-256 framed DFT, sqrt(re^2 + im^2 + 1e-6): audio (B, N) ->
 * (B, 513, N / 256)                                                       */
/* (a 1024-point real FFT per frame in LDS; `scratch` is unused by it and may
 * be NULL - the argument stays for the ABI of rounds 1-2)                  */
size_t pm_stft_scratch_bytes(int batch, int samples);
int pm_stft_magnitude(const float* audio, float* out, int batch, int samples,
                      void* scratch, size_t scratch_bytes, void* stream);
/* The same spectrogram by the brute-force framed-DFT GEMM (exact-fp32 MFMA):
 * an independent cross-check of the FFT; scratch: pm_stft_scratch_bytes()  */
int pm_stft_magnitude_dft(const float* audio, float* out, int batch,
                          int samples, void* scratch, size_t scratch_bytes,
                          void* stream);
/* spectrogram.from_audio(audio, mels=True) (spectrogram.py:56-58 ->
 * linear_to_mel :111-133) in one kernel: log(basis @ magnitude), optional
 * clamp, straight from the FFT workgroup's LDS tile: audio (B, N) ->
 * (B, mels, N / 256). pm_stft_mel_prepare compacts the (mels, 513) basis
 * (librosa.filters.mel at spectrogram.py:118-121) into `prepared`
 * (pm_stft_mel_scratch_bytes(mels) bytes) once; the reference rebuilds its
 * basis on every call.                                                      */
size_t pm_stft_mel_scratch_bytes(int mels);
int pm_stft_mel_prepare(const float* basis, int mels, void* prepared,
                        size_t prepared_bytes, void* stream);
int pm_stft_mel(const float* audio, const void* prepared, float* out,
                int batch, int samples, int mels, int use_threshold,
                float log_threshold, void* stream);
/* Tuning knob: frames per FFT workgroup, 16 (default; two workgroups per CU)
 * or 32 (one 8-wave workgroup, 128-byte output rows). Per host thread; an API
 * call reads it once (both passes of pm_loudness use the same value).      */
int pm_stft_set_frames_per_group(int frames);
/* Schedule of pm_loudness with the default 8 bands: 2 (default) = a maximum
 * pass, then the band pass, two transforms per frame; 1 = OPTIMISTIC: the
 * first pass already writes the band means without a floor and the second
 * transforms only the 16-frame groups that have a bin under their utterance's
 * floor (the others are final, bit for bit). Pays on material at a steady
 * level (56 -> 47 us at batch 32 x 10 s of noise), costs up to + 25 % where
 * most groups hold a bin 80 dB under the maximum. Per host thread.           */
int pm_stft_set_loudness_passes(int passes);
/* The launch geometry one FFT transform would take for (batch, samples) on the
 * current device and host thread: `total_groups` (utterance, frame-group)
 * pairs walked by `workgroups` persistent workgroups (= min(total, occupancy x
 * CUs)); transform 1 = magnitude, 4 = log-mel, 2 / 3 / 5 = the loudness passes
 * (maximum, generic bands, the default 8 bands). Launches nothing.           */
int pm_stft_launch_info(int transform, int batch, int samples,
                        int* total_groups, int* workgroups);
/* spectrogram.linear_to_mel (spectrogram.py:111-133): log(basis @ spec),
 * optional clamp: spec (B, F, T), basis (Mel, F) -> (B, Mel, T)           */
int pm_linear_to_mel(const float* spec, const float* basis, float* out,
                     int batch, int bins, int mels, int frames,
                     int use_threshold, float log_threshold, void* stream);
/* Backward passes of the two functions above, for the training-side mel loss
 * that differentiates through spectrogram.from_audio(generated, True)
 * (promonet/train/core.py:277-305): grad_out (B, 513, N / 256) ->
 * grad_audio (B, N); grad_mel (B, Mel, T) -> grad_spec (B, F, T), `scratch`
 * = batch * mels * frames floats.                                          */
size_t pm_stft_backward_scratch_bytes(int batch, int samples);
int pm_stft_magnitude_backward(const float* audio, const float* grad_out,
                               float* grad_audio, int batch, int samples,
                               void* scratch, size_t scratch_bytes,
                               void* stream);
int pm_linear_to_mel_backward(const float* spec, const float* basis,
                              const float* grad_mel, float* grad_spec,
                              float* scratch, int batch, int bins, int mels,
                              int frames, int use_threshold,
                              float log_threshold, void* stream);
/* loudness.from_audio (loudness.py:17-55) per utterance: A-weighted dB with
 * the utterance-global (max - 80 dB) floor of librosa.amplitude_to_db, then
 * band_average (loudness.py:84-111): audio (B, N) -> (B, bands, N / 256);
 * two FFT passes over the audio (maximum, then bands), no dB tensor in HBM;
 * a_weights (513) = perceptual_weights() (loudness.py:149-160);
 * scratch: pm_loudness_scratch_bytes()                                     */
size_t pm_loudness_scratch_bytes(int batch, int samples);
int pm_loudness(const float* audio, const float* a_weights, float* out,
                int batch, int samples, int bands, float min_db,
                void* scratch, size_t scratch_bytes, void* stream);

/* ---- loudness editing: promonet/preprocess/loudness.py:114-141, :179-193 ---
 * pm_limit, the look-ahead limiter (:114-141), all fp32, every operation one
 * rounding of its own (no fma), for n = 0 .. len + delay - 2 with x[n] = 0
 * from len on, e[-1] = 0, g[-1] = 1:
 *   e[n] = max(|x[n]|, e[n-1] release)
 *   t[n] = e[n] > threshold ? (1 / e[n]) threshold : 1
 *   g[n] = g[n-1] attack + t[n] attack_complement
 *   out[j] = x[j] g[j + delay - 1]
 * attack_complement is the fp32 rounding of 1 - attack_coef taken in double,
 * as the reference's Python arithmetic has it. x: `rows` rows of `samples`,
 * x_stride floats apart; FINITE input is a precondition. lengths: device int32
 * per row, clamped to [0, samples], read on the device only (NULL: full rows);
 * out is exact zero from a row's length on and must not overlap x. gain: NULL,
 * or rows of samples + delay - 1 floats that receive g[0 .. len + delay - 2]
 * (zero beyond). One workgroup per row, in tiles of pm_limit_tile's `tile`
 * steps, a lane taking `chunk` of them: exact whatever the tiling, see
 * pm_limit.h. The workspace (pm_limit_workspace_bytes; 0 for rows < 1)
 * receives 4 int32 per row: envelope steps and gain steps walked serially,
 * chunks walked, tiles skipped as a whole. 1 <= delay, the coefficients inside
 * (0, 1), threshold > 0. Asynchronous, no allocation, capturable; argument
 * errors are reported before any GPU call.
 * pm_loudness_shift (:179-193): out = x gain, gain = 2^(db / 10) per frame,
 * interpolated linearly to the row's samples as torch's interpolate(mode =
 * 'linear', align_corners = False): src = max(0, (n + .5) F / N - .5), split
 * into index and weight in integers. Per row N = lengths[row] (clamped to
 * [0, samples]) and F = frame_lengths[row] (clamped to [1, frames]), device
 * int32 or NULL for `samples` and `frames`; frames == 1 is the scalar shift.
 * db: rows of `frames`, db_stride apart (0: one contour for every row).
 * Zeros from a row's length on; out may be x.                                */
int pm_limit_tile(int* chunk, int* tile);
size_t pm_limit_workspace_bytes(int rows);
int pm_limit(const float* x, const int* lengths, float* out, float* gain,
             int rows, int samples, long long x_stride, long long out_stride,
             int delay, float attack, float attack_complement, float release,
             float threshold, void* workspace, size_t workspace_bytes,
             void* stream);
int pm_loudness_shift(const float* x, const float* db, const int* lengths,
                      const int* frame_lengths, float* out, int rows,
                      int samples, long long x_stride, int frames,
                      long long db_stride, long long out_stride, void* stream);

/* ---- resampling: torchaudio.functional.resample on the device -------------
 * Replaces the host resampler of promonet/load.py:16-28 (load.audio) and
 * promonet/baseline/mels.py:174- (mels.resample): torchaudio's
 * 'sinc_interp_hann' algorithm, a polyphase bank of `new` Hann-windowed sinc
 * filters of taps = 2 width + orig each, applied with stride `orig`.
 * x: `rows` rows of up to n_in samples, x_stride floats apart; lengths: device
 * int32 per row, clamped to [0, n_in] on the device and never read on the
 * host (NULL: every row has n_in); bank: the filters TRANSPOSED, (taps, new).
 * For a row of length len, out[q new + p] = sum_k bank[k][p]
 * x[q orig + k - width] (x = 0 outside [0, len)) up to ceil(new len / orig),
 * and exact zeros from there to n_out >= ceil(new n_in / orig). One fp32
 * accumulator and an fma chain in ascending k per output: its bits depend on
 * its row and index only, not on the tiling, the batch or `lengths`.
 * Asynchronous, no allocation, no workspace; argument errors are reported
 * before any GPU call. pm_resample_tile: the strides q one workgroup takes
 * for this ratio (tile = that many x new outputs); negative on bad arguments
 * and for a filter too long for the kernel's LDS segment (no standard rate
 * pair: 8192 floats hold 4 strides of any of them), which pm_resample refuses
 * in the same way.                                                          */
int pm_resample_tile(int orig, int new_rate, int width);
int pm_resample(const float* x, const int* lengths, const float* bank,
                float* out, int rows, int n_in, long long x_stride, int orig,
                int new_rate, int width, int n_out, long long out_stride,
                void* stream);

/* ---- resampling at any ratio: resampy.resample on the device --------------
 * Replaces the resampy.resample calls ('kaiser_best') of promonet/data/
 * augment/{pitch,loudness}.py. Where pm_resample needs one filter per output
 * phase, this reads ONE long windowed-sinc table with linear interpolation at
 * a per-output phase, so any pair of rates is served (22 051 -> 22 050, or
 * int(1.2345 * 44100) -> 44 100).
 * The table. P = PM_RESAMPLE_INTERP_STEPS = 2^9 steps per zero crossing, 64
 * zero crossings, N = 64 P; win and delta hold N + 1 =
 * PM_RESAMPLE_INTERP_TABLE floats. For resampy's filter, in float64,
 *   win[j] = rolloff sinc(rolloff j / P) kaiser(2 N + 1, beta)[N + j],
 * multiplied by new / orig when new < orig, delta[j] = win[j + 1] - win[j],
 * delta[N] = 0, both then rounded to fp32 (promonet_amd/resampy.py). The
 * entry takes any two tables of that size.
 * Positions, in integers. For output t of a row with rates (orig, new):
 *   n = t orig div new, rem = t orig mod new (64 bits), D = max(orig, new),
 *   left wing:  off  = rem P div D,          eta  = (rem P mod D) / D,
 *   right wing: off' = (new - rem) P div D,  eta' = ((new - rem) P mod D) / D,
 *   step = min(orig, new) P div orig,
 * eta and eta' the fp32 roundings of the exact quotients. (resampy forms the
 * same quantities in float64 from t (orig / new); they agree wherever float64
 * does not round across an integer.)
 * Values. One fp32 accumulator starts at 0; then, ascending,
 *   i = 0 .. min(n + 1, (N + 1 - off) div step) - 1:
 *     w = fma(eta, delta[off + i step], win[off + i step])
 *     acc = fma(w, x[n - i], acc)
 *   k = 0 .. min(len - n - 1, (N + 1 - off') div step) - 1:
 *     the same with eta', off' and x[n + k + 1].
 * A row of length len yields len new div orig outputs; exact zeros follow up
 * to n_out. A sample's bits depend on its row's samples, its row's rates and
 * its own index only.
 * x: `rows` rows of up to n_in samples, x_stride floats apart. lengths, orig,
 * new_rate: device int32 per row, read on the device only (lengths clamped to
 * [0, n_in]; NULL: every row has n_in), so one launch carries one ratio per
 * row and a captured graph replays with other ratios. Asynchronous, no
 * allocation, no workspace; argument errors are reported before any GPU call.
 * pm_resample_interp_tile: the outputs one workgroup takes, or PM_EINVAL for
 * rates the kernel refuses: below 1, 2^21 or more, or a ratio new / orig so
 * small that the input segment of one tile does not fit the kernel's 6144
 * floats of LDS (every ratio from 1/5.3 up fits, every upsampling ratio too).
 * The rates being device data, a row with refused rates is answered on the
 * device: NaN in all of out[0, n_out) of that row, never a slower walk and
 * never an access out of bounds.                                            */
#define PM_RESAMPLE_INTERP_STEPS 512
#define PM_RESAMPLE_INTERP_TABLE (64 * PM_RESAMPLE_INTERP_STEPS + 1)
int pm_resample_interp_tile(int orig, int new_rate);
int pm_resample_interp(const float* x, const int* lengths, const int* orig,
                       const int* new_rate, const float* win,
                       const float* delta, float* out, int rows, int n_in,
                       long long x_stride, int n_out, long long out_stride,
                       void* stream);

/* ---- Viterbi decoding: torbi.from_probabilities on the device -------------
 * (the decoder of promonet/preprocess/harmonics.py:270-276 and of penn's
 * pitch contour). With A = log transition, B = log observation (batch,
 * frames, states), p = log initial, all fp32:
 *   d_0[j] = B[0][j] + p[j];  m_t[j] = argmax_i d_{t-1}[i] + A[j][i];
 *   d_t[j] = B[t][j] + (d_{t-1}[m] + A[j][m])
 * each sum one fp32 add in that association; the last state is the argmax of
 * d_{len-1}, earlier states follow the back-pointers; every tie goes to the
 * lowest index, the tie of all -inf included. A[j][i] is the step from i to
 * j. The transition is passed banded: table (3, states) int32 = lo, count and
 * offset of every row j; band[offset_j + k] = A[j][lo_j + k], k < count_j,
 * padded with -inf to a multiple of 4 floats (offset_j a multiple of 4);
 * outside [lo_j, lo_j + count_j) A is -inf. A table entry that points outside
 * the band or the states makes its row empty, never an access out of bounds.
 * lengths: device int32 per row, clamped to [0, frames], read on the device
 * only (NULL: every row has `frames`); out (batch, frames) int32 is zero from
 * a row's length on. states <= 32767 (int16 back-pointers in the workspace,
 * pm_viterbi_workspace bytes: 0 for invalid sizes) and two rows of scores
 * must fit 64 KiB of LDS (states <= 8188). One workgroup per row;
 * asynchronous, no allocation, capturable.                                  */
size_t pm_viterbi_workspace(int batch, int frames, int states);
int pm_viterbi(const float* observation, const int* lengths,
               const float* band, long long band_floats, const int* table,
               const float* initial, int* out, int batch, int frames,
               int states, void* workspace, size_t workspace_bytes,
               void* stream);

/* ---- harmonic analysis: promonet/preprocess/harmonics.py ------------------
 * pm_harmonics_highpass (:378-381): y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2]
 * - a1 y[n-1] - a2 y[n-2] over each row's length (device int32 or NULL), zero
 * state, clamped to [-1, 1] once at the end as torchaudio's lfilter does;
 * zeros past the length.
 * pm_harmonics_stft (:390-428): geometry (rows, 3) int32 = samples, frames
 * and reflect padding of each row; Hann `window` (4096); twiddle (2048, 2) =
 * (cos, -sin)(2 pi k / 4096); out (rows, frames, states) = sqrt(re^2 + im^2 +
 * 1e-6) of bins [bin0, bin0 + states), frames-major, zeros past a row's
 * frames.
 * pm_harmonics_observation (:228-229, :252-264, :285-295): one decode round's
 * log softmax per frame. f0 NULL: round 0, the bias 0.5 (states - s) added.
 * Else masked to [searchsorted(frequencies, f0 low), searchsorted(
 * frequencies, f0 high)), -inf outside; a frame with an empty mask, a NaN f0
 * or past row_frames (device int32 or NULL) is all zeros and valid = 0.
 * pm_harmonics_peaks (:199-212): the first `peaks` local maxima of each
 * frame (scipy.signal.find_peaks without conditions) as frequencies, NaN
 * beyond them; out (rows, peaks, frames).                                   */
int pm_harmonics_highpass(const float* x, const int* lengths, float* y,
                          int rows, int samples, long long x_stride,
                          long long y_stride, float b0, float b1, float b2,
                          float a1, float a2, void* stream);
int pm_harmonics_stft(const float* x, const int* geometry,
                      const float* window, const float* twiddle, float* out,
                      int rows, long long x_stride, int frames, int states,
                      int bin0, int hop, void* stream);
int pm_harmonics_observation(const float* x, const float* f0,
                             const float* frequencies, const int* row_frames,
                             float* out, int* valid, int rows, int frames,
                             int states, float low, float high, void* stream);
int pm_harmonics_peaks(const float* x, const float* frequencies,
                       const int* row_frames, float* out, int rows, int frames,
                       int states, int peaks, void* stream);

/* ---- LPC features: promonet/preprocess/harmonics.py:305-330 ---------------
 * lpc_coefficients on the device. audio: `rows` rows of up to `samples`
 * samples, `stride` floats apart; lengths: device int32 per row, clamped to
 * [0, samples] on the device and never read on the host (NULL: every row has
 * `samples`). Frame t of a row of len samples is samples [256 t - 384,
 * 256 t + 640) of it, zero outside [0, len), times `window` (1024 floats,
 * 16-byte aligned); a row has max(0, (len - 256) / 256 + 1) frames. Per frame
 * Burg's predictor of `order` (1 to 32; librosa.lpc restated, parity
 * unpinned), its denominator recomputed as sum(f^2 + b^2) every order, and
 *   features[row][t][k] = -log10 |sum_j a[j] e^(-i pi j k / 512)|, k < 512,
 * with table (1024, 4) = the float64 (cos, sin)(2 pi m / 1024) split by the
 * caller into float heads (cos, sin) and float tails (cos, sin), 16-byte
 * aligned: the response is summed in float64. features (rows, frames, 512);
 * coefficients (rows, frames, order + 1) = a, or NULL. A silent frame gives
 * a = [1, 0, ...] and features +0; frames from a row's count on give zeros in
 * both. One wave a frame: a frame's bits depend on its samples alone. At most
 * 2^32 - 1 threads a launch (67 108 860 frames). Asynchronous, no allocation,
 * no workspace, no atomics, capturable; argument errors are reported before
 * any GPU call.                                                             */
int pm_harmonics_lpc(const float* audio, const int* lengths,
                     const float* window, const float* table, float* features,
                     float* coefficients, int rows, long long stride,
                     int samples, int frames, int order, void* stream);

/* ---- training losses of the FARGAN configurations: promonet/train/loss.py --
 * Spectral convergence (:61-150): s = sqrt(max(|STFT(x)|, 1e-7)) with
 * torch.stft's center = True reflect padding (samples > fft_size / 2), the
 * loss is sum |s_y - s_x| / sum s_y over the whole batch. fft_size is 2^a or
 * 5 2^a in [64, 2560], 1 <= hop_size <= fft_size; frames = 1 + samples /
 * hop_size, bins = fft_size / 2 + 1. window (fft_size) is the window already
 * zero-padded to fft_size; twiddle (fft_size, 2) = (cos, -sin)(2 pi m /
 * fft_size); both fp32, rounded from float64 by the caller.
 * Stage 1, the transform: s (batch, bins, frames), or NULL. With `gradient`
 * (batch, bins, frames, 2) it also writes upstream * X / (2 s |X|) where |X| >
 * 1e-7 and 0 elsewhere, the gradient of a loss whose derivative by s is
 * `upstream` (batch, bins, frames).
 * Stage 2, the loss: sums (3) = S1 = sum |s_y - s_x|, S2 = sum s_y and S1 / S2,
 * reduced in a fixed order (per-workgroup partials, one final pass). With
 * with_gradient the workspace begins with G (batch, bins, frames, 2) =
 * -sign(s_y - s_x) X / (2 s_x |X|) where |X| > 1e-7, 0 elsewhere: d S1 / d X.
 * Stage 3, the adjoint: grad_x (batch, samples) = (or, with accumulate, +=)
 * scale[0] * A(G), A the adjoint of x -> STFT(x): the inverse real transform
 * of each frame with every bin counted once (the imaginary parts of bins 0
 * and fft_size / 2 are ignored), the window, overlap-add in gather form and
 * the fold of the two reflected margins. scale is a device scalar.
 * No float atomics: every output is bit-identical from run to run. All
 * asynchronous, no allocation, capturable; the workspace queries return 0 for
 * sizes outside the limits.                                                 */
size_t pm_sc_forward_workspace_bytes(int batch, int samples, int fft_size,
                                     int hop_size, int with_gradient);
size_t pm_sc_adjoint_workspace_bytes(int batch, int samples, int fft_size,
                                     int hop_size);
int pm_sc_stft(const float* x, const float* window, const float* twiddle,
               const float* upstream, float* s, float* gradient, int batch,
               int samples, int fft_size, int hop_size, void* stream);
int pm_sc_forward(const float* x, const float* y, const float* window,
                  const float* twiddle, float* sums, int batch, int samples,
                  int fft_size, int hop_size, int with_gradient,
                  void* workspace, size_t workspace_bytes, void* stream);
int pm_sc_adjoint(const float* gradient, const float* window,
                  const float* twiddle, const float* scale, float* grad_x,
                  int batch, int samples, int fft_size, int hop_size,
                  int accumulate, void* workspace, size_t workspace_bytes,
                  void* stream);
/* signal (:158-162): out (1) = mean over rows of 1 - <p, t> with p, t the
 * rows of y_pred, y_true over (1e-15 + their L2 norm). The forward leaves the
 * rows' sums in the workspace; the backward reads them there and writes
 * grad (rows, samples) = grad_out[0] * d out / d y_pred.                    */
size_t pm_signal_loss_workspace_bytes(int rows);
int pm_signal_loss(const float* y_true, const float* y_pred, float* out,
                   int rows, int samples, void* workspace,
                   size_t workspace_bytes, void* stream);
int pm_signal_loss_backward(const float* y_true, const float* y_pred,
                            const float* grad_out, float* grad, int rows,
                            int samples, const void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- discriminator spectrograms: promonet/model/discriminator.py ----------
 * The transform at the entrance of each spectral discriminator, forward and
 * backward, on the FFT of the spectral-convergence loss above (the same sizes,
 * window and twiddle tables). The frames are NOT centred by the transform:
 * the row is reflect padded by `pad` on both sides (samples > pad) and
 * frames = 1 + (samples + 2 pad - fft_size) / hop_size >= 1. bins =
 * fft_size / 2 + 1. win_length (1 .. fft_size) is only checked: the window
 * (fft_size) arrives zero-padded.
 *   PM_DISC_SPEC_R    DiscriminatorR.spectrogram (:129-143), pad = (fft_size
 *                     - hop_size) / 2: out (batch, bins, frames) = |X|
 *   PM_DISC_SPEC_CMB  DiscriminatorCMB.spectrogram (:175-192), the same pad:
 *                     out (batch, frames, bins) = |X|, which the caller slices
 *                     into bands along its last axis
 *   PM_DISC_SPEC_DB   SpecDiscriminatorBase.spectrogram (:278-299), pad =
 *                     fft_size / 2: out (batch, bins, frames) = max(d, floor),
 *                     d = 20 log10 max(|X|, 1e-5), floor = (max of d over the
 *                     WHOLE batch) - 80; stats (2 device floats) receives
 *                     (max, floor). The maximum goes through one partial a
 *                     workgroup in the workspace; nothing syncs with the host.
 * stats and the workspace may be NULL for R and CMB.
 * Backward: grad_x (batch, samples) = (or, with accumulate, +=) scale[0] *
 * (d <upstream, out> / d x); scale is a device scalar, NULL for 1. upstream
 * has the layout of the mode's out. The transform is computed again from x;
 * the bin gradient is upstream X / |X| (0 where |X| = 0) for R and CMB. For DB
 * the caller passes the forward's out and stats back: an element with
 * saved_out > floor passes upstream (20 / ln 10) X / |X|^2 where |X| >= 1e-5
 * and nothing below; the others pass their upstream to the floor, and the sum
 * of those (fixed-order partials in double, one final pass) is shared evenly
 * among the elements whose saved_out equals max. An element exactly at the
 * floor before the floor was applied counts as floored (torch gives each side
 * a half). Then the adjoint of pm_sc_adjoint with the margins of `pad`.
 * No float atomics: every output is bit-identical from run to run. All
 * asynchronous, no allocation, capturable. Sizes outside the limits (fft_size
 * not 2^a or 5 2^a in [64, 2560], hop_size outside [1, fft_size], win_length
 * outside [1, fft_size], pad outside [0, fft_size], samples <= pad, less than
 * one frame, an unknown mode) return PM_EINVAL before any device work; the
 * workspace query returns 0 for them and at least 256 otherwise.            */
#define PM_DISC_SPEC_R 0
#define PM_DISC_SPEC_CMB 1
#define PM_DISC_SPEC_DB 2
size_t pm_disc_spec_workspace_bytes(int mode, int batch, int samples,
                                    int fft_size, int hop_size, int win_length,
                                    int pad, int backward);
int pm_disc_spec_forward(int mode, const float* x, const float* window,
                         const float* twiddle, float* out, float* stats,
                         int batch, int samples, int fft_size, int hop_size,
                         int win_length, int pad, void* workspace,
                         size_t workspace_bytes, void* stream);
int pm_disc_spec_backward(int mode, const float* x, const float* window,
                          const float* twiddle, const float* upstream,
                          const float* saved_out, const float* stats,
                          const float* scale, float* grad_x, int accumulate,
                          int batch, int samples, int fft_size, int hop_size,
                          int win_length, int pad, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- FARGAN discriminator conv stacks: promonet/model/discriminator.py ----
 * One layer of DiscriminatorMagFree (:320-389), forward and backward:
 *   y = act(conv3x3(cat(x, sin, cos)) + bias)
 * with stride 1, dilation (dilation, 1) and padding (dilation, 1), the two
 * channels of FrequencyPositionalEmbedding (:381-389) read from `table`
 * (bins, 2) = sin, cos of 2 pi f / bins and zero outside the map, as the
 * conv's own padding makes them. fp32 throughout; the layers with 16 output
 * channels run on the fp32-input MFMA.
 * MEMORY ORDER: a map of 16 channels is channels_last, in memory (batch, bins,
 * frames, 16); a map of one channel is (batch, bins, frames). x has `channels`
 * (1 or 16) channels, y and upstream `out_channels` (16 or 1; not 1 on both
 * sides); weight is torch's (out_channels, channels + 2, 3, 3), bias
 * (out_channels).
 * Backward: from upstream, the saved y and the saved x, with gz = upstream *
 * act'(y) (relu: y > 0; sigmoid: y (1 - y)): grad_x in the layout of x (NULL
 * skips it), grad_weight and grad_bias (both NULL skips them). The two sums
 * over all pixels go through per-workgroup partials in the workspace, whose
 * count depends on the sizes alone, added in a fixed order: no float atomics,
 * the same bits on every run. All asynchronous, no allocation, capturable.
 * channels not 1 or 16, out_channels not 1 or 16, dilation not 1, 2, 4, 8 or
 * 16, batch, bins or frames below 1, an unknown activation, too many pixels
 * for one launch or a workspace that is too small are refused before any
 * device work; the workspace query returns 0 for such sizes.
 * pm_fdisc_weight_norm_*: w = g v / |v| with the norm per output channel over
 * its `fan` = (channels + 2) * 9 values (torch._weight_norm, dim 0), and the
 * adjoint from grad_w to (grad_g, grad_v).                                  */
#define PM_FDISC_NONE 0
#define PM_FDISC_RELU 1
#define PM_FDISC_SIGMOID 2
size_t pm_fdisc_workspace_bytes(int batch, int channels, int out_channels,
                                int bins, int frames);
int pm_fdisc_conv_forward(const float* x, const float* weight,
                          const float* bias, const float* table, float* y,
                          int batch, int channels, int out_channels, int bins,
                          int frames, int dilation, int activation,
                          void* stream);
int pm_fdisc_conv_backward(const float* upstream, const float* y,
                           const float* x, const float* weight,
                           const float* table, float* grad_x,
                           float* grad_weight, float* grad_bias, int batch,
                           int channels, int out_channels, int bins,
                           int frames, int dilation, int activation,
                           void* workspace, size_t workspace_bytes,
                           void* stream);
/* pm_fdisc_layer_*: one layer of a stack at any of the six resolutions,
 *   y = act(conv2d(cat(x, sin, cos), weight, bias, stride (stride, 1),
 *                  dilation 1, padding (1, 1)))
 * with `bins` the input's and (bins - 1) / stride + 1 output bins: output row
 * fo reads the input rows stride * fo + kf - 1, zero outside the map for the
 * map and the embedding alike; `table` (bins, 2) is the embedding of the
 * INPUT. (channels, out_channels, stride) is one of (1, 16, s), (16, 32, s),
 * (32, 64, s), (64, 128, s), (128, 256, s) with s 1 or 2, (16, 16, 1),
 * (32, 32, 1), (64, 64, 1), (128, 128, 1) and (C, 1, 1) with C 16, 32, 64, 128
 * or 256: what the reference builds. The three forms of pm_fdisc_conv_* at
 * stride 1 run its kernels. Memory order, backward, partials and refusals as
 * above: a map of 16 or more channels is channels_last. A form outside the
 * list, a stride other than 1 or 2, batch, bins or frames below 1, an unknown
 * activation, more than 2^31 - 1 input or output pixels, a null pointer or a
 * workspace that is too small (PM_ENOMEM) are refused before any device work;
 * the workspace query returns 0 for such sizes.                              */
size_t pm_fdisc_layer_workspace_bytes(int batch, int channels,
                                      int out_channels, int bins, int frames,
                                      int stride);
int pm_fdisc_layer_forward(const float* x, const float* weight,
                           const float* bias, const float* table, float* y,
                           int batch, int channels, int out_channels, int bins,
                           int frames, int stride, int activation,
                           void* stream);
int pm_fdisc_layer_backward(const float* upstream, const float* y,
                            const float* x, const float* weight,
                            const float* table, float* grad_x,
                            float* grad_weight, float* grad_bias, int batch,
                            int channels, int out_channels, int bins,
                            int frames, int stride, int activation,
                            void* workspace, size_t workspace_bytes,
                            void* stream);
int pm_fdisc_weight_norm_forward(const float* g, const float* v, float* w,
                                 int out_channels, int fan, void* stream);
int pm_fdisc_weight_norm_backward(const float* grad_w, const float* g,
                                  const float* v, float* grad_g, float* grad_v,
                                  int out_channels, int fan, void* stream);

/* ---- CMB and resolution discriminator conv stacks --------------------------
 * One layer of DiscriminatorCMB.band_convs / conv_post
 * (promonet/model/discriminator.py:146-208) and of DiscriminatorR.convs /
 * conv_post (:96-127), forward and backward:
 *   y = leaky(conv2d(x, weight, bias, stride (1, stride),
 *                    padding (1, (kernel_width - 1) / 2)), slope)
 * with (channels, out_channels, kernel_width, stride) one of (1, 32, 9, 1),
 * (32, 32, 9, 2), (32, 32, 3, 1), (32, 1, 3, 1): the whole reference. The
 * output is (width - 1) / stride + 1 wide and `height` high. slope 1 is no
 * activation. fp32 throughout; the 32 -> 32 layers run on the fp32-input MFMA.
 * MEMORY ORDER: a map of 32 channels is channels_last, in memory (batch,
 * height, width, 32); a map of one channel is (batch, height, width). weight
 * is torch's (out_channels, channels, 3, kernel_width), bias (out_channels).
 * Backward: from upstream, the saved y and the saved x, with gz = upstream *
 * (y > 0 ? 1 : slope): grad_x in the layout of x (NULL skips it), grad_weight
 * and grad_bias (both NULL skips them). The two sums over all pixels go
 * through per-workgroup partials in the workspace, whose count depends on the
 * sizes alone, added in a fixed order in double: no float atomics, the same
 * bits on every run. All asynchronous, no allocation, capturable.
 * Another form, batch, height or width below 1, a slope that is not finite or
 * not in (0, 1], more than 2^31 - 1 input or output pixels, a null pointer or
 * a workspace that is too small are refused before any device work; the
 * workspace query returns 0 for such sizes.                                 */
size_t pm_dconv_workspace_bytes(int batch, int channels, int out_channels,
                                int height, int width, int kernel_width,
                                int stride);
int pm_dconv_forward(const float* x, const float* weight, const float* bias,
                     float* y, int batch, int channels, int out_channels,
                     int height, int width, int kernel_width, int stride,
                     float slope, void* stream);
int pm_dconv_backward(const float* upstream, const float* y, const float* x,
                      const float* weight, float* grad_x, float* grad_weight,
                      float* grad_bias, int batch, int channels,
                      int out_channels, int height, int width,
                      int kernel_width, int stride, float slope,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- period discriminator conv stack ---------------------------------------
 * One layer of DiscriminatorP.convs / conv_post
 * (promonet/model/discriminator.py:57-93), forward and backward:
 *   y = leaky(conv2d(x, weight, bias, stride (stride, 1),
 *                    padding ((kernel - 1) / 2, 0)), slope)
 * with x (batch, channels, height, period) and (channels, out_channels,
 * kernel, stride) one of (1, 32, 5, 3), (32, 128, 5, 3), (128, 512, 5, 3),
 * (512, 1024, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1): the whole
 * reference. The conv runs along the height alone; the output is (height - 1)
 * / stride + 1 high and `period` wide. slope 1 is no activation. fp32
 * throughout; the layers of 32 and more channels on both sides run on the
 * fp32-input MFMA.
 * MEMORY ORDER: a map of 32 or more channels is channels_last, in memory
 * (batch, height, period, channels); a map of one channel is (batch, height,
 * period). weight is torch's (out_channels, channels, kernel, 1), bias
 * (out_channels).
 * THE FOLD: pm_pconv_fold_* are the first layer, (1, 32, 5, 3), on the audio
 * (batch, samples) itself: the map (batch, (samples + n) / period, period) of
 * the reference, n = (period - samples mod period) mod period samples
 * reflected on the right, is read in place (sample t >= samples is sample
 * 2 (samples - 1) - t) and never written. grad_audio (batch, samples) holds
 * the adjoint of that reflection, in gather form.
 * Backward: from upstream, the saved y and the saved x, with gz = upstream *
 * (y > 0 ? 1 : slope): grad_x in the layout of x (NULL skips it), grad_weight
 * and grad_bias (both NULL skips them). The sums over all pixels go through
 * partials in the workspace, whose count depends on the sizes alone, added in
 * a fixed order in double: no float atomics, the same bits on every run. All
 * asynchronous, no allocation, capturable.
 * Another form, batch or height below 1, a period outside 1 ... 64, samples <=
 * n, a slope that is not finite or not in (0, 1], more than 2^31 - 1 input or
 * output pixels, a null pointer or a workspace that is too small are refused
 * before any device work; the workspace queries return 0 for such sizes.    */
size_t pm_pconv_workspace_bytes(int batch, int channels, int out_channels,
                                int height, int period, int kernel,
                                int stride);
int pm_pconv_forward(const float* x, const float* weight, const float* bias,
                     float* y, int batch, int channels, int out_channels,
                     int height, int period, int kernel, int stride,
                     float slope, void* stream);
int pm_pconv_backward(const float* upstream, const float* y, const float* x,
                      const float* weight, float* grad_x, float* grad_weight,
                      float* grad_bias, int batch, int channels,
                      int out_channels, int height, int period, int kernel,
                      int stride, float slope, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t pm_pconv_fold_workspace_bytes(int batch, int samples, int period);
int pm_pconv_fold_forward(const float* audio, const float* weight,
                          const float* bias, float* y, int batch, int samples,
                          int period, float slope, void* stream);
int pm_pconv_fold_backward(const float* upstream, const float* y,
                           const float* audio, const float* weight,
                           float* grad_audio, float* grad_weight,
                           float* grad_bias, int batch, int samples,
                           int period, float slope, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- generator training: one conv of an MRF Block --------------------------
 * One conv of Block (promonet/model/hifigan.py:198-210) with its input
 * activation and its residual add, forward and backward:
 *   y = conv1d(leaky(x, slope), weight, bias, dilation,
 *              padding (kernel - 1) dilation / 2) [+ residual]
 * with x, y and residual (batch, channels, frames), channels in and out
 * equal, channels 32, 64, 128 or 256, kernel 3, 7 or 11, dilation 1, 3 or 5:
 * 36 forms. slope 1 is no activation; residual may be NULL. fp32 throughout,
 * the products on the fp32-input MFMA.
 * MEMORY ORDER: channels_last, in memory (batch, frames, channels). weight is
 * torch's (channels, channels, kernel), bias (channels). A tap outside [0,
 * frames) of its own utterance reads zero.
 * Backward: from upstream and the saved INPUT x: grad_x = leaky'(x) * (the
 * conv of upstream with the transposed, tap-mirrored weight), x = 0 taking
 * the slope (NULL skips it); grad_weight and grad_bias from upstream and
 * leaky(x) (both NULL skips them). The gradient of the residual is upstream
 * itself. The sums over all pixels go through partials in the workspace,
 * whose count depends on the sizes alone, added in a fixed order in double:
 * no float atomics, the same bits on every run. All asynchronous, no
 * allocation, capturable.
 * Another form, batch or frames below 1, more than 2^31 - 1 pixels, a slope
 * that is not finite or not in (0, 1], a null pointer other than the optional
 * ones or a workspace that is too small (PM_ENOMEM) are refused before any
 * device work; the workspace query returns 0 for such sizes.               */
size_t pm_gconv_workspace_bytes(int batch, int channels, int frames,
                                int kernel, int dilation);
int pm_gconv_forward(const float* x, const float* weight, const float* bias,
                     const float* residual, float* y, int batch, int channels,
                     int frames, int kernel, int dilation, float slope,
                     void* stream);
int pm_gconv_backward(const float* upstream, const float* x,
                      const float* weight, float* grad_x, float* grad_weight,
                      float* grad_bias, int batch, int channels, int frames,
                      int kernel, int dilation, float slope, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- adversarial losses: promonet/train/loss.py:11-53 ---------------------
 * feature_matching, discriminator and generator are each a sum of means over
 * a list of tensors of unrelated sizes. pm_multi_mean takes the whole list:
 * for entry k of `count`,  mean_k = (1 / numel[k]) sum_i op_k(a_k[i], b_k[i])
 * in fp32, a_k and b_k read as fp32 whatever they are stored as:
 *   PM_ADV_ABS_DIFF         |a - b|           (feature matching: a real, b fake)
 *   PM_ADV_SQ_ONE_MINUS     (1 - a)^2
 *   PM_ADV_SQ               a^2
 *   PM_ADV_HINGE_ONE_MINUS  max(1 - a, 0)
 *   PM_ADV_HINGE_ONE_PLUS   max(1 + a, 0)
 * a, b, numel, op and dtype are HOST arrays of `count` values; a[k] and b[k]
 * are device pointers to numel[k] dense elements of dtype[k] = PM_F32, PM_F16
 * or PM_BF16. b is read by PM_ADV_ABS_DIFF only (the array may be NULL when no
 * entry has that op). out is count + 1 device floats: the means, then their
 * total. A tensor is cut into chunks of pm_multi_mean_chunk() elements, one
 * workgroup a chunk, summed in a fixed order; a chunk never spans two tensors,
 * so a tensor's mean is the same bits alone and in any list, at any alignment
 * (16-byte aligned pointers take 16-byte loads). One final workgroup sums a
 * tensor's partials in ascending order in double, divides by numel in double
 * and rounds once; the total is the double means summed in list order,
 * rounded once. The table of entries travels in the kernel arguments, 64
 * entries a launch: no host-to-device copy, any count. No float atomics: every
 * output is bit-identical from run to run.
 * pm_multi_mean_backward: with c_k = grad_out[0] / (float)numel[k] (grad_out a
 * device scalar, one fp32 division), grad_b[k] = -sign(a - b) c_k for
 * PM_ADV_ABS_DIFF (0 where a = b; nothing goes to a: the reference detaches
 * the real maps, and a non-NULL grad_a[k] is an error), and grad_a[k] =
 * 2 (a - 1) c_k, 2 a c_k, -c_k where 1 - a >= 0, c_k where 1 + a >= 0 (else 0)
 * for the other four, rounded to dtype[k]. grad_a and grad_b are host arrays
 * of device pointers; a NULL entry (or a NULL array) asks for no gradient. The
 * backward reads nothing from the workspace, which may be NULL.
 * Both are asynchronous, allocate nothing and capture into a graph. Bad
 * arguments (count <= 0, a NULL array or pointer, numel <= 0, an unknown op
 * or dtype, a workspace smaller than pm_multi_mean_workspace_bytes) return
 * PM_EINVAL before any device work; the workspace query returns 0 for them. */
#define PM_ADV_ABS_DIFF 0
#define PM_ADV_SQ_ONE_MINUS 1
#define PM_ADV_SQ 2
#define PM_ADV_HINGE_ONE_MINUS 3
#define PM_ADV_HINGE_ONE_PLUS 4
int pm_multi_mean_chunk(void);
size_t pm_multi_mean_workspace_bytes(const long long* numel, int count);
int pm_multi_mean(const void* const* a, const void* const* b,
                  const long long* numel, const int* op, const int* dtype,
                  int count, float* out, void* workspace,
                  size_t workspace_bytes, void* stream);
int pm_multi_mean_backward(const void* const* a, const void* const* b,
                           const long long* numel, const int* op,
                           const int* dtype, int count, const float* grad_out,
                           void* const* grad_a, void* const* grad_b,
                           void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- optimizer step: promonet/train/core.py:335-369 ------------------------
 * The gradient statistics, the clip, the AdamW update and the update of the
 * loss scale of a training step, with no host read in between. An entry is
 * one parameter: param, exp_avg and exp_avg_sq dense fp32, grad numel[k] dense
 * elements of dtype[k] = PM_F32, PM_F16 or PM_BF16, read as stored. param,
 * exp_avg, exp_avg_sq, grad, numel and dtype are HOST arrays of `count`
 * values (device pointers where they are pointers). A tensor is cut into
 * chunks of pm_optim_chunk() elements, one workgroup a chunk, and a chunk
 * never spans two tensors; the table of entries travels in the kernel
 * arguments, pm_optim_entries_per_launch() entries a launch: no host-to-device
 * copy, any count. No float atomics: every output is bit-identical from run
 * to run.
 * pm_optim_grad_stats: over the whole list the maximum and the minimum
 * gradient, mean = sum / numel, norm = sqrt(sum of squares) (the L2 norm of
 * the concatenation) and the count of NaN and +-inf elements, which are left
 * out of the other four. The sums: fp32 inside a chunk in pm_multi_mean's
 * order, the chunks in ascending order in double, rounded once. They go to
 * `stats`, PM_OPTIM_STATS device floats indexed by PM_OPTIM_*, with the
 * step's control block:
 *   FOUND_INF  1 if the count is not 0, or found_inf (an optional device
 *              scalar, torch's protocol for fused optimizers) is not 0; else 0
 *   INV_SCALE  (float)(1.0 / (double)grad_scale[0]) of the optional device
 *              scalar grad_scale, else 1
 *   COEF       1; with clip >= 0 (a negative clip is no clip) the reference's
 *              order: if max(max, |min|) of the gradients as they are (still
 *              scaled) is above clip,  total = max(max, |min|) INV_SCALE  and
 *              COEF = min((float)clip / (total + 1e-6f), 1.f)
 * and, unless FOUND_INF, advance `state` (optional; 3 device doubles {step,
 * beta1^step, beta2^step}): step += 1 and one multiplication of each power.
 * pm_optim_adamw_step: nothing when FOUND_INF; else for every element, each
 * fp32 operation rounded on its own, / and sqrt correctly rounded,
 *   g = (grad INV_SCALE) COEF
 *   p = p (float)(1 - lr weight_decay)
 *   m = m + (float)(1 - beta1) (g - m)
 *   v = v (float)beta2 + (float)(1 - beta2) (g g)
 *   d = sqrtf(v) / (float)sqrt(1 - state[2]) + (float)eps
 *   p = p + (float)(-lr / (1 - state[1])) (m / d)
 * with the constants formed in double on the device. stats and state MUST be
 * those that one pm_optim_grad_stats call wrote for the same list just before:
 * every such call with a state advances the step (unless FOUND_INF), so one
 * statistics call goes with one update, and a second statistics call without
 * an update moves the step and the powers on (pass state = NULL for
 * statistics alone). The hyper-parameters are
 * kernel arguments: a captured graph keeps the values it was captured with.
 * pm_optim_scaler_update: torch.amp.GradScaler.update()'s rule on the device
 * scalars scale (fp32) and growth_tracker (int32): if any of the `count`
 * (1 .. 8) device scalars found_inf[k] (a HOST array) is not 0, scale *=
 * backoff and the tracker = 0; else the tracker += 1 and, when it reaches
 * growth_interval, scale *= growth (unless that is inf) and the tracker = 0.
 * The products are made in double and rounded once. Then every found_inf[k]
 * is set to 0.
 * All three are asynchronous, allocate nothing and capture into a graph. Bad
 * arguments (count <= 0, a NULL array or pointer, numel <= 0, an unknown
 * dtype, a clip, lr, beta, eps, weight_decay or factor that is not finite, a
 * beta outside [0, 1), a negative lr, eps or weight_decay, growth <= 1,
 * backoff outside (0, 1), growth_interval <= 0, a workspace smaller than
 * pm_optim_workspace_bytes) return PM_EINVAL before any device work; the
 * workspace query returns 0 for them. */
#define PM_OPTIM_MAX 0
#define PM_OPTIM_MIN 1
#define PM_OPTIM_MEAN 2
#define PM_OPTIM_NORM 3
#define PM_OPTIM_NORM_SQ 4          /* the sum of squares, rounded once */
#define PM_OPTIM_NONFINITE 5        /* the count, rounded to fp32 */
#define PM_OPTIM_FOUND_INF 6
#define PM_OPTIM_INV_SCALE 7
#define PM_OPTIM_COEF 8
#define PM_OPTIM_STATS 16
int pm_optim_chunk(void);
int pm_optim_entries_per_launch(void);
size_t pm_optim_workspace_bytes(const long long* numel, int count);
int pm_optim_grad_stats(const void* const* grad, const long long* numel,
                        const int* dtype, int count, const float* grad_scale,
                        const float* found_inf, double clip, double beta1,
                        double beta2, double* state, float* stats,
                        void* workspace, size_t workspace_bytes, void* stream);
int pm_optim_adamw_step(void* const* param, void* const* exp_avg,
                        void* const* exp_avg_sq, const void* const* grad,
                        const long long* numel, const int* dtype, int count,
                        const float* stats, const double* state, double lr,
                        double beta1, double beta2, double eps,
                        double weight_decay, void* stream);
int pm_optim_scaler_update(float* scale, int* growth_tracker,
                           float* const* found_inf, int count, double growth,
                           double backoff, int growth_interval, void* stream);

/* ---- Vocos mel vocoder engine: replaces promonet.model.Vocos --------------
 * (promonet/model/vocos.py, config/baselines/vocos.py MODEL = 'vocos').
 * conv_pre (k7) + cond, backbone embed (k7) + LayerNorm, `layers` fused
 * ConvNeXt blocks, final LayerNorm, ISTFTHead (Linear C -> n_fft + 2,
 * exp-clip magnitude, phase) and the inverse STFT with overlap-add.
 * channels must be 512, hidden a multiple of 64, n_fft 1024, hop 256,
 * features a multiple of 16. dtype PM_F32, PM_F16 or PM_BF16 is the MFMA
 * operand type of the contractions; everything else is fp32.               */
typedef struct pm_vocos_s* pm_vocos_t;
int pm_vocos_create(int num_features, int global_channels, int channels,
                    int hidden, int layers, int n_fft, int hop, int dtype,
                    pm_vocos_t* out);
int pm_vocos_destroy(pm_vocos_t h);
/* Vocos.state_dict() keys, e.g. conv_pre.weight (512, 80, 7),
 * backbone.convnext.3.pwconv1.weight (1536, 512), head.istft.window (1024) */
int pm_vocos_load_tensor(pm_vocos_t h, const char* name, const float* dev,
                         const int64_t* shape, int ndim, void* stream);
int pm_vocos_finalize(pm_vocos_t h, void* stream);
size_t pm_vocos_workspace_bytes(pm_vocos_t h, int batch, int frames);
/* Vocos.forward(x, g) (vocos.py:41-54): features (B, F, T), global
 * (Bg, G) with Bg 1 or B, or NULL (no cond); audio (B, 256 T).              */
int pm_vocos_forward(pm_vocos_t h, const float* features,
                     const float* global_features, int global_batch,
                     float* audio, int batch, int frames, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Ragged batch (no reference counterpart: the reference reconstructs one
 * file per call, promonet/baseline/mels.py:146-166): lengths (B) int32 device
 * array of valid frames, 1 <= lengths[b] <= frames; frames past an
 * utterance's end are never read, so each utterance equals its stand-alone
 * synthesis; audio is (B, 256 frames) and its tail is zero. lengths is read
 * on the device only: the call stays asynchronous and capturable.          */
size_t pm_vocos_ragged_workspace_bytes(pm_vocos_t h, int batch, int frames);
int pm_vocos_forward_ragged(pm_vocos_t h, const float* features,
                            const float* global_features, int global_batch,
                            const int* lengths, float* audio, int batch,
                            int frames, void* workspace,
                            size_t workspace_bytes, void* stream);
/* One ConvNeXtBlock (vocos.py:113-146), channels-last: x, y (B, T, 512),
 * y != x; fp32 weights as in the state dict (dwconv (C, 1, 7), pwconv1
 * (H, C), pwconv2 (C, H)); workspace: pm_convnext_block_workspace_bytes.   */
size_t pm_convnext_block_workspace_bytes(int dtype, int channels, int hidden);
int pm_convnext_block_cl(int dtype, const float* x, float* y,
                         const float* dw_w, const float* dw_b,
                         const float* ln_w, const float* ln_b,
                         const float* w1, const float* b1, const float* w2,
                         const float* b2, const float* gamma, int batch,
                         int frames, int channels, int hidden,
                         void* workspace, size_t workspace_bytes,
                         void* stream);
/* The contraction of conv_pre, embed and head.out on its own (a test entry):
 * out (B, T, N) = conv1d(x, w, padding = taps / 2) + bias (+ gbias[b], or
 * gbias[0] when gbatch is 1; NULL: none), out channels-last. x (B, T, K)
 * channels-last or, channels_first (taps 7 only), (B, K, T); w (N, K, taps)
 * fp32, packed to the operand type of `dtype` on every call; taps 1 or 7,
 * K a multiple of 16. workspace: pm_vocos_gemm_workspace_bytes.             */
size_t pm_vocos_gemm_workspace_bytes(int dtype, int taps, int in_channels,
                                     int out_channels);
int pm_vocos_gemm_cl(int dtype, int taps, int channels_first, const float* x,
                     const float* w, const float* bias, const float* gbias,
                     int gbatch, float* out, int batch, int frames,
                     int in_channels, int out_channels, void* workspace,
                     size_t workspace_bytes, void* stream);
/* ISTFTHead (vocos.py:154-172): x (B, T, 512) channels-last, w (1026, 512),
 * bias (1026), window (1024) -> audio (B, 256 T).                          */
size_t pm_vocos_head_workspace_bytes(int dtype, int batch, int frames);
int pm_vocos_head(int dtype, const float* x, const float* w,
                  const float* bias, const float* window, float* audio,
                  int batch, int frames, void* workspace,
                  size_t workspace_bytes, void* stream);
/* ISTFT (vocos.py:175-206): spectrum (B, 513, T) complex as (re, im) pairs
 * -> audio (B, 256 T); the imaginary parts of bins 0 and 512 are ignored. */
size_t pm_istft_workspace_bytes(int batch, int frames);
int pm_istft(const float* spectrum, const float* window, float* audio,
             int batch, int frames, void* workspace, size_t workspace_bytes,
             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROMONET_HIP_H */

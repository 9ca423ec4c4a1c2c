"""Float64 restatement of pm_stft_magnitude_backward's ALGORITHM (not of the
reference): reflect pad truncated to Np, framing, windowed DFT, the cotangent
g / sqrt(re^2 + im^2 + 1e-6) * (re, im), overlap-add in 128-row tiles with a
3-row halo, the three-term adjoint of the reflect pad. Switches plant the
defects a tiled kernel can have; tests/test_cpu_spectrogram_backward.py shows
that the shapes of tests/test_gpu_spectrogram_backward.py reject them and
that the shapes the suite had before (T = 24, 9, 31) do not.

Also here, shared by the CPU and the GPU file: the shapes, the seeded inputs,
the float64 autograd reference and the support of one frame in the audio."""
import math

import torch

import restatement as oracle

NFFT, HOP, BINS, PAD = 1024, 256, 513, 384
TILE = 128            # columns (frames / padded rows) per conv workgroup
ROWS = 1088           # 2 * 513 (re, im) rows padded to 17 M blocks of 64

LONG = (3, HOP * 300 + 77)
# EPI 3 tile edge | overlap-add tile edge (T + 3 = 127, 128, 129) | three
# tiles x 17 / 4 M blocks x three utterances, ragged | the shortest lengths
LINEAR_SHAPES = (
    (1, HOP * 127), (1, HOP * 128), (1, HOP * 129),
    (2, HOP * 124), (2, HOP * 125), (2, HOP * 126 + 5),
    LONG,
    (2, 385), (2, 511), (2, 512), (2, 640))
# what test_spectrogram_backward (tests/test_gpu_model.py) runs
OLD_SHAPES = ((2, HOP * 24), (1, HOP * 9 + 100), (3, HOP * 31))
MEL_SHAPES = ((2, HOP * 255), (2, HOP * 256), (2, HOP * 257), (2, HOP * 300))
SILENT_UTTERANCE = 2
ZERO_STRETCH = (0, 30000, 30000 + 4096)    # utterance, first, past the last

TILE_DEFECTS = ('halo_dropped', 'wrong_tile')
DEFECTS = TILE_DEFECTS + (
    'left_mirror_skips_pad', 'right_mirror_untruncated',
    'right_mirror_at_last', 'padding_rows_live')


CEILING = 2e-5        # on e, from test_spectrogram_backward


def draw_case(batch, samples, channels, seed):
    gen = torch.Generator().manual_seed(
        1000003 * seed + 7919 * batch + samples + channels)
    audio = torch.randn(batch, 1, samples, generator=gen) * .1
    weight = torch.randn(batch, channels, samples // HOP, generator=gen)
    if (batch, samples) == LONG:
        audio[SILENT_UTTERANCE] = 0.
        item, first, last = ZERO_STRETCH
        audio[item, 0, first:last] = 0.
    return audio, weight


def fp32_floor(audio, weight):
    """What ANY float32 evaluation can be off by, in the metric e. The
    cotangent g X / sqrt(|X|^2 + 1e-6) moves by |g| / sqrt(|X|^2 + 1e-6) per
    unit of X, and a float32 DFT of frame t is uncertain by 2^-24 sum_n
    |x_n w_n|: a bin that cancels to |X| ~ 1e-3 under a large weight (the
    real bins 0 and 512 do so most often) carries the forward's rounding into
    the gradient x 1000. A silent frame has nothing to round."""
    a = audio.double().reshape(audio.shape[0], 1, -1)
    padded = torch.nn.functional.pad(a, (PAD, PAD), mode='reflect')[:, 0]
    window = torch.hann_window(NFFT, dtype=torch.float64)
    mass = (padded.abs().unfold(-1, NFFT, HOP) * window).sum(-1)   # (B, T)
    reference, spec = reference_gradient(audio, weight)
    worst = (weight.double().abs() * 2. ** -24 * mass[:, None] / spec).max()
    return worst.item() / max(1., reference.abs().max().item())


def make_case(batch, samples, channels=BINS, seed=0):
    """Seeded audio (B, 1, N) float32 `randn * .1` and loss weight (B, C, T).
    The LONG batch carries the silence: one all-zero utterance and a stretch
    of exact zeros in another. A linear case is drawn again (next seed) until
    the ceiling can be asked of float32 at all: fp32_floor <= CEILING."""
    while True:
        audio, weight = draw_case(batch, samples, channels, seed)
        if channels != BINS or fp32_floor(audio, weight) <= CEILING:
            return audio, weight
        seed += 1


def reference_graph(audio, mels=False, threshold=None):
    """float64 leaf (B, 1, N) and the oracle's torch.stft spectrogram of it,
    (B, C, T) with the batch axis kept."""
    leaf = audio.double().clone().requires_grad_(True)
    spec = oracle.spectrogram(leaf, mels=mels, threshold=threshold)
    return leaf, spec.reshape(audio.shape[0], -1, audio.shape[-1] // HOP)


def reference_gradient(audio, weight, mels=False, threshold=None):
    """float64 autograd through the oracle: d sum(spec * weight) / d audio,
    (B, N), and the spectrogram (B, C, T)."""
    leaf, spec = reference_graph(audio, mels, threshold)
    grad, = torch.autograd.grad(spec, leaf, weight.double())
    return grad[:, 0], spec.detach()


ONE_HOT_BINS = (0, 1, 256, 512)
ONE_HOT_FRAMES = (0, 127, 128, 299)
ONE_HOT_UTTERANCE = 1


def one_hot(shape, item, channel, frame, dtype=torch.float32):
    weight = torch.zeros(shape, dtype=dtype)
    weight[item, channel, frame] = 1.
    return weight


def zero_mismatches(ours, reference):
    """Samples where the float64 gradient is exactly zero and ours is not."""
    return int(((reference.cpu() == 0) & (ours.cpu() != 0)).sum())


def clamp_threshold(mel, low=-2.7, high=-2.3):
    """A log-mel clamp threshold that no element sits on: the middle of the
    widest gap between neighbouring float64 values inside [low, high] (the
    median of these cases is -2.54), and half that gap. A float32 forward
    within that margin of float64 clamps the same elements."""
    values = mel.detach().double().flatten()
    values = values[(values > low) & (values < high)].sort().values
    gaps = values[1:] - values[:-1]
    at = int(gaps.argmax())
    return float(values[at] + gaps[at] / 2), float(gaps[at] / 2)


def reference_gradient_dft(audio, weight):
    """The same through oracle.spectrogram_dft (an independent framing)."""
    leaf = audio.double().clone().requires_grad_(True)
    (oracle.spectrogram_dft(leaf) * weight.double()).sum().backward()
    return leaf.grad[:, 0]


def _basis(rows_live):
    """(rows, 1024) float64, row 2 bin + part: hann(n) cos | -hann(n) sin
    (pm_dft_basis_kernel; the formula of oracle.spectrogram_dft). Rows at or
    above `rows_live` are the zero padding of the last M block."""
    window = torch.hann_window(NFFT, dtype=torch.float64)
    n = torch.arange(NFFT, dtype=torch.float64)
    k = torch.arange(ROWS // 2, dtype=torch.float64)
    angle = 2 * math.pi * k[:, None] * n[None] / NFFT
    basis = torch.stack(
        (window * torch.cos(angle), -window * torch.sin(angle)), 1)
    basis = basis.reshape(ROWS, NFFT)
    basis[rows_live:] = 0.
    return basis


def restated_gradient(audio, weight, defect=None):
    """audio (B, 1, N), weight (B, 513, T) -> d sum(|STFT| weight) / d audio
    (B, N) float64, computed the way the kernels compute it. `defect` plants
    one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    a = audio.double().reshape(audio.shape[0], -1)
    batch, samples = a.shape
    frames = samples // HOP
    kept = (frames + 3) * HOP               # Np <= N + 2 pad
    # pm_reflect_pad_kernel
    j = (torch.arange(kept) - PAD).abs()
    j = torch.where(j >= samples, 2 * (samples - 1) - j, j)
    padded = a[:, j]
    # EPI 3 launch: the framed DFT, then the cotangent, (B, T, 1088). Rows at
    # or above 2 * 513 are masked by `bin < a.bins` and zero in the basis.
    # 'padding_rows_live' treats the 1088 rows as 544 bins: no mask, no zero
    # rows, so bin 513 + k reads its gradient where the flat (B, 513, T)
    # buffer continues - bin k of the next utterance.
    live = ROWS if defect == 'padding_rows_live' else 2 * BINS
    basis = _basis(live)
    x = torch.einsum('btn,mn->btm', padded.unfold(-1, NFFT, HOP), basis)
    re, im = x[..., 0::2], x[..., 1::2]
    flat = torch.cat((
        weight.double().reshape(-1),
        torch.zeros((ROWS // 2 - BINS) * frames, dtype=torch.float64)))
    at = (torch.arange(batch)[:, None, None] * BINS * frames +
          torch.arange(ROWS // 2)[None, None, :] * frames +
          torch.arange(frames)[None, :, None])
    g = flat[at]                                        # (B, T, 544)
    g[..., live // 2:] = 0.
    scale = g / torch.sqrt(re * re + im * im + 1e-6)
    cot = torch.stack((scale * re, scale * im), -1).reshape(
        batch, frames, ROWS)
    if defect == 'wrong_tile':
        # the tile index is lost on the way in: every tile computes tile 0's
        # frames and writes them to its own columns
        cot = cot[:, torch.arange(frames) % TILE]
    # overlap-add launch: padded row q = t + s receives frame t's samples
    # 256 s .. 256 s + 255; a 128-row tile stages frames q0 - 3 .. q0 + 127
    spread = torch.einsum('btm,mn->btn', cot, basis)
    t = torch.arange(frames)
    gpad = torch.zeros(batch, frames + 3, HOP, dtype=torch.float64)
    for s in range(NFFT // HOP):
        part = spread[..., s * HOP:(s + 1) * HOP]
        if defect == 'halo_dropped':
            same_tile = ((t + s) // TILE == t // TILE).double()
            part = part * same_tile[None, :, None]
        gpad[:, s:s + frames] += part
    # pm_reflect_pad_adjoint_kernel on the flat (B, Np) buffer
    flat = torch.cat((gpad.reshape(-1), torch.zeros(2 * PAD + 1).double()))
    i = torch.arange(samples)
    base = torch.arange(batch)[:, None] * kept
    own = i + PAD
    result = torch.where(own < kept, flat[base + own.clamp(max=kept)], 0.)
    left_last = PAD - 1 if defect == 'left_mirror_skips_pad' else PAD
    left = (i >= 1) & (i <= left_last)
    result = result + torch.where(left, flat[base + (PAD - i).clamp(min=0)], 0.)
    mirror = 2 * (samples - 1) - i + PAD
    last = samples - 1 if defect == 'right_mirror_at_last' else samples - 2
    right = (i <= last) & (mirror < samples + 2 * PAD)
    if defect != 'right_mirror_untruncated':
        right = right & (mirror < kept)
    mirror = torch.where(right, mirror, 0)
    return result + torch.where(right, flat[base + mirror], 0.)


def frame_support(samples, frame):
    """Boolean (N): the audio samples that frame `frame` reads with a non-zero
    window - its padded samples 256 t + 1 .. 256 t + 1023 (hann(0) == 0),
    folded back through the reflection."""
    k = torch.arange(frame * HOP + 1, frame * HOP + NFFT)
    j = (k - PAD).abs()
    j = torch.where(j >= samples, 2 * (samples - 1) - j, j)
    support = torch.zeros(samples, dtype=torch.bool)
    support[j] = True
    return support


def relative_error(ours, reference):
    """e = max|ours - ref64| / max(1, max|ref64|)"""
    reference = reference.double().cpu()
    error = (ours.double().cpu() - reference).abs().max().item()
    return error / max(1., reference.abs().max().item())

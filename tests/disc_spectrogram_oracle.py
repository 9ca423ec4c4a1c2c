"""The project's own statement of the three discriminator spectrograms, in
torch on the CPU in float64, with gradients by autograd: the yardstick of
test_gpu_disc_spectrogram.py, pinned to the reference's own methods by
scripts/make_golden_disc_spectrogram.py (tests/golden/disc_spectrogram.pt).

Written from the formulas:
  R    reflect pad (n_fft - hop) / 2, frames not centred, a window of `win`
       ones centred in n_fft zeros, |X| as (B, 1, bins, frames);
  CMB  the same with n_fft = win = 1024, hop 256, |X| as (B, 1, frames, bins)
       cut into bands [..., b0:b1];
  DB   reflect pad n_fft / 2, torch.hann_window(win) (periodic, computed in
       fp32 as the reference computes it), d = 20 log10 max(|X|, 1e-5) and
       max(d, amax(d over the WHOLE batch) - 80), (B, bins, frames).

Every function takes `defect`, the name of one planted mistake (DEFECTS):
test_cpu_disc_spectrogram.py shows that the comparison of the GPU tests
rejects each of them at the shapes the GPU tests use.

The error model is that of the spectral-convergence loss:
delta = 2^-24 log2(N) |windowed frame|_2 per frame.
"""
import functools
import math

import torch

AMIN, TOP_DB = 1e-5, 80.
SLOPE = 20. / math.log(10.)
EPS = 2. ** -24
FRAGILE = 64.           # the width of the fragile bands, in units of delta
DEFAULT_EDGES = ((0, 51), (51, 128), (128, 256), (256, 384), (384, 513))

DEFECTS = (
    'pad_off_by_one', 'pad_half', 'window_left', 'window_hann',
    'row_maximum', 'floor_gradient_dropped', 'band_edge', 'swapped_axes',
    'right_margin_not_folded')


###############################################################################
# The transform
###############################################################################


def window_table(kind, win_length, fft_size, left_aligned=False):
    """`kind` window of win_length centred in fft_size zeros, float64"""
    if kind == 'ones':
        window = torch.ones(win_length, dtype=torch.float64)
    else:
        window = torch.hann_window(win_length).double()
    left = 0 if left_aligned else (fft_size - win_length) // 2
    table = torch.zeros(fft_size, dtype=torch.float64)
    table[left:left + win_length] = window
    return table


def reflect(x, pad, fold_right=True):
    """(B, T) -> (B, T + 2 pad), the margins as mirror images without the
    edge sample; fold_right=False cuts the right margin out of the graph"""
    samples = x.shape[-1]
    left = x[:, 1:pad + 1].flip(-1)
    right = x[:, samples - 1 - pad:samples - 1].flip(-1)
    if not fold_right:
        right = right.detach()
    return torch.cat([left, x, right], -1)


def margin(kind, fft_size, hop_size, defect=None):
    pad = fft_size // 2 if kind == 'DB' else int((fft_size - hop_size) / 2)
    if defect == 'pad_off_by_one':
        pad += 1
    if defect == 'pad_half' and kind != 'DB':
        pad = fft_size // 2
    return pad


def windowed_frames(x, kind, sizes, defect=None):
    """(B, T) float64 -> (B, frames, fft_size), windowed"""
    fft_size, hop_size, win_length = sizes
    pad = margin(kind, fft_size, hop_size, defect)
    name = 'hann' if kind == 'DB' or defect == 'window_hann' else 'ones'
    table = window_table(
        name, win_length, fft_size, left_aligned=defect == 'window_left')
    padded = reflect(x, pad, defect != 'right_margin_not_folded')
    return padded.unfold(-1, fft_size, hop_size) * table


def transform(x, kind, sizes, defect=None):
    """One-sided spectrum (B, bins, frames), complex128"""
    return torch.fft.rfft(
        windowed_frames(x, kind, sizes, defect), dim=-1).transpose(1, 2)


def flat(x):
    return (x[:, 0] if x.ndim == 3 else x).double()


###############################################################################
# The three methods
###############################################################################


def resolution(x, sizes, defect=None):
    """DiscriminatorR.spectrogram -> (B, 1, bins, frames)"""
    return transform(flat(x), 'R', sizes, defect).abs()[:, None]


def multiband(x, window_length=1024, hop_size=256, edges=DEFAULT_EDGES,
              defect=None):
    """DiscriminatorCMB.spectrogram -> list of (B, 1, frames, b1 - b0)"""
    magnitude = transform(
        flat(x), 'CMB', (window_length, hop_size, window_length),
        defect).abs()[:, None]
    if defect != 'swapped_axes':
        magnitude = magnitude.permute(0, 1, 3, 2)
    if defect == 'band_edge':
        edges = [(low + (low > 0), high + (high < edges[-1][1]))
                 for low, high in edges]
    return [magnitude[..., low:high] for low, high in edges]


def amplitude_to_db(x, multiplier=20, amin=AMIN, db_multiplier=0.,
                    top_db=TOP_DB, defect=None):
    """The published formula of torchaudio.functional.amplitude_to_DB for a
    3-D input, which it reads as (channel, freq, time): one maximum for the
    whole tensor. (torchaudio is not on the build host: unpinned.)"""
    x_db = multiplier * torch.log10(torch.clamp(x, min=amin))
    x_db = x_db - multiplier * db_multiplier
    if defect == 'row_maximum':
        floor = x_db.amax(dim=(-2, -1), keepdim=True) - top_db
    else:
        floor = x_db.amax() - top_db
    if defect == 'floor_gradient_dropped':
        floor = floor.detach()
    return torch.maximum(x_db, floor)


def decibel(x, sizes, defect=None):
    """SpecDiscriminatorBase.spectrogram -> (B, bins, frames)"""
    return amplitude_to_db(
        transform(flat(x), 'DB', sizes, defect).abs(), defect=defect)


def output(kind, x, sizes, defect=None):
    """The method's output as ONE tensor (CMB: the bands side by side)"""
    if kind == 'R':
        return resolution(x, sizes, defect)
    if kind == 'CMB':
        return torch.cat(multiband(x, sizes[0], sizes[1], defect=defect), -1)
    return decibel(x, sizes, defect)


def gradient(kind, x, sizes, upstream, defect=None):
    """d <upstream, output> / d x by autograd, float64, in x's shape"""
    leaf = x.double().clone().requires_grad_(True)
    out = output(kind, leaf, sizes, defect)
    out.backward(upstream.double().reshape(out.shape))
    return leaf.grad


###############################################################################
# Error model
###############################################################################


def delta(x, kind, sizes):
    """2^-24 log2(N) |windowed frame|_2 per frame, (B, 1, frames)"""
    frames = windowed_frames(flat(x), kind, sizes)
    return (EPS * math.log2(sizes[0]) * frames.norm(dim=-1))[:, None]


def fragile(kind, x, sizes):
    """Bins (B, bins, frames) where fp32 rounding may change the answer
    discontinuously: |X| within FRAGILE delta of 0 (the phase of the bin
    gradient) and, for DB, of 1e-5 (the clamp), and d within the propagated
    error of the floor (the error of the element plus that of the maximum)."""
    X = transform(flat(x), kind, sizes).abs()
    d = delta(x, kind, sizes)
    out = X <= FRAGILE * d
    if kind == 'DB':
        out |= (X - AMIN).abs() <= FRAGILE * d
        unit = SLOPE * d / X.clamp(min=AMIN)
        x_db = 20. * torch.log10(X.clamp(min=AMIN))
        top = x_db.flatten().argmax()
        floor = x_db.flatten()[top] - TOP_DB
        out |= (x_db - floor).abs() <= FRAGILE * (unit + unit.flatten()[top])
    return out


###############################################################################
# The cases of the tests, their inputs and their figures
###############################################################################

# name: (kind, (n_fft, hop, win), T)
CASES = {
    'R-512': ('R', (512, 50, 240), 700),
    'R-1024': ('R', (1024, 120, 600), 1600),
    'R-2048': ('R', (2048, 240, 1200), 2500),
    'CMB': ('CMB', (1024, 256, 1024), 2300),
    'DB-64': ('DB', (64, 16, 64), 1000),
    'DB-256': ('DB', (256, 64, 256), 1500),
    'DB-2048': ('DB', (2048, 512, 2048), 3000),
}
FRAMES = {'R-512': 14, 'R-1024': 13, 'R-2048': 10, 'CMB': 8, 'DB-64': 63,
          'DB-256': 24, 'DB-2048': 6}
BATCH, SIGMA, QUIET = 2, .1, 3e-4
# (DB-2048: a seed whose row 0 has no bin 80 dB under its own maximum)
SEEDS = {'R-512': 40, 'R-1024': 41, 'R-2048': 42, 'CMB': 43, 'DB-64': 44,
         'DB-256': 45, 'DB-2048': 47}


def inputs(name):
    """(B, T) fp32: Gaussian, sigma 0.1; DB: row 1 scaled by 3e-4"""
    kind, _, samples = CASES[name]
    generator = torch.Generator().manual_seed(SEEDS[name])
    x = SIGMA * torch.randn(BATCH, samples, generator=generator)
    if kind == 'DB':
        x[1] *= QUIET
    return x


def layout(kind, tensor):
    """(B, bins, frames) statistics in the layout of the kind's output"""
    if kind == 'R':
        return tensor[:, None]
    if kind == 'CMB':
        return tensor.transpose(1, 2)[:, None]
    return tensor


@functools.lru_cache(maxsize=None)
def truth(name):
    """Everything the float64 oracle says about a case, computed once. The
    random upstream gradient is zero on the fragile bins: what they pass to
    grad_x is not defined to fp32 accuracy."""
    kind, sizes, _ = CASES[name]
    x = inputs(name)
    out = output(kind, x, sizes)
    weak = layout(kind, fragile(kind, x, sizes))
    d = layout(kind, delta(x, kind, sizes))
    X = layout(kind, transform(flat(x), kind, sizes).abs())
    unit = SLOPE * d / X.clamp(min=AMIN) if kind == 'DB' else d.expand_as(X)
    generator = torch.Generator().manual_seed(SEEDS[name] + 100)
    upstream = torch.randn(out.shape, generator=generator)
    upstream[weak] = 0.
    start = torch.randn(x.shape, generator=generator)
    return {'x': x, 'out': out, 'fragile': weak, 'unit': unit,
            'upstream': upstream, 'start': start,
            'gradient': gradient(kind, x, sizes, upstream)}


def figure_forward(name, got):
    """The largest error of a non-fragile element, in units of the model:
    delta for R and CMB, (20 / ln 10) delta / |X| for DB"""
    want = truth(name)
    keep = ~want['fragile']
    error = (got.double().reshape(want['out'].shape) - want['out']).abs()
    return (error[keep] / want['unit'][keep]).max().item()


def figure_gradient(name, got, want=None):
    """The largest relative L2 error of a row of grad_x, over 2^-24 log2 N"""
    want = truth(name)['gradient'] if want is None else want
    got = got.double().reshape(want.shape)
    relative = (got - want).norm(dim=-1) / want.norm(dim=-1)
    return relative.max().item() / (EPS * math.log2(CASES[name][1][0]))


###############################################################################
# The reference's own arithmetic in fp32: torch.stft and the torch ops of the
# three methods (the figures behind the gates of the GPU tests)
###############################################################################


def torch_fp32(kind, x, sizes):
    fft_size, hop_size, win_length = sizes
    x = x.float()
    if kind == 'DB':
        X = torch.stft(
            x, fft_size, hop_size, win_length,
            window=torch.hann_window(win_length), return_complex=True)
        return amplitude_to_db(X.abs())
    pad = int((fft_size - hop_size) / 2)
    padded = torch.nn.functional.pad(x[:, None], (pad, pad), 'reflect')[:, 0]
    X = torch.stft(
        padded, fft_size, hop_size, win_length,
        window=torch.ones(win_length), center=False, return_complex=True)
    magnitude = torch.view_as_real(X).norm(p=2, dim=-1)[:, None]
    return magnitude.permute(0, 1, 3, 2) if kind == 'CMB' else magnitude


@functools.lru_cache(maxsize=None)
def fp32_figures(name):
    """(forward, gradient) figures of the fp32 torch arithmetic on a case"""
    kind, sizes, _ = CASES[name]
    want = truth(name)
    leaf = want['x'].clone().requires_grad_(True)
    out = torch_fp32(kind, leaf, sizes)
    out.backward(want['upstream'].reshape(out.shape))
    return (figure_forward(name, out.detach()),
            figure_gradient(name, leaf.grad))


###############################################################################
# The gates of test_gpu_disc_spectrogram.py
###############################################################################

# The figures of fp32_figures on the build host, (forward, gradient) per case
# (DESIGN section 19 lists them beside the device's)
FP32_RECORDED = {
    'R-512': (0.839, 0.414), 'R-1024': (0.743, 0.383),
    'R-2048': (0.919, 0.445), 'CMB': (0.719, 0.389),
    'DB-64': (3.870, 152.809), 'DB-256': (3.208, 218.901),
    'DB-2048': (1.881, 25.888)}


def family(name):
    return 'DB' if CASES[name][0] == 'DB' else 'magnitude'


# K = 4 x the largest recorded figure of a family (R and CMB compute one
# quantity, |X|, under one model; DB another): (forward, gradient)
GATES = {
    which: tuple(
        4. * max(FP32_RECORDED[name][i] for name in CASES
                 if family(name) == which) for i in range(2))
    for which in ('magnitude', 'DB')}


def gate(name, direction):
    return GATES[family(name)][direction == 'gradient']

"""Planted inf and NaN on top of the float64 oracles the suite already has:
what a training kernel must do with a non-finite value, so that an overflow
reaches the optimizer's scaler as torch's own ops would carry it.

No arithmetic of its own. A plant writes ONE value of VALUES into ONE element
of a case's floating-point input or upstream gradient (never into a length, an
index or a table), the family's oracle runs on the clean and on the planted
inputs, and every output (forward, gx, gW, gb, or a loss and its gradients)
falls into three sets (`masks`):
  BAD      non-finite in the planted truth;
  CLEAN    planted truth == clean truth, elementwise in float64;
  CHANGED  the rest: finite but different (what relu(-inf) = 0 does downstream).
The GPU tests (test_gpu_nonfinite.py) hold the device to: the same BAD mask
exactly (inf against NaN is not told apart: a sum of two infinities may be
either), the same bits as its own clean run on CLEAN, the family's existing
gate on CHANGED. test_cpu_nonfinite.py checks the table itself.

The families here: the multi-tensor mean of the adversarial losses, the
FARGAN discriminator's frequency conv layers at both strides and their weight
norm, the three
discriminator spectrograms, and loss.stft / SpectralConvergence / loss.signal.

Plant sites: an upstream plant is interior (at least the layer's reach from
every border of its row), so that no BAD element owes its non-finiteness to a
product with a padding zero; an input plant may sit on a border, and one sits
on the last pixel (sample) of batch row 0. No family here needs FREE elements
for a window's zeros: the transforms multiply every sample by its window
entry, a zero included, as the oracles do.

TWO OUTCOMES. An infinite SAMPLE goes through an FFT, and whether a bin comes
out as +-inf or as NaN (inf - inf) depends on the FFT's factorisation:
torch.fft.rfft in float64 gave NaN bins on one CPU and none on another for the
same frame. Where only "BAD" is asked that does not matter. It decides a whole
tensor in two places, both through a reduction over the batch: the decibel
spectrogram's gradient (amax of +inf floors every element and the gradient is
0 everywhere; amax of NaN makes it NaN everywhere) and the spectral-
convergence gradient under an infinite TARGET sample (sum s_y = inf scales
every element to 0, NaN to NaN). For these two gradients (`two_outcomes`) the
truth on a given CPU is one of exactly two tensors, all BAD or all zero, and
the device is held to being one of the two, whole; test_cpu_nonfinite.py
asserts that the truth is. No element of any output is free.
"""
import functools
import math

import torch

import adversarial_oracle
import disc_spectrogram_oracle
import fdisc_oracle
import fdisc_strided_oracle
import losses_oracle

NAN, INF = float('nan'), float('inf')
VALUES = {'nan': NAN, 'inf': INF, '-inf': -INF}
EPS = 2. ** -24


def plant(tensor, index, value):
    out = tensor.clone()
    out[index] = value
    return out


def masks(clean, planted):
    """BAD, CLEAN, CHANGED of one output, bool in its shape"""
    clean, planted = clean.double(), planted.double()
    bad = ~torch.isfinite(planted)
    same = (planted == clean) & ~bad
    return {'bad': bad, 'clean': same, 'changed': ~bad & ~same}


def two_outcomes(family, case, where, value):
    """The outputs of a plant that are all BAD or all zero, whichever the
    transform's own additions make of an infinite sample (the docstring)"""
    if not math.isinf(value):
        return ()
    if family == 'spectrogram' and where == 'x' and \
            disc_spectrogram_oracle.family(case) == 'DB':
        return ('gx',)
    if family == 'loss' and case == 'spectral_convergence' and where == 'y':
        return ('gx',)
    return ()


def is_one_of_the_two(tensor):
    """all BAD, or all zero"""
    tensor = tensor.double()
    return bool((~torch.isfinite(tensor)).all()) or bool((tensor == 0.).all())


###############################################################################
# The multi-tensor mean (adversarial_oracle.term / derivative / multi_mean)
###############################################################################

ADV_DTYPES = {'fp32': torch.float32, 'f16': torch.float16,
              'bf16': torch.bfloat16}


def adversarial_sizes(chunk):
    """One element, a chunk less one, a chunk and a ragged tail: one list"""
    return (1, chunk - 1, chunk + 3)


@functools.lru_cache(maxsize=None)
def adversarial_inputs(op, dtype, chunk):
    """(a, b): lists of Gaussian tensors (b None but for ABS_DIFF)"""
    a, b = [], []
    for index, numel in enumerate(adversarial_sizes(chunk)):
        seed = 700 + 10 * op + 2 * index
        a.append(adversarial_oracle.gaussian((numel,), seed, dtype))
        b.append(adversarial_oracle.gaussian((numel,), seed + 1, dtype)
                 if op == adversarial_oracle.ABS_DIFF else None)
    return tuple(a), tuple(b)


def adversarial_plants(op, chunk):
    """(which list, tensor, element): the lone element, the last element of
    the first chunk's neighbour (a full chunk's ragged tail), in a; in b too
    for ABS_DIFF"""
    sites = [('a', 0, 0), ('a', 1, chunk - 2), ('a', 2, chunk + 1)]
    if op == adversarial_oracle.ABS_DIFF:
        sites.append(('b', 2, chunk + 1))
    return sites


def adversarial_outputs(op, a, b):
    """means (K), total and the gradient of the total: of b for ABS_DIFF, of
    a otherwise, one tensor a list entry"""
    ops = (op,) * len(a)
    means, total = adversarial_oracle.multi_mean(ops, list(a), list(b))
    out = {'means': means, 'total': total.reshape(1)}
    for index, tensor in enumerate(a):
        other = None if b[index] is None else b[index].double()
        out[f'gradient{index}'] = adversarial_oracle.derivative(
            op, tensor.double(), other) / tensor.numel()
    return out


def adversarial_case(op, dtype, chunk, site, value):
    """(inputs (a, b), clean truth, planted inputs, planted truth)"""
    a, b = adversarial_inputs(op, dtype, chunk)
    which, index, element = site
    planted_a, planted_b = list(a), list(b)
    target = planted_a if which == 'a' else planted_b
    target[index] = plant(target[index], element, value)
    return ((a, b), adversarial_outputs(op, a, b),
            (tuple(planted_a), tuple(planted_b)),
            adversarial_outputs(op, planted_a, planted_b))


###############################################################################
# The frequency conv layer (fdisc_oracle.layer / layer_backward)
###############################################################################

FDISC_CASES = ('first', 'd16', 'last', 'large')
FDISC_QUANTITIES = fdisc_oracle.QUANTITIES


def embedding_table(bins):
    """(bins, 2) = sin, cos of 2 pi f / bins with the values the device's
    fp32 table holds (the reference's own expression in fp32), for the clean
    and the planted truth alike. An input plant changes the ReLU gates of the
    pixels it reaches, and the embedding's weight gradient adds their
    upstream times sin or cos of a tap's row. Times 1.2e-16 (sin pi in
    float64) that change is absorbed by the float64 sum and the element would
    count as CLEAN, while fp32 holds -8.7e-8 there, which an fp32 sum of a
    few hundred terms does not absorb; with fp32's values the float64 sum
    keeps the change and the element is CHANGED, as it is on the device."""
    args = torch.arange(0, bins, dtype=torch.float32) * torch.pi * 2 / bins
    return torch.stack((torch.sin(args), torch.cos(args)), dim=1)


def fdisc_sites(name):
    """where -> index. The input on the last pixel of batch row 0 (the conv
    kernel's tile that holds it crosses into row 1) and inside row 1; the
    upstream inside row 1, the layer's reach (d bins, one frame) from every
    border"""
    channels, out_channels, bins, frames, dilation, _ = \
        fdisc_oracle.CASES[name]
    assert bins > 2 * dilation and frames > 2
    inside = (bins // 2, frames // 2)
    assert dilation <= inside[0] < bins - dilation
    assert 1 <= inside[1] < frames - 1
    # the output channel that is largest there: its ReLU is open in any
    # arithmetic and the plant gets through
    y = fdisc_oracle.truth(name)['forward'][(1, slice(None)) + inside]
    open_channel = int(y.argmax())
    assert y[open_channel] > .01
    return {
        'x-last-pixel': ('x', (0, channels - 1, bins - 1, frames - 1)),
        'x-inside': ('x', (1, min(5, channels - 1)) + inside),
        'upstream-inside': ('upstream', (1, open_channel) + inside),
    }


def fdisc_field(name, index):
    """The pixels (row, bins, frames) a tap of the layer links to pixel
    `index`, from the geometry alone: bool (B, F, T)"""
    _, _, bins, frames, dilation, _ = fdisc_oracle.CASES[name]
    row, _, f, t = index
    out = torch.zeros(fdisc_oracle.BATCH, bins, frames, dtype=torch.bool)
    for kf in (-1, 0, 1):
        for kt in (-1, 0, 1):
            ff, tt = f + kf * dilation, t + kt
            if 0 <= ff < bins and 0 <= tt < frames:
                out[row, ff, tt] = True
    return out


def fdisc_outputs(name, where=None, index=None, value=None):
    _, _, _, _, dilation, activation = fdisc_oracle.CASES[name]
    want = fdisc_oracle.truth(name)
    tensors = {key: want[key] for key in ('x', 'weight', 'bias', 'upstream')}
    if where is not None:
        tensors[where] = plant(tensors[where], index, value)
    table = embedding_table(tensors['x'].shape[2])
    y = fdisc_oracle.layer(
        tensors['x'], tensors['weight'], tensors['bias'], dilation, activation,
        table=table)
    gx, gw, gb = fdisc_oracle.layer_backward(
        tensors['x'], tensors['weight'], y, tensors['upstream'], dilation,
        activation, table=table)
    return tensors, {'forward': y, 'gx': gx, 'gW': gw, 'gb': gb}


@functools.lru_cache(maxsize=None)
def fdisc_clean(name):
    return fdisc_outputs(name)


def fdisc_case(name, site, value):
    where, index = fdisc_sites(name)[site]
    return fdisc_clean(name) + fdisc_outputs(name, where, index, value)


###############################################################################
# The discriminator spectrograms (disc_spectrogram_oracle.output / gradient)
###############################################################################

SPECTROGRAM_CASES = ('R-512', 'CMB', 'DB-64')


def spectrogram_sites(name):
    """A sample inside row 0, the last sample of row 0 (it is read again by
    the reflected margin) and one upstream element of row 0, a frame inside,
    that is neither fragile nor (DB) on the floor"""
    want = disc_spectrogram_oracle.truth(name)
    samples = want['x'].shape[1]
    out = want['out']
    usable = ~want['fragile'][0]
    if disc_spectrogram_oracle.family(name) == 'DB':
        usable = usable & (out[0] > out.min())
    usable = usable.reshape(out[0].shape)
    kind = disc_spectrogram_oracle.CASES[name][0]
    frame_axis = {'R': 2, 'CMB': 1, 'DB': 1}[kind]
    frames = out[0].shape[frame_axis]
    middle = torch.zeros_like(usable)
    middle.select(frame_axis, frames // 2).fill_(True)
    spot = torch.nonzero(usable & middle)[0]
    return {
        'x-inside': ('x', (0, samples // 2 + 1)),
        'x-last-sample': ('x', (0, samples - 1)),
        'upstream-inside': ('upstream', (0,) + tuple(int(i) for i in spot)),
    }


def spectrogram_outputs(name, where=None, index=None, value=None):
    kind, sizes, _ = disc_spectrogram_oracle.CASES[name]
    want = disc_spectrogram_oracle.truth(name)
    tensors = {'x': want['x'], 'upstream': want['upstream']}
    if where is not None:
        tensors[where] = plant(tensors[where], index, value)
    return tensors, {
        'forward': disc_spectrogram_oracle.output(
            kind, tensors['x'], sizes).detach(),
        'gx': disc_spectrogram_oracle.gradient(
            kind, tensors['x'], sizes, tensors['upstream'])}


@functools.lru_cache(maxsize=None)
def spectrogram_clean(name):
    return spectrogram_outputs(name)


def spectrogram_case(name, site, value):
    where, index = spectrogram_sites(name)[site]
    return spectrogram_clean(name) + \
        spectrogram_outputs(name, where, index, value)


def frames_of(sample, samples, fft_size, hop_size, pad, frames):
    """The frames whose fft_size samples hold `sample` of a row, the reflected
    margins of `pad` counted: from the geometry alone"""
    positions = {sample + pad}
    if 1 <= sample <= pad:
        positions.add(pad - sample)
    if samples - 1 - pad <= sample <= samples - 2:
        positions.add(pad + 2 * (samples - 1) - sample)
    return sorted(f for f in range(frames) if any(
        f * hop_size <= p < f * hop_size + fft_size for p in positions))


def samples_of(frame, samples, fft_size, hop_size, pad):
    """The samples of a row that frame `frame` holds, reflected ones
    included: bool (samples)"""
    out = torch.zeros(samples, dtype=torch.bool)
    for position in range(frame * hop_size, frame * hop_size + fft_size):
        n = abs(position - pad)
        if n >= samples:
            n = 2 * (samples - 1) - n
        out[n] = True
    return out


def spectrogram_geometry(name):
    """(samples, n_fft, hop, pad, frames) of a case"""
    kind, sizes, samples = disc_spectrogram_oracle.CASES[name]
    return (samples, sizes[0], sizes[1],
            disc_spectrogram_oracle.margin(kind, sizes[0], sizes[1]),
            disc_spectrogram_oracle.FRAMES[name])


def loss_geometry():
    return (LOSS_SHAPE[1], LOSS_SIZES[0], LOSS_SIZES[1], LOSS_SIZES[0] // 2,
            1 + LOSS_SHAPE[1] // LOSS_SIZES[1])


###############################################################################
# loss.stft, SpectralConvergence and loss.signal (losses_oracle)
###############################################################################

LOSS_SIZES = min(losses_oracle.CONFIGURATIONS)
LOSS_SHAPE = (2, 1281)
LOSS_ENTRIES = ('stft', 'spectral_convergence', 'signal')


@functools.lru_cache(maxsize=None)
def loss_inputs():
    """x, y of the losses' tests and a Gaussian upstream gradient of stft"""
    x, y = losses_oracle.inputs(losses_oracle.NOISE_SEED, *LOSS_SHAPE)
    shape = (LOSS_SHAPE[0], LOSS_SIZES[0] // 2 + 1,
             1 + LOSS_SHAPE[1] // LOSS_SIZES[1])
    upstream = torch.randn(shape, generator=torch.Generator().manual_seed(13))
    return {'x': x, 'y': y, 'upstream': upstream}


def loss_sites(entry):
    samples = LOSS_SHAPE[1]
    sites = {'x-inside': ('x', (0, samples // 2)),
             'x-last-sample': ('x', (0, samples - 1))}
    if entry == 'stft':
        frames = 1 + samples // LOSS_SIZES[1]
        sites['upstream-inside'] = ('upstream', (0, 7, frames // 2))
    else:
        sites['y-inside'] = ('y', (0, samples // 2))
    return sites


def loss_outputs(entry, where=None, index=None, value=None):
    """x is the prediction (it carries the gradient), y the target"""
    tensors = dict(loss_inputs())
    if where is not None:
        tensors[where] = plant(tensors[where], index, value)
    x, y = tensors['x'].double(), tensors['y'].double()
    if entry == 'signal':
        return tensors, {
            'forward': losses_oracle.signal(y, x).reshape(1),
            'gx': losses_oracle.signal_gradient(y, x)}
    leaf = x.clone().requires_grad_(True)
    if entry == 'stft':
        out = losses_oracle.stft(leaf, *LOSS_SIZES)
        out.backward(tensors['upstream'].double())
    else:
        out = losses_oracle.spectral_convergence(leaf, y, *LOSS_SIZES)
        out.backward()
    return tensors, {'forward': out.detach().reshape(
        out.shape if out.ndim else (1,)), 'gx': leaf.grad}


@functools.lru_cache(maxsize=None)
def loss_clean(entry):
    return loss_outputs(entry)


def loss_case(entry, site, value):
    where, index = loss_sites(entry)[site]
    return loss_clean(entry) + loss_outputs(entry, where, index, value)


def loss_gate():
    """The relative L2 gate of a row of grad_x (test_gpu_disc_spectrogram's
    and test_gpu_losses' model): units of 2^-24 log2 N"""
    return EPS * math.log2(LOSS_SIZES[0])


###############################################################################
# Weight norm (fdisc_oracle.weight_norm / weight_norm_backward)
###############################################################################

WEIGHT_NORM_SHAPE = (16, 18, 3, 3)


@functools.lru_cache(maxsize=None)
def weight_norm_inputs():
    """g, v and the weight gradient of test_gpu_fdisc.py's first shape"""
    shape = WEIGHT_NORM_SHAPE
    generator = torch.Generator().manual_seed(shape[0] * 100 + shape[1])
    g = torch.rand(shape[0], 1, 1, 1, generator=generator) + .5
    v = torch.randn(shape, generator=generator)
    upstream = torch.randn(shape, generator=generator)
    return {'g': g, 'v': v, 'upstream': upstream}


WEIGHT_NORM_SITES = {'v': ('v', (5, 7, 1, 2)),
                     'upstream': ('upstream', (5, 7, 1, 2))}


def weight_norm_outputs(where=None, index=None, value=None):
    tensors = dict(weight_norm_inputs())
    if where is not None:
        tensors[where] = plant(tensors[where], index, value)
    grad_g, grad_v = fdisc_oracle.weight_norm_backward(
        tensors['upstream'], tensors['g'], tensors['v'])
    return tensors, {
        'forward': fdisc_oracle.weight_norm(tensors['g'], tensors['v']),
        'g_g': grad_g, 'g_v': grad_v}


@functools.lru_cache(maxsize=None)
def weight_norm_clean():
    return weight_norm_outputs()


def weight_norm_case(site, value):
    where, index = WEIGHT_NORM_SITES[site]
    return weight_norm_clean() + weight_norm_outputs(where, index, value)


###############################################################################
# The strided frequency conv layer (fdisc_strided_oracle.layer /
# layer_backward)
###############################################################################

STRIDED_CASES = ('first-even', 'two-bins', 'square', 'last', 'large')


def strided_fields(name, index, upstream):
    """The pixels a tap links to pixel `index`, from the geometry alone:
    (bool (B, F', T) of the output, whether every tap is inside) for an input
    pixel, (bool (B, F, T) of the input, ...) for an output pixel"""
    _, _, bins, frames, stride, _ = fdisc_strided_oracle.CASES[name]
    rows_out = fdisc_strided_oracle.out_bins(bins, stride)
    row, _, f, t = index
    out = torch.zeros(fdisc_strided_oracle.BATCH, bins if upstream
                      else rows_out, frames, dtype=torch.bool)
    whole = True
    if upstream:
        pairs = [(stride * f + kf - 1, bins) for kf in range(3)]
    else:
        pairs = [(source, rows_out) for _, source in
                 fdisc_strided_oracle.reaching(f, stride)]
    for other, limit in pairs:
        for kt in range(3):
            tt = t + kt - 1
            if 0 <= other < limit and 0 <= tt < frames:
                out[row, other, tt] = True
            else:
                whole = False
    return out, whole


def strided_sites(name):
    """As fdisc_sites; the upstream plant only where a pixel of the output
    has every tap inside the input map (two-bins has none)"""
    channels, _, bins, frames, stride, _ = fdisc_strided_oracle.CASES[name]
    rows_out = fdisc_strided_oracle.out_bins(bins, stride)
    sites = {
        'x-last-pixel': ('x', (0, channels - 1, bins - 1, frames - 1)),
        'x-inside': ('x', (1, min(5, channels - 1), bins // 2, frames // 2)),
    }
    inside = (rows_out // 2, frames // 2)
    if strided_fields(name, (1, 0) + inside, True)[1]:
        y = fdisc_strided_oracle.truth(name)['forward'][
            (1, slice(None)) + inside]
        open_channel = int(y.argmax())
        assert y[open_channel] > .01
        sites['upstream-inside'] = ('upstream', (1, open_channel) + inside)
    return sites


def strided_outputs(name, where=None, index=None, value=None):
    _, _, _, _, stride, activation = fdisc_strided_oracle.CASES[name]
    want = fdisc_strided_oracle.truth(name)
    tensors = {key: want[key] for key in ('x', 'weight', 'bias', 'upstream')}
    if where is not None:
        tensors[where] = plant(tensors[where], index, value)
    table = embedding_table(tensors['x'].shape[2])
    y = fdisc_strided_oracle.layer(
        tensors['x'], tensors['weight'], tensors['bias'], stride, activation,
        table=table)
    gx, gw, gb = fdisc_strided_oracle.layer_backward(
        tensors['x'], tensors['weight'], y, tensors['upstream'], stride,
        activation, table=table)
    return tensors, {'forward': y, 'gx': gx, 'gW': gw, 'gb': gb}


@functools.lru_cache(maxsize=None)
def strided_clean(name):
    return strided_outputs(name)


def strided_case(name, site, value):
    where, index = strided_sites(name)[site]
    return strided_clean(name) + strided_outputs(name, where, index, value)

"""A float64 restatement of the conv stack of the multi-period discriminator
(promonet/model/discriminator.py:57-93): one layer
    y = leaky(conv2d(x, W, b, stride (s, 1), padding ((k - 1) / 2, 0)), slope)
with the zero padding explicit and the taps an explicit loop (no conv2d), the
fold of the audio (B, 1, T) into (B, 1, ceil(T / P), P) restated by index with
its right reflect pad, the gradients gz, gx (into the audio: with the adjoint
of the reflection), gW and gb written out by hand, and the DiscriminatorP
stack with its gradients (the loop over the taps and weight norm:
tests/conv_oracle.py). `defect` plants one wrong reading (DEFECTS,
FOLD_DEFECTS, STACK_DEFECTS): the comparisons of the GPU tests must reject
each of them (tests/test_cpu_pconv.py).

Also the closed-form parameters of the stacks (the multiplicative hash of
tests/conv_oracle.py: one period has 8.3 M of them, stored nowhere), the
cases of the tests, their seeded inputs, the figures of the comparison and the
gates.
"""
import re
from pathlib import Path

import torch

import conv_oracle
from conv_oracle import (  # noqa: F401 (used by the tests through here)
    QUANTITIES, figure, hashed, integers, leaky, weight_norm,
    weight_norm_backward, weight_norm_fp32_figures, weight_norm_inputs)

ROOT = Path(__file__).resolve().parent.parent

DEFECTS = (
    'stride_on_width', 'padding_one_at_k5', 'height_rounded_up',
    'taps_flipped', 'tap_across_batch_row', 'tap_from_neighbour_column',
    'gx_second_tap_dropped', 'gw_bottom_rows_dropped', 'slope_on_positive',
    'slope_left_out_of_gz', 'mask_from_input')
FOLD_DEFECTS = (
    'fold_axes_swapped', 'zero_pad', 'reflect_repeats_edge',
    'reflect_adjoint_left_out')
STACK_DEFECTS = ('maps_before_activation', 'activation_after_post')
# (channels, out_channels, kernel, stride): the six forms, in the order of the
# layers, conv_post last
FORMS = ((1, 32, 5, 3), (32, 128, 5, 3), (128, 512, 5, 3), (512, 1024, 5, 3),
         (1024, 1024, 5, 1), (1024, 1, 3, 1))
SLOPE = .1


def kernel_constants():
    """The tile constants of the kernels, read from their header"""
    text = (ROOT / 'promonet_amd' / 'csrc' / 'pm_pconv.h').read_text()
    return {name: int(value) for name, value in re.findall(
        r'#define (PC_[A-Z_]+) (\d+)\b', text)}


CONSTANTS = kernel_constants()
BATCH = 2
_NT, _PIX = CONSTANTS['PC_NT'], CONSTANTS['PC_GW_PIX']
# the smallest height whose output at stride 3 and period 11 has more than
# PC_NT pixels in the batch (a second pixel tile, which the first batch row
# does not fill: the first tile crosses into the second row) and more than
# PC_GW_MIN_CHUNKS chunks of PC_GW_PIX (a second gW partial)
_ROWS = max(_NT, CONSTANTS['PC_GW_MIN_CHUNKS'] * _PIX) // (BATCH * 11) + 1
# (C, O, k, s, H, P, slope): every form at H = 0, 1 and 2 (mod 3), at the
# periods 2, 3 and 11
CASES = {
    'first-0': FORMS[0] + (9, 2, .1),
    'first-1': FORMS[0] + (10, 3, .1),
    'first-2': FORMS[0] + (3 * (4 * _ROWS) + 2, 11, .1),
    'second-0': FORMS[1] + (12, 3, .1),
    'second-1': FORMS[1] + (13, 2, .1),
    # H = 1
    'second-one-row': FORMS[1] + (1, 3, .1),
    # two pixel tiles of the forward, six of gx (two a residue class), the
    # first of each across the batch row; two gW partials
    'second-2': FORMS[1] + (3 * _ROWS + 2, 11, .1),
    'third-0': FORMS[2] + (6, 2, .1),
    'third-1': FORMS[2] + (7, 3, .1),
    # four K chunks of the forward, sixteen of gx; the tiles as 'second-2'
    'third-2': FORMS[2] + (3 * _ROWS - 1, 11, .1),
    # an output height of 1
    'fourth-0': FORMS[3] + (3, 2, .1),
    'fourth-1': FORMS[3] + (3 * _ROWS - 2, 11, .1),
    'fourth-2': FORMS[3] + (5, 3, .1),
    'fifth-0': FORMS[4] + (3, 2, .1),
    # H = 1: every tap but the centre is padding
    'fifth-1': FORMS[4] + (1, 3, .1),
    'fifth-2': FORMS[4] + (2, 11, .1),
    # stride 1: two pixel tiles both ways, two gW partials
    'fifth-large': FORMS[4] + (_ROWS, 11, .1),
    'post-0': FORMS[5] + (3, 2, 1.),
    'post-1': FORMS[5] + (1, 3, 1.),
    # seven partials of PC_POST_CHUNK pixels
    'post-2': FORMS[5] + (5, 11, 1.),
}
# (T, P, slope): the first layer on the audio itself
FOLD_CASES = {
    # T mod P = 0: nothing reflected; two partials of PC_FOLD_CHUNK pixels
    'audio-even': (486, 2, .1),
    # n = P - 1 reflected samples
    'audio-reflect': (487, 3, .1),
    # n = P - 1 with T just above n: one row of the map is all but the audio
    'audio-short': (12, 11, .1),
    'audio-five': (98, 5, .1),
}
ALL_CASES = {**CASES, **FOLD_CASES}
# The largest error of the reference's own arithmetic in fp32 (pad(reflect),
# view, conv2d and leaky_relu with autograd on the build host's CPU) against
# this oracle, per case, relative to the RMS of the true quantity
# (fp32_figures; printed by tests/test_cpu_pconv.py). The gates stand on
# these.
FP32_RECORDED = {
    'first-0': (3.552e-07, 6.944e-07, 1.964e-07, 2.045e-07),
    'first-1': (2.380e-07, 6.251e-07, 3.029e-07, 1.160e-07),
    'first-2': (4.226e-07, 8.732e-07, 1.156e-06, 8.287e-07),
    'second-0': (1.133e-06, 1.663e-06, 9.152e-07, 3.580e-07),
    'second-1': (1.317e-06, 2.216e-06, 9.750e-07, 5.566e-07),
    'second-one-row': (4.471e-07, 1.058e-06, 1.978e-06, 1.327e-07),
    'second-2': (1.400e-06, 2.629e-06, 1.312e-06, 9.616e-07),
    'third-0': (9.192e-07, 2.811e-06, 1.128e-06, 3.541e-07),
    'third-1': (1.087e-06, 4.258e-06, 1.126e-06, 4.180e-07),
    'third-2': (1.241e-06, 5.281e-06, 2.370e-06, 6.806e-07),
    'fourth-0': (1.022e-06, 3.822e-06, 1.076e-06, 3.072e-07),
    'fourth-1': (1.718e-06, 8.244e-06, 1.826e-06, 6.266e-07),
    'fourth-2': (1.220e-06, 6.874e-06, 1.233e-06, 3.359e-07),
    'fifth-0': (1.701e-06, 1.222e-06, 1.587e-06, 4.121e-07),
    'fifth-1': (1.431e-06, 1.013e-06, 2.410e-06, 2.664e-07),
    'fifth-2': (1.950e-06, 1.457e-06, 2.761e-06, 7.586e-07),
    'fifth-large': (2.541e-06, 1.313e-06, 2.794e-06, 8.347e-07),
    'post-0': (1.942e-07, 1.860e-07, 4.660e-07, 5.306e-08),
    'post-1': (3.984e-07, 1.713e-07, 6.077e-07, 1.190e-08),
    'post-2': (5.966e-07, 5.290e-07, 9.100e-07, 8.179e-09),
    'audio-even': (4.879e-07, 1.193e-06, 5.192e-07, 4.997e-07),
    'audio-reflect': (5.459e-07, 1.121e-06, 4.326e-07, 4.056e-07),
    'audio-short': (2.346e-07, 2.863e-07, 2.181e-07, 3.891e-07),
    'audio-five': (3.448e-07, 8.952e-07, 4.117e-07, 2.983e-07),
}
# What one MI355X showed on the same cases (tests/test_gpu_pconv.py prints
# them): for the record, the gates do not stand on them
DEVICE_RECORDED = {
    'first-0': (3.552e-07, 3.470e-07, 2.504e-07, 2.182e-07),
    'first-1': (2.380e-07, 4.284e-07, 3.029e-07, 1.457e-07),
    'first-2': (4.226e-07, 4.671e-07, 5.960e-07, 3.099e-07),
    'second-0': (9.681e-07, 8.589e-07, 9.152e-07, 3.580e-07),
    'second-1': (1.315e-06, 8.296e-07, 9.750e-07, 5.566e-07),
    'second-one-row': (5.794e-07, 4.098e-07, 1.978e-06, 1.327e-07),
    'second-2': (1.785e-06, 9.301e-07, 1.025e-06, 4.650e-07),
    'third-0': (1.597e-06, 1.644e-06, 1.128e-06, 3.541e-07),
    'third-1': (1.786e-06, 1.524e-06, 1.126e-06, 4.180e-07),
    'third-2': (1.873e-06, 1.761e-06, 2.370e-06, 6.806e-07),
    'fourth-0': (1.931e-06, 1.339e-06, 1.076e-06, 3.072e-07),
    'fourth-1': (3.929e-06, 2.683e-06, 1.999e-06, 6.266e-07),
    'fourth-2': (3.461e-06, 2.085e-06, 1.233e-06, 3.359e-07),
    'fifth-0': (3.304e-06, 3.723e-06, 1.587e-06, 4.121e-07),
    'fifth-1': (1.830e-06, 1.682e-06, 2.410e-06, 2.664e-07),
    'fifth-2': (3.616e-06, 2.850e-06, 2.761e-06, 7.586e-07),
    'fifth-large': (5.703e-06, 3.607e-06, 2.794e-06, 1.173e-06),
    'post-0': (1.942e-07, 1.860e-07, 4.660e-07, 5.306e-08),
    'post-1': (1.963e-07, 1.713e-07, 6.077e-07, 1.190e-08),
    'post-2': (3.496e-07, 5.290e-07, 4.198e-07, 6.648e-07),
    'audio-even': (4.879e-07, 4.274e-07, 5.014e-07, 3.378e-07),
    'audio-reflect': (5.459e-07, 3.866e-07, 5.716e-07, 3.346e-07),
    'audio-short': (2.346e-07, 1.391e-07, 2.982e-07, 2.494e-07),
    'audio-five': (3.448e-07, 3.124e-07, 3.822e-07, 3.148e-07),
}
# torch._weight_norm and its autograd in fp32 on the build host's CPU against
# the oracle at fan 5, 160, 640, 2560, 5120 and 3072: w, g_g, g_v, the largest
# over the six shapes
WEIGHT_NORM_SHAPES = tuple(
    (form[1], form[0], form[2], 1) for form in FORMS)
WEIGHT_NORM_RECORDED = (1.328e-06, 1.566e-06, 1.346e-06)
# (one MI355X, the largest over the six shapes)
WEIGHT_NORM_DEVICE_RECORDED = (7.826e-07, 6.017e-07, 9.878e-07)
WEIGHT_NORM_GATES = tuple(4. * value for value in WEIGHT_NORM_RECORDED)


def gate(quantity):
    return conv_oracle.gate(FP32_RECORDED, quantity)


###############################################################################
# The fold
###############################################################################


def reflected(samples, period):
    """n: the samples the reference reflects on the right"""
    return (period - samples % period) % period


def fold_index(samples, period, defect=None):
    """(H, P) int64: the sample each pixel of the folded map reads, -1 being
    zero"""
    pad = reflected(samples, period)
    assert samples > pad
    position = torch.arange(samples + pad)
    source = torch.where(
        position < samples, position, 2 * (samples - 1) - position)
    if defect == 'reflect_repeats_edge':
        source = torch.where(
            position < samples, position, 2 * samples - 1 - position)
    if defect == 'zero_pad':
        source = torch.where(
            position < samples, position, torch.full_like(position, -1))
    height = (samples + pad) // period
    if defect == 'fold_axes_swapped':
        return source.reshape(period, height).t().contiguous()
    return source.reshape(height, period)


def fold(audio, period, defect=None):
    """audio (B, 1, T) -> (B, 1, ceil(T / P), P), by index"""
    index = fold_index(audio.shape[-1], period, defect)
    values = audio[..., index.clamp(min=0).flatten()]
    values = values * (index.flatten() >= 0).to(values.dtype)
    return values.reshape(*audio.shape[:2], *index.shape)


def fold_backward(grad_map, samples, period, defect=None):
    """The gradient in the audio (B, 1, T) of the gradient in the folded map:
    sample t receives its own position and, for T - 1 - n <= t <= T - 2, the
    position 2 (T - 1) - t"""
    planted = defect if defect in ('zero_pad', 'reflect_repeats_edge') \
        else None
    index = fold_index(samples, period, planted).flatten()
    flat = grad_map.reshape(*grad_map.shape[:2], -1)
    grad = flat[..., :samples].clone()
    if defect == 'reflect_adjoint_left_out':
        return grad
    for position in range(samples, len(index)):
        if index[position] >= 0:
            grad[..., index[position]] += flat[..., position]
    return grad


###############################################################################
# The layer
###############################################################################


def geometry(kernel, stride, defect=None):
    """(stride h, stride w, padding h)"""
    pad = (kernel - 1) // 2
    if defect == 'padding_one_at_k5' and kernel == 5:
        pad = 1
    if defect == 'stride_on_width':
        return 1, stride, pad
    return stride, 1, pad


def out_shape(height, period, kernel, stride, defect=None):
    sh, sw, pad = geometry(kernel, stride, defect)
    out_height = (height + 2 * pad - kernel) // sh + 1
    if defect == 'height_rounded_up':
        out_height = height // stride + 1
    return out_height, (period - 1) // sw + 1


def padded_input(x, kernel, stride, defect=None):
    """x with the zero padding of the conv above and below it (and, where a
    defect reads past it, zeros further down)"""
    batch, channels, height, period = x.shape
    sh, _, pad = geometry(kernel, stride, defect)
    out_height, _ = out_shape(height, period, kernel, stride, defect)
    rows = max(height + 2 * pad, (out_height - 1) * sh + kernel)
    out = x.new_zeros(batch, channels, rows, period)
    out[:, :, pad:pad + height] = x
    if defect == 'tap_across_batch_row':
        # the padding rows hold what lies there in memory (B, H, P, C): the
        # last rows of the batch row before, the first of the one after
        for b in range(batch):
            if b and height >= pad:
                out[b, :, :pad] = x[b - 1, :, height - pad:]
            if b + 1 < batch:
                below = min(rows - pad - height, height)
                out[b, :, pad + height:pad + height + below] = \
                    x[b + 1, :, :below]
    return out


def taps(height, period, kernel, stride, defect=None):
    """(kh, 0, rows, columns) of the padded input that each tap reads"""
    sh, sw, _ = geometry(kernel, stride, defect)
    out_height, out_width = out_shape(height, period, kernel, stride, defect)
    for tap in range(kernel):
        yield (tap, 0, slice(tap, tap + (out_height - 1) * sh + 1, sh),
               slice(0, (out_width - 1) * sw + 1, sw))


def wrong_weight(weight, defect):
    if defect == 'taps_flipped':
        return weight.flip(2)
    return weight


def neighbour_columns(x, kernel, stride):
    """'tap_from_neighbour_column': tap t of the output pixel (ho, w) reads
    the pixel t - pad places on in the flattened (h, w) order of its batch
    row, in place of t - pad rows on: (B, C, k, Ho, P)"""
    batch, channels, height, period = x.shape
    pad = (kernel - 1) // 2
    out_height = (height - 1) // stride + 1
    flat = x.new_zeros(batch, channels, height * period + 2 * pad)
    flat[..., pad:pad + height * period] = x.reshape(batch, channels, -1)
    start = (torch.arange(out_height) * stride * period)[:, None] + \
        torch.arange(period)[None]
    return torch.stack(
        [flat[..., (start + tap).flatten()].reshape(
            batch, channels, out_height, period) for tap in range(kernel)],
        dim=2)


def pre_activation(x, weight, bias, stride, defect=None):
    x, weight, bias = x.double(), weight.double(), bias.double()
    weight = wrong_weight(weight, defect)
    kernel = weight.shape[2]
    if defect == 'tap_from_neighbour_column':
        z = torch.einsum(
            'ock,bckhw->bohw', weight[..., 0], neighbour_columns(
                x, kernel, stride))
        return z + bias[None, :, None, None]
    z = conv_oracle.conv_forward(
        padded_input(x, kernel, stride, defect), weight,
        taps(*x.shape[2:], kernel, stride, defect))
    return z + bias[None, :, None, None]


def layer(x, weight, bias, stride, slope, defect=None):
    return leaky(pre_activation(x, weight, bias, stride, defect), slope, defect)


def gate_gradient(upstream, y, x, stride, slope, defect=None):
    """gz = upstream * leaky'(y), y = 0 taking the slope as torch does"""
    mask = y > 0.
    if defect == 'mask_from_input':
        source = x if x.shape[1] == y.shape[1] else x[:, :1]
        mask = (source[:, :, ::stride][:, :, :y.shape[2]] > 0.).expand_as(y)
    if defect == 'slope_left_out_of_gz':
        return upstream.clone()
    return torch.where(mask, upstream, upstream * slope)


def layer_backward(x, weight, y, upstream, stride, slope, defect=None):
    """(gx, gW, gb) from the upstream gradient, the output and the input"""
    x, weight, y = x.double(), weight.double(), y.double()
    gz = gate_gradient(upstream.double(), y, x, stride, slope, defect)
    weight = wrong_weight(weight, defect)
    kernel = weight.shape[2]
    source = padded_input(x, kernel, stride, defect)
    sh, _, pad = geometry(kernel, stride, defect)
    # at stride 3 the residue classes 1 and 2 take two taps each, t and t + 3
    scatters = (lambda kh, kw: kh < stride) \
        if defect == 'gx_second_tap_dropped' else None
    kept = None
    if defect == 'gw_bottom_rows_dropped':
        # the output rows whose window reaches the bottom padding
        inside = (torch.arange(gz.shape[2]) * sh + kernel - 1 - pad) < \
            x.shape[2]
        kept = gz * inside[:, None]
    spread, grad_weight = conv_oracle.conv_adjoint(
        source, weight, gz, taps(*x.shape[2:], kernel, stride, defect),
        scatters, kept)
    grad_weight = wrong_weight(grad_weight, defect)
    grad_x = spread[:, :, pad:pad + x.shape[2]]
    return grad_x.contiguous(), grad_weight.contiguous(), gz.sum((0, 2, 3))


###############################################################################
# The parameters and the input of the stacks: closed forms of integer indices,
# exact in fp32, the same on every machine (no RNG, no libm)
###############################################################################

PERIODS = (2, 5, 11)
STACK_AUDIO = (2, 1, 486)


def shapes():
    """{key: shape} of the state_dict of DiscriminatorP, in its order"""
    out = {}
    for index, (channels, out_channels, kernel, _) in enumerate(FORMS):
        prefix = f'convs.{index}.' if index < 5 else 'conv_post.'
        out[prefix + 'bias'] = (out_channels,)
        out[prefix + 'weight_g'] = (out_channels, 1, 1, 1)
        out[prefix + 'weight_v'] = (out_channels, channels, kernel, 1)
    return out


def parameters(period):
    """{key: fp32 tensor}: weight_v in [-.5, .5), bias in [-.125, .125),
    weight_g in [.5, 1.25)"""
    return conv_oracle.hashed_parameters(shapes(), 2000 + 30 * period)


def stack_audio():
    """The fixed audio of the stacks: [-1, 1), multiples of 2^-11"""
    count = STACK_AUDIO[0] * STACK_AUDIO[2]
    return (2. * hashed(count, 8000) - 1.).float().reshape(STACK_AUDIO)


def coefficients(period, shapes_of_maps):
    """The fixed linear functional: one fp32 tensor per map (the last is the
    logits), in [-.5, .5) for the maps and in [0, 1) for the logits, whose
    bias gradient would otherwise be a cancelling sum (tests/fdisc_oracle.py,
    coefficients)"""
    return conv_oracle.hashed_coefficients(shapes_of_maps, 9000 + 10 * period)


###############################################################################
# The stack
###############################################################################

# A pre-activation this close to zero, relative to the RMS of its layer, is
# fragile: 64 x 3e-6, the fp32 error of a layer (FP32_RECORDED): its side of
# the mask cannot be told in fp32
FRAGILE = 2e-4
PREFIXES = tuple(f'convs.{index}.' for index in range(5)) + ('conv_post.',)


def stack(period, audio, parameters_, defect=None):
    """audio (B, 1, T) -> (logits (B, 1, H, P), the six maps in the
    reference's order, the logits last, what the backward needs)"""
    x = fold(audio.double(), period)
    maps, saved = [], []
    for prefix, (_, _, _, stride) in zip(PREFIXES, FORMS):
        weight = weight_norm(
            parameters_[prefix + 'weight_g'], parameters_[prefix + 'weight_v'])
        last = prefix == 'conv_post.'
        slope = 1. if last and defect != 'activation_after_post' else SLOPE
        z = pre_activation(x, weight, parameters_[prefix + 'bias'], stride)
        y = leaky(z, slope)
        saved.append((prefix, x, weight, y, z, stride, slope))
        maps.append(
            z if defect == 'maps_before_activation' and not last else y)
        x = y
    return maps[-1], maps, (saved, audio.shape[-1], period)


def stack_backward(saved, parameters_, upstreams, mend=False):
    """upstreams: the gradient at every map (the logits last) -> (the gradient
    in the audio (B, 1, T), {key: gradient}, the upstreams as used). With
    `mend`, the upstream of a fragile element is replaced by minus what the
    later layers carry to it, rounded to fp32: its gz is then zero to 2^-24
    whichever side of the mask it is on."""
    records, samples, period = saved
    upstreams = [u.double().clone() for u in upstreams]
    gradients = {}
    carried = None
    for index in reversed(range(len(records))):
        prefix, x, weight, y, z, stride, slope = records[index]
        upstream = upstreams[index]
        if carried is not None:
            if mend and slope != 1.:
                fragile = z.abs() < FRAGILE * z.pow(2).mean().sqrt()
                upstream[fragile] = (-carried[fragile]).float().double()
            upstream = upstream + carried
        carried, grad_weight, grad_bias = layer_backward(
            x, weight, y, upstream, stride, slope)
        grad_g, grad_v = weight_norm_backward(
            grad_weight, parameters_[prefix + 'weight_g'],
            parameters_[prefix + 'weight_v'])
        gradients[prefix + 'weight_g'] = grad_g
        gradients[prefix + 'weight_v'] = grad_v
        gradients[prefix + 'bias'] = grad_bias
    return (fold_backward(carried, samples, period), gradients,
            [u.float() for u in upstreams])


def fragile_share(saved):
    """The share of the fragile pre-activations of a stack"""
    fragile = total = 0
    for _, _, _, _, z, _, slope in saved[0]:
        if slope != 1.:
            fragile += (z.abs() < FRAGILE * z.pow(2).mean().sqrt()).sum().item()
            total += z.numel()
    return fragile / total


def golden_coefficients(golden, period):
    """The functional of the golden: the closed form, mended where the golden
    says"""
    kept = golden['stacks'][period]
    return conv_oracle.golden_coefficients(
        kept, coefficients(period, kept['map_shapes']))


def stack_figures(golden, period, logits, maps, grad_audio, gradients):
    """[(label, quantity, figure)] of a stack's results against the golden:
    the comparison of the GPU tests. `maps` without the logits; `gradients`
    {key: tensor}."""
    kept = golden['stacks'][period]
    return conv_oracle.stack_figures(
        golden, kept, logits, maps, grad_audio, kept['gradient_audio'],
        gradients)


###############################################################################
# The inputs of the cases, the truth and the figures
###############################################################################


def form_of(name):
    """(C, O, k, s, slope) of a case; a fold case is the first form"""
    if name in FOLD_CASES:
        return FORMS[0] + (FOLD_CASES[name][2],)
    return CASES[name][:4] + (CASES[name][6],)


def out_height_of(name):
    if name in FOLD_CASES:
        samples, period, _ = FOLD_CASES[name]
        height = (samples + reflected(samples, period)) // period
        return (height - 1) // 3 + 1
    return (CASES[name][4] - 1) // CASES[name][3] + 1


def inputs(name, seed=0):
    """fp32: x (a map (B, C, H, P), or the audio (B, 1, T) of a fold case),
    upstream Gaussian; weight and bias from Conv2d's default initialisation,
    seeded without touching the global generator"""
    channels, out_channels, kernel, _, _ = form_of(name)
    index = list(ALL_CASES).index(name)
    generator = torch.Generator().manual_seed(seed * 1000 + index)
    if name in FOLD_CASES:
        samples, period, _ = FOLD_CASES[name]
        x = torch.randn(BATCH, 1, samples, generator=generator)
    else:
        period = CASES[name][5]
        x = torch.randn(
            BATCH, channels, CASES[name][4], period, generator=generator)
    upstream = torch.randn(
        BATCH, out_channels, out_height_of(name), period, generator=generator)
    weight, bias = conv_oracle.conv_parameters(
        torch.nn.Conv2d, seed * 1000 + 500 + index, channels, out_channels,
        (kernel, 1))
    return x, weight, bias, upstream


def reference_fold(audio, period):
    """The reference's own fold (:78-83)"""
    batch, channels, samples = audio.shape
    if samples % period != 0:
        pad = period - samples % period
        audio = torch.nn.functional.pad(audio, (0, pad), 'reflect')
        samples = samples + pad
    return audio.view(batch, channels, samples // period, period)


def reference_fp32(name, x, weight, bias, dtype=torch.float32, upstream=None):
    """The reference's own arithmetic: (pad(reflect) and view,) conv2d and
    leaky_relu with autograd in `dtype` on the CPU -> pre-activation, output
    and, with an upstream gradient, (gx, gW, gb)"""
    _, _, kernel, stride, slope = form_of(name)
    x = x.to(dtype).clone().requires_grad_(True)
    weight = weight.to(dtype).clone().requires_grad_(True)
    bias = bias.to(dtype).clone().requires_grad_(True)
    folded = reference_fold(x, FOLD_CASES[name][1]) \
        if name in FOLD_CASES else x
    z = torch.nn.functional.conv2d(
        folded, weight, bias, stride=(stride, 1),
        padding=((kernel - 1) // 2, 0))
    y = z if slope == 1. else torch.nn.functional.leaky_relu(z, slope)
    if upstream is None:
        return z.detach(), y.detach(), None
    y.backward(upstream.to(dtype))
    return z.detach(), y.detach(), (x.grad, weight.grad, bias.grad)


def case_layer(name, x, weight, bias, defect=None):
    """The oracle's layer of a case, `defect` planted where it applies"""
    _, _, _, stride, slope = form_of(name)
    if name in FOLD_CASES:
        period = FOLD_CASES[name][1]
        folded = fold(
            x.double(), period, defect if defect in FOLD_DEFECTS else None)
        return layer(folded, weight, bias, stride, slope,
                     None if defect in FOLD_DEFECTS else defect)
    return layer(x, weight, bias, stride, slope, defect)


def case_backward(name, x, weight, y, upstream, defect=None):
    _, _, _, stride, slope = form_of(name)
    if name in FOLD_CASES:
        period = FOLD_CASES[name][1]
        planted = defect if defect in FOLD_DEFECTS else None
        grad_map, grad_weight, grad_bias = layer_backward(
            fold(x.double(), period, planted), weight, y, upstream, stride,
            slope, None if planted else defect)
        if planted == 'fold_axes_swapped':
            grad_map = grad_map.transpose(2, 3)
        return (fold_backward(grad_map, x.shape[-1], period, planted),
                grad_weight, grad_bias)
    return layer_backward(x, weight, y, upstream, stride, slope, defect)


# The truth of a case (the kink is that of a slope other than 1), the figures
# of a result against it and those of the reference's own arithmetic in fp32
_TRUTHS = conv_oracle.Truths(
    inputs,
    lambda name, x, weight, bias: pre_activation(
        fold(x.double(), FOLD_CASES[name][1]) if name in FOLD_CASES else x,
        weight, bias, form_of(name)[3]),
    lambda name: form_of(name)[4] != 1.,
    lambda name, z: leaky(z, form_of(name)[4]),
    case_backward, reference_fp32)
truth, figures = _TRUTHS.truth, _TRUTHS.figures
fp32_figures = _TRUTHS.fp32_figures



"""A float64 restatement of the conv stacks of the FARGAN discriminator
(promonet/model/discriminator.py:320-389): one layer
    y = act(conv3x3(cat(x, sin, cos)) + bias),
stride 1, dilation (d, 1), padding (d, 1), the embedding of
FrequencyPositionalEmbedding (:381-389) explicit, the zero padding explicit,
the taps an explicit loop (no conv2d), with its gradients in x, W and b written
out by hand; weight norm and its adjoint; the stack of six and its gradients.
`defect` plants one wrong reading of the layer (DEFECTS): the comparisons of
the GPU tests must reject each of them (tests/test_cpu_fdisc.py).

Also the cases of the tests, their seeded inputs, the figures of the
comparison and the gates.
"""
import math
import re
from pathlib import Path

import torch

import conv_oracle
from conv_oracle import (  # noqa: F401 (used by the tests through here)
    QUANTITIES, activate, figure, integers, weight_norm, weight_norm_backward)

ROOT = Path(__file__).resolve().parent.parent

DEFECTS = (
    'angle', 'swapped', 'embedding_unpadded_frequency',
    'embedding_unpadded_time', 'dilation_on_time', 'padding_one',
    'taps_transposed', 'relu_mask_from_input', 'sigmoid_gradient_left_out',
    'embedding_weight_gradient_dropped', 'norm_whole_tensor')


def kernel_constants():
    """The tile constants of the kernels, read from their header"""
    text = (ROOT / 'promonet_amd' / 'csrc' / 'pm_fdisc.h').read_text()
    found = {name: int(value) for name, value in re.findall(
        r'#define (FD_[A-Z_]+) (\d+)\b', text)}
    found['FD_CONV_PIXELS'] = \
        found['FD_THREADS'] // 64 * found['FD_WAVE_TILES'] * 16
    return found


CONSTANTS = kernel_constants()
BATCH = 2
# (C, O, F, T, d, activation): the smallest shapes that reach each thing that
# can go wrong
CASES = {
    'first': (1, 16, 33, 7, 1, 'relu'),
    'd2': (16, 16, 65, 5, 2, 'relu'),
    'd4': (16, 16, 129, 3, 4, 'relu'),
    # T = 1: both time borders at once
    'd8-one-frame': (16, 16, 40, 1, 8, 'relu'),
    # most frequency taps out of range, pixels no multiple of a tile
    'd16': (16, 16, 70, 9, 16, 'relu'),
    'last': (16, 1, 33, 7, 1, 'sigmoid'),
    # more than one workgroup of the conv kernel, more than one partial of the
    # weight gradient (the last wave's pixels no multiple of a step of 4)
    'large': (16, 16, 41, CONSTANTS['FD_GW_CHUNK'] // (BATCH * 41) + 3, 2,
              'relu'),
}
# The largest error of the reference's own arithmetic in fp32 (torch.cat +
# conv2d + the activation, with autograd, on the build host's CPU) against
# this oracle, per case, relative to the RMS of the true quantity
# (fp32_figures; printed by tests/test_cpu_fdisc.py). The gates stand on these.
FP32_RECORDED = {
    'first': (8.851e-07, 5.911e-07, 1.019e-06, 2.956e-07),
    'd2': (1.975e-06, 1.104e-06, 1.664e-06, 4.647e-07),
    'd4': (1.832e-06, 1.377e-06, 1.397e-06, 5.531e-07),
    'd8-one-frame': (7.624e-07, 6.320e-07, 9.820e-07, 2.115e-07),
    'd16': (2.382e-06, 1.706e-06, 1.629e-06, 3.749e-07),
    'last': (2.629e-07, 5.383e-07, 5.261e-07, 1.972e-07),
    'large': (2.603e-06, 1.345e-06, 2.293e-06, 1.290e-06),
}
# torch._weight_norm and its autograd in fp32 on the build host's CPU against
# the oracle, the largest of the three shapes of tests/test_gpu_fdisc.py:
# w, g_g, g_v, relative to the RMS of each
WEIGHT_NORM_RECORDED = (2.664e-07, 2.878e-07, 3.359e-07)
WEIGHT_NORM_GATES = tuple(4. * value for value in WEIGHT_NORM_RECORDED)


def gate(quantity):
    return conv_oracle.gate(FP32_RECORDED, quantity)


###############################################################################
# The layer
###############################################################################


def embedding(bins, defect=None, first=0, count=None):
    """sin, cos (count) of 2 pi f / bins at f = first ... first + count - 1"""
    count = bins if count is None else count
    args = torch.arange(first, first + count, dtype=torch.float64) * \
        torch.pi * 2 / (bins - 1 if defect == 'angle' else bins)
    sin, cos = torch.sin(args), torch.cos(args)
    return (cos, sin) if defect == 'swapped' else (sin, cos)


def geometry(dilation, defect=None):
    """(dilation f, dilation t, padding f, padding t)"""
    if defect == 'dilation_on_time':
        return 1, dilation, 1, dilation
    if defect == 'padding_one':
        return dilation, 1, 1, 1
    return dilation, 1, dilation, 1


def padded_input(x, dilation, defect=None, table=None):
    """cat(x, sin, cos) (B, C + 2, F + 2 pf, T + 2 pt) with the zero padding
    of the conv around all of it"""
    batch, channels, bins, frames = x.shape
    _, _, pf, pt = geometry(dilation, defect)
    out = x.new_zeros(batch, channels + 2, bins + 2 * pf, frames + 2 * pt)
    out[:, :channels, pf:pf + bins, pt:pt + frames] = x
    if table is None:
        sin, cos = embedding(bins, defect)
    else:
        sin, cos = table.double().unbind(1)
    f0, f1, t0, t1 = pf, pf + bins, pt, pt + frames
    if defect == 'embedding_unpadded_frequency':
        sin, cos = embedding(bins, None, -pf, bins + 2 * pf)
        f0, f1 = 0, bins + 2 * pf
    if defect == 'embedding_unpadded_time':
        t0, t1 = 0, frames + 2 * pt
    out[:, channels, f0:f1, t0:t1] = sin[None, :, None]
    out[:, channels + 1, f0:f1, t0:t1] = cos[None, :, None]
    return out


def taps(bins, frames, dilation, defect=None):
    """(kf, kt, rows, columns) of the padded input that each tap reads"""
    df, dt, pf, pt = geometry(dilation, defect)
    out_bins = bins + 2 * pf - 2 * df
    out_frames = frames + 2 * pt - 2 * dt
    for kf in range(3):
        for kt in range(3):
            yield (kf, kt, slice(kf * df, kf * df + out_bins),
                   slice(kt * dt, kt * dt + out_frames))


def pre_activation(x, weight, bias, dilation, defect=None, table=None):
    x, weight, bias = x.double(), weight.double(), bias.double()
    if defect == 'taps_transposed':
        weight = weight.transpose(2, 3)
    z = conv_oracle.conv_forward(
        padded_input(x, dilation, defect, table), weight,
        taps(*x.shape[2:], dilation, defect))
    return z + bias[None, :, None, None]


def layer(x, weight, bias, dilation, activation, defect=None, table=None):
    return activate(
        pre_activation(x, weight, bias, dilation, defect, table), activation)


def layer_backward(x, weight, y, upstream, dilation, activation, defect=None,
                   table=None):
    """(gx, gW, gb) from the upstream gradient, the output and the input"""
    x, weight, y = x.double(), weight.double(), y.double()
    upstream = upstream.double()
    if defect == 'taps_transposed':
        weight = weight.transpose(2, 3)
    channels = x.shape[1]
    if activation == 'relu':
        # torch's threshold_backward: 0 where y <= 0, the upstream elsewhere
        # (a NaN output passes it), a choice and not a product (an infinite
        # upstream behind a closed gate gives 0)
        mask = ~(y <= 0.)
        if defect == 'relu_mask_from_input':
            mask = (x if channels == y.shape[1] else x[:, :1]) > 0.
            mask = mask.expand_as(y)
        gz = torch.where(mask, upstream, torch.zeros_like(upstream))
    elif activation == 'sigmoid':
        gz = upstream if defect == 'sigmoid_gradient_left_out' \
            else upstream * y * (1. - y)
    else:
        gz = upstream
    source = padded_input(x, dilation, defect, table)
    spread, grad_weight = conv_oracle.conv_adjoint(
        source, weight, gz, taps(*x.shape[2:], dilation, defect))
    if defect == 'taps_transposed':
        grad_weight = grad_weight.transpose(2, 3)
    if defect == 'embedding_weight_gradient_dropped':
        grad_weight[:, channels:] = 0.
    _, _, pf, pt = geometry(dilation, defect)
    grad_x = spread[:, :channels, pf:pf + x.shape[2], pt:pt + x.shape[3]]
    return grad_x.contiguous(), grad_weight.contiguous(), gz.sum((0, 2, 3))


###############################################################################
# The stack (weight norm: tests/conv_oracle.py)
###############################################################################


def coefficients(batch, bins, frames):
    """The fixed linear functional of the stack's tests: one fp32 tensor per
    output (the five maps, then the logits), from integer arithmetic alone, so
    every machine forms the same. In [-.5, .5) for the maps and in [0, 1) for
    the logits: the last layer's bias gradient is ONE number, the sum of c y
    (1 - y) over all pixels, and with signed c it is a cancelling sum (0.006
    from 330 terms of up to 0.125, partial sums near 1): half an ulp of a
    partial sum is then 1e-5 of the result in any fp32 order, which a figure
    relative to the result cannot tell from an error."""
    out = []
    for index in range(6):
        shape = (batch, 1 if index == 5 else 16, bins, frames)
        count = math.prod(shape)
        mixed = (torch.arange(count, dtype=torch.int64) + 7919 * (index + 1)) \
            * 2654435761 % 2 ** 32
        out.append((mixed.double() / 2 ** 32 - (.5 if index < 5 else 0.))
                   .float().reshape(shape))
    return out


def stack(x, parameters, dilations, defect=None):
    """x (B, 1, F, T); parameters: [(weight_g, weight_v, bias)] of the six
    layers -> (logits (B, 1, F, T), [five maps], what the backward needs)"""
    saved, outputs = [], []
    for index, ((g, v, bias), dilation) in enumerate(
            zip(parameters, dilations)):
        activation = 'sigmoid' if index == len(dilations) - 1 else 'relu'
        weight = weight_norm(g, v, defect)
        y = layer(x, weight, bias, dilation, activation, defect)
        saved.append((x.double(), weight, y, dilation, activation))
        outputs.append(y)
        x = y
    return outputs[-1], outputs[:-1], saved


def stack_backward(saved, parameters, upstreams, defect=None):
    """upstreams: the gradient at each of the six outputs (the maps, then the
    logits) -> (gradient in x, [(g_g, g_v, g_b)])"""
    carried, gradients = None, []
    for (x, weight, y, dilation, activation), (g, v, _), upstream in zip(
            reversed(saved), reversed(parameters), reversed(upstreams)):
        total = upstream.double() if carried is None \
            else upstream.double() + carried
        carried, grad_weight, grad_bias = layer_backward(
            x, weight, y, total, dilation, activation, defect)
        gradients.append(
            weight_norm_backward(grad_weight, g, v, defect) + (grad_bias,))
    return carried, gradients[::-1]


###############################################################################
# The inputs of the cases, the truth and the figures
###############################################################################


def inputs(name, seed=0):
    """fp32: x Gaussian (16 channels) or 20 N(0, 1) - 40, decibel-like (one
    channel); weight and bias from Conv2d's default init; upstream Gaussian"""
    channels, out_channels, bins, frames, _, _ = CASES[name]
    generator = torch.Generator().manual_seed(
        seed * 1000 + list(CASES).index(name))
    x = torch.randn(BATCH, channels, bins, frames, generator=generator)
    if channels == 1:
        x = 20. * x - 40.
    upstream = torch.randn(
        BATCH, out_channels, bins, frames, generator=generator)
    weight, bias = conv_oracle.conv_parameters(
        torch.nn.Conv2d, seed * 1000 + 500 + list(CASES).index(name),
        channels + 2, out_channels, 3)
    return x, weight, bias, upstream


def reference_fp32(x, weight, bias, dilation, activation, dtype=torch.float32,
                   upstream=None):
    """The reference's own arithmetic: its embedding, torch.cat, conv2d and
    the activation, with autograd, in `dtype` on the CPU -> pre-activation,
    output and, with an upstream gradient, (gx, gW, gb)"""
    x = x.to(dtype).clone().requires_grad_(True)
    weight = weight.to(dtype).clone().requires_grad_(True)
    bias = bias.to(dtype).clone().requires_grad_(True)
    bins = x.shape[2]
    args = torch.arange(0, bins, dtype=dtype) * torch.pi * 2 / bins
    cos = torch.cos(args).reshape(1, 1, -1, 1)
    sin = torch.sin(args).reshape(1, 1, -1, 1)
    zeros = torch.zeros_like(x[:, 0:1, :, :])
    z = torch.nn.functional.conv2d(
        torch.cat((x, zeros + sin, zeros + cos), dim=1), weight, bias,
        stride=1, dilation=(dilation, 1), padding=(dilation, 1))
    y = {'relu': torch.relu, 'sigmoid': torch.sigmoid,
         'none': lambda v: v}[activation](z)
    if upstream is None:
        return z.detach(), y.detach(), None
    y.backward(upstream.to(dtype))
    return z.detach(), y.detach(), (x.grad, weight.grad, bias.grad)


# The truth of a case (the kink is the ReLU's), the figures of a result
# against it and those of the reference's own arithmetic in fp32
_TRUTHS = conv_oracle.Truths(
    inputs,
    lambda name, x, weight, bias: pre_activation(
        x, weight, bias, CASES[name][4]),
    lambda name: CASES[name][5] == 'relu',
    lambda name, z: activate(z, CASES[name][5]),
    lambda name, x, weight, y, upstream: layer_backward(
        x, weight, y, upstream, *CASES[name][4:]),
    lambda name, x, weight, bias, dtype, upstream: reference_fp32(
        x, weight, bias, *CASES[name][4:], dtype, upstream))
truth, figures = _TRUTHS.truth, _TRUTHS.figures
fp32_figures = _TRUTHS.fp32_figures

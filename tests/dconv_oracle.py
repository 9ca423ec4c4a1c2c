"""A float64 restatement of the conv stacks of the complex multi-band and the
multi-resolution discriminators (promonet/model/discriminator.py:96-127 and
:146-208): one layer
    y = leaky(conv2d(x, W, b, stride (1, s), padding (1, (kw - 1) / 2)), slope)
with the zero padding explicit and the taps an explicit loop (no conv2d), its
gradients gz, gx, gW and gb written out by hand, and the two stacks with their
gradients (the loop over the taps and weight norm: tests/conv_oracle.py).
`defect` plants one wrong reading (DEFECTS, STACK_DEFECTS): the comparisons of
the GPU tests must reject each of them (tests/test_cpu_dconv.py).

Also the closed-form parameters of the stacks, the cases of the tests, their
seeded inputs, the figures of the comparison and the gates.
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
    'stride_on_height', 'padding_swapped', 'taps_flipped', 'taps_transposed',
    'width_rounded_up', 'slope_on_positive', 'slope_left_out_of_gz',
    'mask_from_input', 'gx_odd_taps_dropped', 'gw_padded_columns_dropped')
STACK_DEFECTS = (
    'bands_wrong_order', 'activation_after_post', 'maps_before_activation')
# (channels, out_channels, kernel_width, stride): the four forms, and the
# layers of a band / of R in them
FORMS = ((1, 32, 9, 1), (32, 32, 9, 2), (32, 32, 3, 1), (32, 1, 3, 1))
LAYERS = (FORMS[0], FORMS[1], FORMS[1], FORMS[1], FORMS[2])


def kernel_constants():
    """The tile constants of the kernels, read from their header"""
    text = (ROOT / 'promonet_amd' / 'csrc' / 'pm_dconv.h').read_text()
    return {name: int(value) for name, value in re.findall(
        r'#define (DC_[A-Z_]+) (\d+)\b', text)}


CONSTANTS = kernel_constants()
BATCH = 2
# (C, O, kw, s, H, W, slope)
CASES = {
    'first': (1, 32, 9, 1, 5, 51, .1),
    'odd-width': (32, 32, 9, 2, 5, 51, .1),
    'even-width': (32, 32, 9, 2, 3, 26, .2),
    'one-row': (32, 32, 9, 2, 1, 13, .2),
    # W below the kernel's width
    'narrow': (32, 32, 9, 2, 4, 8, .1),
    'layer5': (32, 32, 3, 1, 5, 7, .2),
    'post': (32, 1, 3, 1, 5, 66, 1.),
    # DC_ROWS x DC_COLS output tiles: three row blocks (the last of one row)
    # x three column tiles (the last of 3 of 16 columns) x the batch = 18
    # tiles: more than one workgroup of the conv kernel, and with
    # DC_GW_MIN_TILES = 4 five partials of at most four tiles
    'large': (32, 32, 9, 2, 2 * CONSTANTS['DC_ROWS'] + 1,
              2 * (2 * CONSTANTS['DC_COLS'] + 3), .1),
}
# Beside the table (the gates do not stand on it, and it meets them):
# 2 x 129 tiles (of the forward and of gx), more than the 256 compute units of
# an MI355X, whose walked grid is one workgroup a unit, so a workgroup takes a
# second tile, loaded while it computes the first
EXTRA_CASES = {'walked': (32, 32, 9, 2, 2, 4097, .2)}
ALL_CASES = {**CASES, **EXTRA_CASES}
# The largest error of the reference's own arithmetic in fp32 (conv2d +
# leaky_relu with autograd on the build host's CPU) against this oracle, per
# case, relative to the RMS of the true quantity (fp32_figures; printed by
# tests/test_cpu_dconv.py). The gates stand on these.
FP32_RECORDED = {
    'first': (1.234e-06, 1.430e-06, 1.352e-06, 7.706e-07),
    'odd-width': (3.291e-06, 4.042e-06, 1.706e-06, 9.131e-07),
    'even-width': (2.730e-06, 1.161e-06, 1.001e-06, 3.274e-07),
    'one-row': (1.894e-06, 1.298e-06, 5.324e-07, 1.713e-07),
    'narrow': (2.064e-06, 9.357e-07, 7.674e-07, 3.247e-07),
    'layer5': (1.618e-06, 1.114e-06, 6.498e-07, 2.367e-07),
    'post': (1.256e-06, 6.185e-07, 1.631e-06, 2.186e-06),
    'large': (3.000e-06, 2.869e-06, 1.980e-06, 6.595e-07),
}
# torch._weight_norm and its autograd in fp32 on the build host's CPU against
# the oracle at fan 27, 288 and 864, the largest of the three: w, g_g, g_v
WEIGHT_NORM_SHAPES = ((32, 1, 3, 9), (1, 32, 3, 3), (32, 32, 3, 9))
WEIGHT_NORM_RECORDED = (4.876e-07, 8.505e-07, 4.916e-07)
WEIGHT_NORM_GATES = tuple(4. * value for value in WEIGHT_NORM_RECORDED)


def gate(quantity):
    return conv_oracle.gate(FP32_RECORDED, quantity)


###############################################################################
# The layer
###############################################################################


def geometry(kernel_width, stride, defect=None):
    """(stride h, stride w, padding h, padding w)"""
    pad = (kernel_width - 1) // 2
    if defect == 'stride_on_height':
        return stride, 1, 1, pad
    if defect == 'padding_swapped':
        return 1, stride, pad, 1
    return 1, stride, 1, pad


def out_shape(height, width, kernel_width, stride, defect=None):
    sh, sw, ph, pw = geometry(kernel_width, stride, defect)
    out_height = (height + 2 * ph - 3) // sh + 1
    out_width = (width + 2 * pw - kernel_width) // sw + 1
    if defect == 'width_rounded_up' and stride == 2:
        out_width = width // 2 + 1
    return out_height, out_width


def padded_input(x, kernel_width, stride, defect=None):
    """x with the zero padding of the conv around it (and, where a defect
    reads past it, zeros further right)"""
    batch, channels, height, width = x.shape
    sh, sw, ph, pw = geometry(kernel_width, stride, defect)
    out_height, out_width = out_shape(
        height, width, kernel_width, stride, defect)
    rows = max(height + 2 * ph, (out_height - 1) * sh + 3)
    columns = max(width + 2 * pw, (out_width - 1) * sw + kernel_width)
    out = x.new_zeros(batch, channels, rows, columns)
    out[:, :, ph:ph + height, pw:pw + width] = x
    return out


def taps(height, width, kernel_width, stride, defect=None):
    """(kh, kw, rows, columns) of the padded input that each tap reads"""
    sh, sw, _, _ = geometry(kernel_width, stride, defect)
    out_height, out_width = out_shape(
        height, width, kernel_width, stride, defect)
    for kh in range(3):
        for kw in range(kernel_width):
            yield (kh, kw, slice(kh, kh + (out_height - 1) * sh + 1, sh),
                   slice(kw, kw + (out_width - 1) * sw + 1, sw))


def wrong_weight(weight, defect):
    if defect == 'taps_flipped':
        return weight.flip(3)
    if defect == 'taps_transposed':
        assert weight.shape[2] == weight.shape[3]
        return weight.transpose(2, 3)
    return weight


def pre_activation(x, weight, bias, stride, defect=None):
    x, weight, bias = x.double(), weight.double(), bias.double()
    weight = wrong_weight(weight, defect)
    kernel_width = weight.shape[3]
    z = conv_oracle.conv_forward(
        padded_input(x, kernel_width, stride, defect), weight,
        taps(*x.shape[2:], kernel_width, stride, defect))
    return z + bias[None, :, None, None]


def layer(x, weight, bias, stride, slope, defect=None):
    return leaky(pre_activation(x, weight, bias, stride, defect), slope, defect)


def gate_gradient(upstream, y, x, stride, slope, defect=None):
    """gz = upstream * leaky'(y), y = 0 taking the slope as torch does"""
    mask = y > 0.
    if defect == 'mask_from_input':
        source = x if x.shape[1] == y.shape[1] else x[:, :1]
        mask = (source[..., ::stride][..., :y.shape[3]] > 0.).expand_as(y)
    if defect == 'slope_left_out_of_gz':
        return upstream.clone()
    return torch.where(mask, upstream, upstream * slope)


def layer_backward(x, weight, y, upstream, stride, slope, defect=None):
    """(gx, gW, gb) from the upstream gradient, the output and the input"""
    x, weight, y = x.double(), weight.double(), y.double()
    gz = gate_gradient(upstream.double(), y, x, stride, slope, defect)
    weight = wrong_weight(weight, defect)
    kernel_width = weight.shape[3]
    source = padded_input(x, kernel_width, stride, defect)
    _, sw, ph, pw = geometry(kernel_width, stride, defect)
    scatters = (lambda kh, kw: not kw % 2) \
        if defect == 'gx_odd_taps_dropped' else None
    kept = None
    if defect == 'gw_padded_columns_dropped':
        # the output columns whose window reaches the right padding
        inside = (torch.arange(gz.shape[3]) * sw + kernel_width - 1 - pw) < \
            x.shape[3]
        kept = gz * inside
    spread, grad_weight = conv_oracle.conv_adjoint(
        source, weight, gz,
        taps(*x.shape[2:], kernel_width, stride, defect), scatters, kept)
    grad_weight = wrong_weight(grad_weight, defect)
    grad_x = spread[:, :, ph:ph + x.shape[2], pw:pw + x.shape[3]]
    return grad_x.contiguous(), grad_weight.contiguous(), gz.sum((0, 2, 3))


###############################################################################
# The parameters and the inputs of the stacks: closed forms of integer
# indices, exact in fp32, the same on every machine (no RNG, no libm)
###############################################################################


def shapes(name):
    """{key: shape} of the state_dict of 'cmb' or 'r', in its order"""
    out = {}

    def conv(prefix, form):
        channels, out_channels, kernel_width, _ = form
        out[prefix + 'bias'] = (out_channels,)
        out[prefix + 'weight_g'] = (out_channels, 1, 1, 1)
        out[prefix + 'weight_v'] = (out_channels, channels, 3, kernel_width)

    if name == 'cmb':
        for band in range(5):
            for index, form in enumerate(LAYERS):
                conv(f'band_convs.{band}.{index}.0.', form)
    else:
        for index, form in enumerate(LAYERS):
            conv(f'convs.{index}.', form)
    conv('conv_post.', FORMS[3])
    return out


def parameters(name):
    """{key: fp32 tensor}: weight_v in [-.5, .5), bias in [-.125, .125),
    weight_g in [.5, 1.25): positive, and away from |v| (1.5, 4.9 and 8.5 at
    fan 27, 288 and 864), so that weight norm shows"""
    return conv_oracle.hashed_parameters(
        shapes(name), 1000 if name == 'r' else 0)


STACK_INPUTS = {'cmb': (2, 1, 6, 513), 'r': (2, 1, 33, 21)}
CMB_EDGES = ((0, 51), (51, 128), (128, 256), (256, 384), (384, 513))


def stack_input(name):
    """The fixed input of a stack: magnitudes in [0, 4), multiples of 2^-10"""
    shape = STACK_INPUTS[name]
    return (4. * hashed(shape[0] * shape[2] * shape[3],
                        5000 if name == 'cmb' else 6000)).float().reshape(shape)


def coefficients(name, shapes_of_maps):
    """The fixed linear functional: one fp32 tensor per map (the last is the
    logits), in [-.5, .5) for the maps and in [0, 1) for the logits, whose
    bias gradient would otherwise be a cancelling sum (tests/fdisc_oracle.py,
    coefficients)"""
    return conv_oracle.hashed_coefficients(
        shapes_of_maps, 7000 + (100 if name == 'r' else 0))


###############################################################################
# The stacks
###############################################################################

SLOPES = {'cmb': .1, 'r': .2}
# A pre-activation this close to zero, relative to the RMS of its layer, is
# fragile: 64 x 3e-6, the fp32 error of a layer (FP32_RECORDED): its side of
# the mask cannot be told in fp32
FRAGILE = 2e-4


def chain(x, parameters_, prefixes, slope, defect=None):
    """The five layers of a band / of R -> (last map, maps, saved)"""
    maps, saved = [], []
    for prefix, (_, _, _, stride) in zip(prefixes, LAYERS):
        weight = weight_norm(
            parameters_[prefix + 'weight_g'], parameters_[prefix + 'weight_v'])
        z = pre_activation(x, weight, parameters_[prefix + 'bias'], stride)
        y = leaky(z, slope)
        saved.append((prefix, x.double(), weight, y, z, stride, slope))
        maps.append(z if defect == 'maps_before_activation' else y)
        x = y
    return x, maps, saved


def prefixes_of(name, band=0):
    if name == 'cmb':
        return [f'band_convs.{band}.{index}.0.' for index in range(5)]
    return [f'convs.{index}.' for index in range(5)]


def stack(name, inputs_, parameters_, defect=None):
    """inputs_: the band tensors ('cmb') or [x] ('r') -> (logits, every map
    in the reference's order, the logits last, what the backward needs)"""
    last, maps, saved = [], [], []
    for band, x in enumerate(inputs_):
        y, chain_maps, chain_saved = chain(
            x.double(), parameters_, prefixes_of(name, band), SLOPES[name],
            defect)
        last.append(y)
        maps += chain_maps
        saved.append(chain_saved)
    if defect == 'bands_wrong_order':
        last = last[::-1]
    joined = torch.cat(last, dim=-1)
    weight = weight_norm(
        parameters_['conv_post.weight_g'], parameters_['conv_post.weight_v'])
    logits = layer(
        joined, weight, parameters_['conv_post.bias'], 1,
        SLOPES[name] if defect == 'activation_after_post' else 1.)
    post = ('conv_post.', joined, weight, logits, None, 1, 1.)
    return logits, maps + [logits], (saved, post)


def stack_backward(saved, parameters_, upstreams, mend=False):
    """upstreams: the gradient at every map (the logits last) -> (gradients in
    the inputs, {key: gradient}, the upstreams as used). With `mend`, the
    upstream of a fragile element is replaced by minus what the later layers
    carry to it, rounded to fp32: its gz is then zero to 2^-24 whichever side
    of the mask it is on."""
    chains, post = saved
    upstreams = [u.double().clone() for u in upstreams]
    gradients = {}

    def one(record, total):
        prefix, x, weight, y, _, stride, slope = record
        carried, grad_weight, grad_bias = layer_backward(
            x, weight, y, total, stride, slope)
        grad_g, grad_v = weight_norm_backward(
            grad_weight, parameters_[prefix + 'weight_g'],
            parameters_[prefix + 'weight_v'])
        gradients[prefix + 'weight_g'] = grad_g
        gradients[prefix + 'weight_v'] = grad_v
        gradients[prefix + 'bias'] = grad_bias
        return carried

    joined = one(post, upstreams[-1])
    grad_inputs, column = [], 0
    for band, records in enumerate(chains):
        width = records[-1][3].shape[3]
        carried = joined[..., column:column + width]
        column += width
        for index in reversed(range(len(records))):
            upstream = upstreams[band * len(records) + index]
            if mend:
                z = records[index][4]
                fragile = z.abs() < FRAGILE * z.pow(2).mean().sqrt()
                upstream[fragile] = (-carried[fragile]).float().double()
            carried = one(records[index], upstream + carried)
        grad_inputs.append(carried)
    return grad_inputs, gradients, [u.float() for u in upstreams]


def golden_coefficients(golden, name):
    """The functional of the golden: the closed form, mended where the golden
    says"""
    kept = golden['stacks'][name]
    return conv_oracle.golden_coefficients(
        kept, coefficients(name, kept['map_shapes']))


def stack_figures(golden, name, logits, maps, grad_x, gradients):
    """[(label, quantity, figure)] of a stack's results against the golden:
    the comparison of the GPU tests. `maps` without the logits; `gradients`
    {key: tensor}."""
    kept = golden['stacks'][name]
    return conv_oracle.stack_figures(
        golden, kept, logits, maps, grad_x, kept['gradient_x'], gradients)


###############################################################################
# The inputs of the cases, the truth and the figures
###############################################################################


def inputs(name, seed=0):
    """fp32: x, upstream Gaussian; weight and bias from Conv2d's default
    initialisation, seeded without touching the global generator"""
    channels, out_channels, kernel_width, stride, height, width, _ = \
        ALL_CASES[name]
    index = list(ALL_CASES).index(name)
    generator = torch.Generator().manual_seed(seed * 1000 + index)
    x = torch.randn(BATCH, channels, height, width, generator=generator)
    upstream = torch.randn(
        BATCH, out_channels, height, (width - 1) // stride + 1,
        generator=generator)
    weight, bias = conv_oracle.conv_parameters(
        torch.nn.Conv2d, seed * 1000 + 500 + index, channels, out_channels,
        (3, kernel_width))
    return x, weight, bias, upstream


def reference_fp32(x, weight, bias, stride, slope, dtype=torch.float32,
                   upstream=None):
    """The reference's own arithmetic: conv2d and leaky_relu with autograd in
    `dtype` on the CPU -> pre-activation, output and, with an upstream
    gradient, (gx, gW, gb)"""
    x = x.to(dtype).clone().requires_grad_(True)
    weight = weight.to(dtype).clone().requires_grad_(True)
    bias = bias.to(dtype).clone().requires_grad_(True)
    z = torch.nn.functional.conv2d(
        x, weight, bias, stride=(1, stride),
        padding=(1, (weight.shape[3] - 1) // 2))
    y = z if slope == 1. else torch.nn.functional.leaky_relu(z, slope)
    if upstream is None:
        return z.detach(), y.detach(), None
    y.backward(upstream.to(dtype))
    return z.detach(), y.detach(), (x.grad, weight.grad, bias.grad)


# The truth of a case (the kink is that of a slope other than 1), the figures
# of a result against it and those of the reference's own arithmetic in fp32
_TRUTHS = conv_oracle.Truths(
    inputs,
    lambda name, x, weight, bias: pre_activation(
        x, weight, bias, ALL_CASES[name][3]),
    lambda name: ALL_CASES[name][6] != 1.,
    lambda name, z: leaky(z, ALL_CASES[name][6]),
    lambda name, x, weight, y, upstream: layer_backward(
        x, weight, y, upstream, ALL_CASES[name][3], ALL_CASES[name][6]),
    lambda name, x, weight, bias, dtype, upstream: reference_fp32(
        x, weight, bias, ALL_CASES[name][3], ALL_CASES[name][6], dtype,
        upstream))
truth, figures = _TRUTHS.truth, _TRUTHS.figures
fp32_figures = _TRUTHS.fp32_figures



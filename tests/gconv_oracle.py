"""A float64 restatement of one conv of the generator's MRF Block
(promonet/model/hifigan.py:198-210) with its input activation and its
residual add,
    y = conv1d(leaky(x, slope), W, b, dilation d, padding (k - 1) d / 2) [+ r]
with the zero padding explicit and the taps an explicit loop (no conv1d), its
gradients gx, gW and gb written out by hand from the upstream gradient and
the INPUT, and the compositions Block, ResidualBlock on it. `defect` plants
one wrong reading (LAYER_DEFECTS, MODULE_DEFECTS): the comparisons of the GPU
tests must reject each of them (tests/test_cpu_gconv.py).

Also the closed-form parameters of the modules (the multiplicative hash of
tests/conv_oracle.py), the cases of the tests, their seeded inputs, the
figures of the comparison and the gates.
"""
import re
from pathlib import Path

import torch

import conv_oracle
from conv_oracle import (  # noqa: F401 (used by the tests through here)
    QUANTITIES, figure, hashed, integers, leaky, weight_norm,
    weight_norm_backward)

ROOT = Path(__file__).resolve().parent.parent

LAYER_DEFECTS = (
    'gx_dilation_ignored', 'gx_taps_not_mirrored', 'gate_from_output',
    'zero_gated_as_one', 'slope_left_out_of_gw', 'padding_reads_neighbour',
    'residual_twice')
MODULE_DEFECTS = (
    'residual_gradient_dropped', 'conv2_dilated', 'no_division',
    'kernels_permuted')
CHANNELS = (32, 64, 128, 256)
KERNELS = (3, 7, 11)
DILATIONS = (1, 3, 5)
SLOPE = .1
# the Blocks of a ResidualBlock: HIFIGAN_RESBLOCK_KERNEL_SIZES / _DILATION_SIZES
BLOCKS = ((3, (1, 3, 5)), (7, (1, 3, 5)), (11, (1, 3, 5)))


def kernel_constants():
    """The tile constants of the kernels, read from their header"""
    text = (ROOT / 'promonet_amd' / 'csrc' / 'pm_gconv.h').read_text()
    return {name: int(value) for name, value in re.findall(
        r'#define (GC_[A-Z_]+) (\d+)\b', text)}


CONSTANTS = kernel_constants()


def split(batch, channels, frames):
    """(partials, K chunks of each) of gW: the host's split_of (pm_gconv.hip)
    restated; tests/test_cpu_gconv.py holds it against the workspace query"""
    pix, least = CONSTANTS['GC_GW_PIX'], CONSTANTS['GC_GW_MIN_CHUNKS']
    chunks = -(-batch * frames // pix)
    tiles = (channels // (32 if channels < 64 else 64)) * \
        (channels // CONSTANTS['GC_GW_CT'])
    want = min(-(-chunks // least),
               max(CONSTANTS['GC_GW_WORKGROUPS'] // tiles, 1))
    each = -(-chunks // want)
    return -(-chunks // each), each


def _large_frames(batch, channels, sign):
    """The smallest 16 n + sign frames past one pixel tile of the forward, one
    K chunk of gW and one gW partial at that size"""
    n = 1
    while True:
        frames = 16 * n + sign
        if frames > CONSTANTS['GC_NT'] and frames > CONSTANTS['GC_GW_PIX'] * \
                split(batch, channels, frames)[1] and frames >= 340:
            return frames
        n += 1


# name: (C, k, d, B, T)
CASES = {
    f'form-{c}-{k}-{d}': (c, k, d, 2, 37)
    for c in CHANNELS for k in KERNELS for d in DILATIONS}
CASES.update({
    # one frame: every tap but the centre is padding
    'short-32-1': (32, 11, 5, 2, 1),
    'short-32-5': (32, 11, 5, 2, 5),
    'short-256-1': (256, 3, 1, 2, 1),
    'short-256-5': (256, 3, 1, 2, 5),
    # the reach of one side is 25: the outermost taps never and once inside
    'short-64-25': (64, 11, 5, 2, 25),
    'short-64-26': (64, 11, 5, 2, 26),
    # past one pixel tile, one K chunk and one gW partial; the tiles cross the
    # batch rows
    'large-32': (32, 7, 3, 3, _large_frames(3, 32, -1)),
    'large-128': (128, 11, 5, 3, _large_frames(3, 128, 1)),
})
SLOPES = (SLOPE, 1.)
# the integer cases of the exact test, and their slopes
EXACT_CASES = ('form-32-3-1', 'form-64-7-3', 'form-128-11-5', 'form-256-3-5',
               'form-256-11-1', 'short-32-1', 'short-64-25', 'short-64-26',
               'large-32', 'large-128')
EXACT_SLOPES = (.5, 1.)
# The largest error of the reference's own arithmetic in fp32 (leaky_relu and
# conv1d with autograd on the build host's CPU) against this oracle, per case,
# the larger of the two slopes, relative to the RMS of the true quantity
# (fp32_figures; printed by tests/test_cpu_gconv.py). The gates stand on
# these.
FP32_RECORDED = {
    'form-32-3-1': (7.869e-07, 8.948e-07, 7.585e-07, 3.214e-07),
    'form-32-3-3': (9.858e-07, 1.015e-06, 7.049e-07, 3.214e-07),
    'form-32-3-5': (6.599e-07, 9.784e-07, 8.565e-07, 1.948e-07),
    'form-32-7-1': (8.345e-07, 1.861e-06, 6.616e-07, 2.493e-07),
    'form-32-7-3': (9.216e-07, 1.600e-06, 6.925e-07, 3.422e-07),
    'form-32-7-5': (9.700e-07, 2.116e-06, 8.655e-07, 2.053e-07),
    'form-32-11-1': (1.394e-06, 1.790e-06, 8.417e-07, 3.015e-07),
    'form-32-11-3': (1.219e-06, 1.628e-06, 7.923e-07, 3.517e-07),
    'form-32-11-5': (1.102e-06, 1.324e-06, 7.629e-07, 2.956e-07),
    'form-64-3-1': (7.701e-07, 1.157e-06, 1.203e-06, 3.169e-07),
    'form-64-3-3': (6.287e-07, 1.098e-06, 1.266e-06, 2.476e-07),
    'form-64-3-5': (6.774e-07, 1.041e-06, 1.125e-06, 3.757e-07),
    'form-64-7-1': (9.814e-07, 1.273e-06, 1.286e-06, 3.778e-07),
    'form-64-7-3': (9.589e-07, 1.312e-06, 1.118e-06, 3.251e-07),
    'form-64-7-5': (1.253e-06, 1.406e-06, 1.393e-06, 3.617e-07),
    'form-64-11-1': (1.072e-06, 1.566e-06, 1.211e-06, 2.372e-07),
    'form-64-11-3': (1.215e-06, 1.556e-06, 1.502e-06, 2.885e-07),
    'form-64-11-5': (1.054e-06, 1.397e-06, 1.762e-06, 3.637e-07),
    'form-128-3-1': (7.710e-07, 9.198e-07, 1.410e-06, 6.650e-07),
    'form-128-3-3': (8.332e-07, 1.148e-06, 1.386e-06, 6.511e-07),
    'form-128-3-5': (7.763e-07, 1.041e-06, 1.509e-06, 6.011e-07),
    'form-128-7-1': (1.150e-06, 1.753e-06, 1.361e-06, 4.922e-07),
    'form-128-7-3': (1.005e-06, 1.628e-06, 1.539e-06, 4.936e-07),
    'form-128-7-5': (8.387e-07, 1.342e-06, 1.874e-06, 4.157e-07),
    'form-128-11-1': (1.235e-06, 2.050e-06, 1.756e-06, 6.193e-07),
    'form-128-11-3': (1.056e-06, 1.458e-06, 1.385e-06, 5.468e-07),
    'form-128-11-5': (1.045e-06, 1.399e-06, 2.209e-06, 4.734e-07),
    'form-256-3-1': (8.079e-07, 1.244e-06, 1.431e-06, 5.826e-07),
    'form-256-3-3': (7.121e-07, 1.053e-06, 1.838e-06, 5.746e-07),
    'form-256-3-5': (9.115e-07, 1.109e-06, 1.778e-06, 7.471e-07),
    'form-256-7-1': (1.081e-06, 1.422e-06, 1.572e-06, 5.731e-07),
    'form-256-7-3': (9.347e-07, 1.720e-06, 1.831e-06, 8.363e-07),
    'form-256-7-5': (1.047e-06, 1.408e-06, 1.920e-06, 6.894e-07),
    'form-256-11-1': (1.104e-06, 1.740e-06, 1.924e-06, 6.755e-07),
    'form-256-11-3': (1.290e-06, 1.645e-06, 1.722e-06, 4.836e-07),
    'form-256-11-5': (9.757e-07, 1.467e-06, 1.946e-06, 7.367e-07),
    'short-32-1': (2.394e-07, 3.401e-07, 9.827e-07, 6.771e-08),
    'short-32-5': (4.550e-07, 6.509e-07, 1.164e-06, 1.511e-07),
    'short-256-1': (4.082e-07, 6.952e-07, 8.661e-07, 9.109e-08),
    'short-256-5': (7.218e-07, 1.300e-06, 8.608e-07, 3.275e-07),
    'short-64-25': (7.756e-07, 1.609e-06, 1.124e-06, 2.522e-07),
    'short-64-26': (7.972e-07, 1.318e-06, 1.526e-06, 3.384e-07),
    'large-32': (1.404e-06, 1.757e-06, 3.488e-06, 5.842e-07),
    'large-128': (1.392e-06, 1.985e-06, 5.164e-06, 2.408e-06),
}
# What one MI355X showed on the same cases, the largest over the table per
# quantity (tests/test_gpu_gconv.py prints every case; the largest forward and
# gx are those of 'form-256-11-1'): for the record, the gates do not stand on
# them
DEVICE_RECORDED = (3.016e-06, 5.358e-06, 1.893e-06, 8.363e-07)


def gate(quantity):
    return conv_oracle.gate(FP32_RECORDED, quantity)


###############################################################################
# The layer
###############################################################################


def padded(x, reach, defect=None):
    """x (B, C, T) with `reach` zeros on either side of every batch row"""
    batch, channels, frames = x.shape
    out = x.new_zeros(batch, channels, frames + 2 * reach)
    out[:, :, reach:reach + frames] = x
    if defect == 'padding_reads_neighbour':
        # the padding holds what lies there in memory (B, T, C): the end of
        # the batch row before, the start of the one after
        width = min(reach, frames)
        for b in range(batch):
            if b:
                out[b, :, reach - width:reach] = x[b - 1, :, frames - width:]
            if b + 1 < batch:
                out[b, :, reach + frames:reach + frames + width] = \
                    x[b + 1, :, :width]
    return out


def layer(x, weight, bias, dilation, slope, residual=None, defect=None):
    """The forward. Built of differentiable torch ops (no conv1d), so that the
    compositions may take their gradients by autograd in float64."""
    x, weight, bias = x.double(), weight.double(), bias.double()
    kernel, frames = weight.shape[2], x.shape[2]
    source = padded(leaky(x, slope), (kernel - 1) // 2 * dilation, defect)
    y = bias[None, :, None]
    for tap in range(kernel):
        y = y + torch.einsum(
            'oc,bct->bot', weight[:, :, tap],
            source[:, :, tap * dilation:tap * dilation + frames])
    if residual is not None:
        y = y + residual.double() * (2. if defect == 'residual_twice' else 1.)
    return y


def layer_backward(x, weight, upstream, dilation, slope, defect=None, y=None):
    """(gx, gW, gb) from the upstream gradient and the input, by hand"""
    x, weight, upstream = x.double(), weight.double(), upstream.double()
    kernel, frames = weight.shape[2], x.shape[2]
    half = (kernel - 1) // 2
    reach = half * dilation
    operand = x if defect == 'slope_left_out_of_gw' else leaky(x, slope)
    source = padded(operand, reach, defect)
    spread = dilation
    if defect == 'gx_dilation_ignored':
        spread = 1
    shown = padded(upstream, half * spread)
    grad = torch.zeros_like(x)
    grad_weight = torch.zeros_like(weight)
    for tap in range(kernel):
        # gx[t] reads the upstream gradient at t - (tap - half) d
        at = (kernel - 1 - tap) * spread
        if defect == 'gx_taps_not_mirrored':
            at = tap * spread
        grad = grad + torch.einsum(
            'oc,bot->bct', weight[:, :, tap], shown[:, :, at:at + frames])
        grad_weight[:, :, tap] = torch.einsum(
            'bot,bct->oc', upstream,
            source[:, :, tap * dilation:tap * dilation + frames])
    mask = x > 0.
    if defect == 'zero_gated_as_one':
        mask = x >= 0.
    if defect == 'gate_from_output':
        mask = y > 0.
    grad_x = torch.where(mask, grad, grad * slope)
    return grad_x, grad_weight, upstream.sum((0, 2))


def reference(x, weight, bias, dilation, slope, residual=None, upstream=None,
              dtype=torch.float32):
    """The reference's own arithmetic: leaky_relu and conv1d with autograd in
    `dtype` on the CPU -> (y, (gx, gW, gb) or None)"""
    x = x.to(dtype).clone().requires_grad_(True)
    weight = weight.to(dtype).clone().requires_grad_(True)
    bias = bias.to(dtype).clone().requires_grad_(True)
    kernel = weight.shape[2]
    xt = x if slope == 1. else torch.nn.functional.leaky_relu(x, slope)
    y = torch.nn.functional.conv1d(
        xt, weight, bias, dilation=dilation,
        padding=(kernel - 1) // 2 * dilation)
    if residual is not None:
        y = y + residual.to(dtype)
    if upstream is None:
        return y.detach(), None
    y.backward(upstream.to(dtype))
    return y.detach(), (x.grad, weight.grad, bias.grad)


###############################################################################
# The inputs of the cases, the truth and the figures
###############################################################################


def inputs(name, exact=False):
    """fp32: x (B, C, T) Gaussian with exact zeros planted, upstream and
    residual Gaussian; weight and bias from Conv1d's default initialisation,
    seeded without touching the global generator. `exact`: integers, x,
    upstream and residual in [-4, 4], weight and bias in [-2, 2]."""
    channels, kernel, _, batch, frames = CASES[name]
    index = list(CASES).index(name)
    generator = torch.Generator().manual_seed(index + (5000 if exact else 0))
    shape = (batch, channels, frames)
    if exact:
        x, upstream, residual = (
            integers(shape, generator) for _ in range(3))
        weight = integers((channels, channels, kernel), generator, -2, 2)
        bias = integers((channels,), generator, -2, 2)
        return x, weight, bias, upstream, residual
    x, upstream, residual = (
        torch.randn(shape, generator=generator) for _ in range(3))
    x.view(-1)[::7] = 0.
    weight, bias = conv_oracle.conv_parameters(
        torch.nn.Conv1d, 500 + index, channels, channels, kernel)
    return x, weight, bias, upstream, residual


# (its own truth: no fragile mask, the kink is at the seeded input and not at
# a computed pre-activation, and a case has two slopes and a residual)
_TRUTH = {}


def truth(name, slope, exact=False):
    """The case in float64, computed once and shared: the inputs, y without
    and with the residual, gx, gW, gb"""
    key = (name, slope, exact)
    if key not in _TRUTH:
        dilation = CASES[name][2]
        x, weight, bias, upstream, residual = inputs(name, exact)
        y = layer(x, weight, bias, dilation, slope)
        gx, gw, gb = layer_backward(x, weight, upstream, dilation, slope)
        _TRUTH[key] = {
            'x': x, 'weight': weight, 'bias': bias, 'upstream': upstream,
            'residual': residual, 'forward': y,
            'forward_residual': y + residual.double(), 'gx': gx, 'gW': gw,
            'gb': gb}
    return _TRUTH[key]


def figures(name, slope, forward, gx, gw, gb, residual=False):
    """The four figures of a result against the truth of the case"""
    want = truth(name, slope)
    return (figure(forward, want[
                'forward_residual' if residual else 'forward']),
            figure(gx, want['gx']), figure(gw, want['gW']),
            figure(gb, want['gb']))


def fp32_figures(name):
    """The figures of the reference's own arithmetic in fp32 on this CPU, the
    larger of the slopes and of with and without the residual"""
    worst = (0.,) * 4
    for slope in SLOPES:
        for with_residual in (False, True):
            want = truth(name, slope)
            y, gradients = reference(
                want['x'], want['weight'], want['bias'], CASES[name][2],
                slope, want['residual'] if with_residual else None,
                want['upstream'])
            got = figures(name, slope, y, *gradients, residual=with_residual)
            worst = tuple(max(a, b) for a, b in zip(worst, got))
    return worst


###############################################################################
# The modules: closed-form parameters (exact in fp32, the same on every
# machine: no RNG, no libm), the float64 compositions
###############################################################################

MODULE_CHANNELS, MODULE_BATCH, MODULE_FRAMES = 32, 2, 48
# a computed leaky input this close to zero, relative to the RMS of its map,
# is fragile: 64 x the largest recorded forward figure of a layer. Its side of
# the mask cannot be told in fp32. The seeds of the module inputs are chosen
# so that there is none (tests/test_cpu_gconv.py asserts it).
MODULE_SEEDS = {'block-3': 2, 'block-7': 3, 'block-11': 8, 'residual': 48}


def fragile_bound():
    return 64. * gate('forward') / 4.


def block_shapes(channels, kernel, prefix=''):
    """{key: shape} of the state_dict of Block, in its order"""
    out = {}
    for name in ('convs1', 'convs2'):
        for index in range(3):
            out[f'{prefix}{name}.{index}.bias'] = (channels,)
            out[f'{prefix}{name}.{index}.weight_g'] = (channels, 1, 1)
            out[f'{prefix}{name}.{index}.weight_v'] = (
                channels, channels, kernel)
    return out


def residual_shapes(channels):
    out = {}
    for index, (kernel, _) in enumerate(BLOCKS):
        out.update(block_shapes(channels, kernel, f'model.{index}.'))
    return out


def parameters(shapes, salt):
    """{key: fp32 tensor}: weight_v in [-.5, .5), bias in [-.125, .125),
    weight_g in [.5, 1.25)"""
    return conv_oracle.hashed_parameters(shapes, 3000 + 100 * salt)


def module_inputs(name):
    """(x, upstream) fp32 (B, C, T) of a module case at its seed"""
    generator = torch.Generator().manual_seed(
        9000 + 1000 * list(MODULE_SEEDS).index(name) + MODULE_SEEDS[name])
    shape = (MODULE_BATCH, MODULE_CHANNELS, MODULE_FRAMES)
    return (torch.randn(shape, generator=generator),
            torch.randn(shape, generator=generator))


def block(x, parameters_, kernel, dilations, prefix='', defect=None,
          leaky_inputs=None):
    """Block.forward (:198-210) in float64 on `layer`; the computed inputs of
    its activations are appended to `leaky_inputs`"""
    x = x.double()
    for index, dilation in enumerate(dilations):
        def weights(name):
            base = f'{prefix}{name}.{index}.'
            return (weight_norm(parameters_[base + 'weight_g'],
                                parameters_[base + 'weight_v']),
                    parameters_[base + 'bias'])
        if leaky_inputs is not None and index:
            leaky_inputs.append(x)
        xt = layer(x, *weights('convs1'), dilation, SLOPE)
        if leaky_inputs is not None:
            leaky_inputs.append(xt)
        skip = x.detach() if defect == 'residual_gradient_dropped' else x
        x = layer(xt, *weights('convs2'),
                  dilation if defect == 'conv2_dilated' else 1, SLOPE,
                  residual=skip)
    return x


def residual_block(x, parameters_, defect=None, leaky_inputs=None):
    """ResidualBlock.forward (:141-145)"""
    kernels = [kernel for kernel, _ in BLOCKS]
    if defect == 'kernels_permuted':
        kernels = kernels[1:] + kernels[:1]
    total = None
    for index, (_, dilations) in enumerate(BLOCKS):
        prefix = f'model.{index}.'
        # (a permuted kernel size reads the centre taps of its weight, or the
        # weight centred in zeros)
        used = parameters_
        if kernels[index] != BLOCKS[index][0]:
            used = dict(parameters_)
            for key, value in parameters_.items():
                if key.startswith(prefix) and key.endswith('weight_v'):
                    used[key] = _resized(value, kernels[index])
        y = block(x, used, kernels[index], dilations, prefix,
                  None if defect in ('no_division', 'kernels_permuted')
                  else defect, leaky_inputs)
        total = y if total is None else total + y
    return total if defect == 'no_division' else total / len(BLOCKS)


def _resized(weight, kernel):
    have = weight.shape[2]
    if kernel <= have:
        first = (have - kernel) // 2
        return weight[:, :, first:first + kernel]
    out = weight.new_zeros(*weight.shape[:2], kernel)
    first = (kernel - have) // 2
    out[:, :, first:first + have] = weight
    return out


def module_case(name):
    """(forward function of (x, parameters), parameters) of a module case"""
    if name == 'residual':
        return residual_block, parameters(
            residual_shapes(MODULE_CHANNELS), 50)
    kernel = int(name.split('-')[1])
    dilations = dict(BLOCKS)[kernel]

    def forward(x, parameters_, defect=None, leaky_inputs=None):
        return block(x, parameters_, kernel, dilations, '', defect,
                     leaky_inputs)
    return forward, parameters(block_shapes(MODULE_CHANNELS, kernel), kernel)


_MODULE_TRUTH = {}


def module_truth(name, defect=None):
    """A module case in float64 with autograd over `layer`: x, upstream, the
    parameters, the output, gx, {key: gradient}, the fragile count"""
    key = (name, defect)
    if key not in _MODULE_TRUTH:
        forward, parameters_ = module_case(name)
        x, upstream = module_inputs(name)
        leaf = x.double().requires_grad_(True)
        leaves = {k: v.double().requires_grad_(True)
                  for k, v in parameters_.items()}
        seen = []
        y = forward(leaf, leaves, defect=defect, leaky_inputs=seen)
        y.backward(upstream.double())
        bound = fragile_bound()
        fragile = sum(
            (z.abs() < bound * z.pow(2).mean().sqrt()).sum().item()
            for z in seen)
        _MODULE_TRUTH[key] = {
            'x': x, 'upstream': upstream, 'parameters': parameters_,
            'forward': y.detach(), 'gx': leaf.grad,
            'gradients': {k: v.grad for k, v in leaves.items()},
            'fragile': fragile}
    return _MODULE_TRUTH[key]


def module_reference(name, dtype=torch.float32):
    """The same composition on torch's own ops (leaky_relu, conv1d,
    _weight_norm) with autograd in `dtype` on the CPU -> (y, gx, {key:
    gradient})"""
    _, parameters_ = module_case(name)
    x, upstream = module_inputs(name)
    leaf = x.to(dtype).requires_grad_(True)
    leaves = {k: v.to(dtype).requires_grad_(True)
              for k, v in parameters_.items()}
    functional = torch.nn.functional

    def one(x, prefix, kernel, dilations):
        for index, dilation in enumerate(dilations):
            for part, d in (('convs1', dilation), ('convs2', 1)):
                base = f'{prefix}{part}.{index}.'
                weight = torch._weight_norm(
                    leaves[base + 'weight_v'], leaves[base + 'weight_g'], 0)
                xt = functional.conv1d(
                    functional.leaky_relu(x if part == 'convs1' else xt,
                                          SLOPE),
                    weight, leaves[base + 'bias'], dilation=d,
                    padding=(kernel - 1) // 2 * d)
            x = xt + x
        return x

    if name == 'residual':
        y = sum(one(leaf, f'model.{index}.', kernel, dilations)
                for index, (kernel, dilations) in enumerate(BLOCKS)) / \
            len(BLOCKS)
    else:
        kernel = int(name.split('-')[1])
        y = one(leaf, '', kernel, dict(BLOCKS)[kernel])
    y.backward(upstream.to(dtype))
    return y.detach(), leaf.grad, {k: v.grad for k, v in leaves.items()}


def module_figures(name, forward, gx, gradients, defect=None):
    """(forward, gx, gW, gb): the figures of a module's results against the
    truth, the weight gradients (weight_g, weight_v) and the bias gradients
    each the largest over the keys"""
    want = module_truth(name, defect)
    worst_w = worst_b = 0.
    for key, value in want['gradients'].items():
        got = figure(gradients[key], value)
        if key.endswith('bias'):
            worst_b = max(worst_b, got)
        else:
            worst_w = max(worst_w, got)
    return (figure(forward, want['forward']), figure(gx, want['gx']), worst_w,
            worst_b)


# The figures of module_reference in fp32 on the build host's CPU (forward,
# gx, weight gradients, bias gradients); the module gates are 4 x these
MODULE_RECORDED = {
    'block-3': (3.932e-07, 7.355e-07, 1.630e-06, 8.459e-07),
    'block-7': (9.388e-07, 1.122e-06, 3.211e-06, 8.827e-07),
    'block-11': (9.199e-07, 1.082e-06, 2.863e-06, 1.176e-06),
    'residual': (4.427e-07, 7.166e-07, 3.080e-06, 1.359e-06),
}


def module_gates():
    """Per quantity, 4 x the largest recorded figure over the module cases"""
    return tuple(4. * max(values) for values in zip(*MODULE_RECORDED.values()))


###############################################################################
# The whole vocoder: oracle/restatement.py: hifigan_forward with autograd on
# the CPU, in float64 (the truth) and in fp32 (the recorded figures)
###############################################################################

TRAINABLE_SEED, TRAINABLE_BATCH, TRAINABLE_FRAMES = 0, 2, 2
TRAINABLE_QUANTITIES = ('forward', 'gx', 'gg', 'gW', 'gb')


def trainable_state():
    """{key: fp32 tensor} of the vocoder under the keys of HiFiGAN"""
    import restatement
    return {key[len('model.'):]: value
            for key, value in restatement.random_state(TRAINABLE_SEED).items()
            if key.startswith('model.')}


def trainable_inputs():
    """fp32: features (B, 113, T), globals (B, 258, 1), upstream (B, 1, T
    hop)"""
    import restatement
    generator = torch.Generator().manual_seed(77)
    hop = 1
    for rate in restatement.UPSAMPLE_RATES:
        hop *= rate
    return (torch.randn(TRAINABLE_BATCH, restatement.NUM_FEATURES,
                        TRAINABLE_FRAMES, generator=generator),
            torch.randn(TRAINABLE_BATCH, restatement.GLOBAL_CHANNELS, 1,
                        generator=generator),
            torch.randn(TRAINABLE_BATCH, 1, TRAINABLE_FRAMES * hop,
                        generator=generator))


_TRAINABLE = {}


def trainable_run(dtype):
    """(y, gx, gg, {key: gradient}) of the restatement in `dtype`, once"""
    import restatement
    if dtype not in _TRAINABLE:
        features, global_features, upstream = trainable_inputs()
        x = features.to(dtype).requires_grad_(True)
        g = global_features.to(dtype).requires_grad_(True)
        leaves = {key: value.to(dtype).requires_grad_(True)
                  for key, value in trainable_state().items()}
        y = restatement.hifigan_forward(
            x, g, {'model.' + key: value for key, value in leaves.items()})
        y.backward(upstream.to(dtype))
        _TRAINABLE[dtype] = (
            y.detach(), x.grad, g.grad,
            {key: value.grad for key, value in leaves.items()})
    return _TRAINABLE[dtype]


def trainable_figures(forward, gx, gg, gradients):
    """(forward, gx, gg, gW, gb) against the float64 run; gW and gb the
    largest over the weight keys (weight, weight_g, weight_v) and the biases"""
    want = trainable_run(torch.float64)
    worst_w = worst_b = 0.
    for key, value in want[3].items():
        got = figure(gradients[key], value)
        if key.endswith('bias'):
            worst_b = max(worst_b, got)
        else:
            worst_w = max(worst_w, got)
    return (figure(forward, want[0]), figure(gx, want[1]),
            figure(gg, want[2]), worst_w, worst_b)


# The figures of the same restatement in fp32 on the build host's CPU. Here a
# figure is dominated by the fp32 run's own mask flips: a leaky input that
# lies within its fp32 error of zero takes the other slope, and the gradients
# downstream of it move by far more than a rounding order. The gates are 4 x
# these.
TRAINABLE_RECORDED = (2.768e-06, 1.788e-06, 1.913e-06, 4.485e-05, 1.238e-05)


def trainable_gates():
    return tuple(4. * value for value in TRAINABLE_RECORDED)

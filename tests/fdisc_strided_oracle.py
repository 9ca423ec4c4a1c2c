"""A float64 restatement of the strided, wider layers of the FARGAN
discriminator's conv stacks (promonet/model/discriminator.py:320-389 at n_fft
128 ... 2048): one layer
    y = act(conv2d(cat(x, sin, cos), W, b, stride (s, 1), padding (1, 1))),
the embedding of FrequencyPositionalEmbedding on the layer's INPUT explicit,
the zero padding explicit, the taps explicit loops (no conv2d), gz, gx, gW and
gb written out by hand; the stack of six at any resolution and its gradients.
The leaves (weight norm, `figure`, `hashed`, `integers`, the truth of a case)
are tests/conv_oracle.py's; the formula of `coefficients` is
tests/fdisc_oracle.py's. The loops over the taps stay here: they gather each
tap's input by index (an embedding defect moves it per tap), gx is in gather
form, an input row at a time, and its defects reach into that loop. `defect`
plants one wrong reading of the layer (DEFECTS): the comparisons of the GPU
tests must reject each of them (tests/test_cpu_fdisc_strided.py).

Also the cases of the tests, their seeded inputs, the hashed parameters of the
stacks, the figures of the comparison and the gates.
"""
import math
import re
from pathlib import Path

import torch

import conv_oracle
from conv_oracle import (  # noqa: F401 (used by the tests through here)
    QUANTITIES, activate, figure, hashed, integers, weight_norm,
    weight_norm_backward)

ROOT = Path(__file__).resolve().parent.parent

DEFECTS = (
    'stride_on_time', 'half_bins', 'angle_from_output',
    'embedding_at_output_row', 'embedding_unpadded_frequency',
    'embedding_weights_first_channels', 'gx_parities_exchanged',
    'gx_row_past_end', 'k_block_dropped', 'k_block_twice',
    'row_block_overwritten', 'gw_later_blocks_dropped',
    'gw_embedding_dropped')


def kernel_constants():
    """The tile constants of the kernels, read from their header"""
    text = (ROOT / 'promonet_amd' / 'csrc' / 'pm_fdisc_strided.h').read_text()
    return {name: int(value) for name, value in re.findall(
        r'#define (FS_[A-Z_]+) (\d+)\b', text)}


CONSTANTS = kernel_constants()
NT, KC = CONSTANTS['FS_NT'], CONSTANTS['FS_KC']
GW_PIX, EDGE = CONSTANTS['FS_GW_PIX'], CONSTANTS['FS_EDGE_CHUNK']
BATCH = 2
# (C, O, F, T, s, activation): the smallest shapes that reach each thing that
# can go wrong
CASES = {
    # odd F: every odd input row has both its taps
    'first-odd': (1, 16, 33, 5, 2, 'relu'),
    # even F: the last odd input row has tap 2 alone (no output row F')
    'first-even': (1, 16, 34, 5, 2, 'relu'),
    # T = 1: both time borders at once, one K chunk a frequency tap
    'one-frame': (16, 32, 9, 1, 2, 'relu'),
    # F' = 1 from two rows: tap 0 outside; the odd row reaches tap 2 alone
    'two-bins': (32, 64, 2, 3, 2, 'relu'),
    # F' = 1 from one row: two taps of three outside, no odd row at all
    'one-bin': (32, 64, 1, 3, 2, 'relu'),
    # the most K chunks (24 forward, 16 and 32 in gx) and row blocks (four
    # row tiles of four blocks)
    'widest': (128, 256, 9, 5, 2, 'relu'),
    'widest-stride-1': (128, 256, 5, 3, 1, 'relu'),
    # 70 pixels: no multiple of the tile of FS_NT, and the first tile crosses
    # the batch row at pixel 35 and frequency rows every 5
    'square': (64, 64, 7, NT // 2 // 7 + 1, 1, 'relu'),
    'last': (256, 1, 5, 3, 1, 'sigmoid'),
    # 98 output pixels: two workgroups of the GEMM a row tile, four gW
    # partials of two chunks of FS_GW_PIX, the last chunk two pixels: a step
    # of four that is half empty
    'large': (16, 32, 13, (NT + 2 * GW_PIX) // (BATCH * 7) + 1, 2, 'relu'),
    # the edge kernels past one gW partial of FS_EDGE_CHUNK pixels
    'first-large': (1, 16, 34, EDGE // (BATCH * 17) + 1, 2, 'relu'),
    'last-large': (32, 1, 9, EDGE // (BATCH * 9) + 5, 1, 'sigmoid'),
}
# The largest error of the reference's own arithmetic in fp32 (torch.cat +
# conv2d + the activation, with autograd, on the build host's CPU) against
# this oracle, per case, relative to the RMS of the true quantity
# (fp32_figures; printed by tests/test_cpu_fdisc_strided.py). The gates stand
# on these.
FP32_RECORDED = {
    'first-odd': (6.770e-07, 3.137e-07, 1.128e-06, 1.556e-06),
    'first-even': (7.590e-07, 7.065e-07, 9.226e-07, 5.335e-07),
    'one-frame': (5.255e-07, 6.453e-07, 1.317e-06, 1.571e-07),
    'two-bins': (9.729e-07, 5.969e-07, 5.211e-07, 9.858e-08),
    'one-bin': (1.027e-06, 4.326e-07, 1.208e-06, 1.278e-07),
    'widest': (1.439e-06, 2.024e-06, 9.928e-07, 6.154e-07),
    'widest-stride-1': (1.230e-06, 7.932e-07, 9.067e-07, 4.995e-07),
    'square': (1.478e-06, 8.756e-07, 8.380e-07, 1.938e-07),
    'last': (1.129e-07, 4.714e-07, 6.598e-07, 1.479e-07),
    'large': (1.967e-06, 7.884e-07, 5.497e-07, 2.915e-07),
    'first-large': (1.052e-06, 8.483e-07, 3.304e-06, 9.556e-07),
    'last-large': (3.337e-07, 7.152e-07, 1.853e-06, 1.793e-06),
}


def gate(quantity):
    return conv_oracle.gate(FP32_RECORDED, quantity)


###############################################################################
# The layer
###############################################################################


def out_bins(bins, stride, defect=None):
    if defect == 'half_bins' and stride == 2:
        return bins // 2
    return (bins - 1) // stride + 1


def embedding_rows(bins, rows, stride, defect=None, table=None):
    """(sin, cos) at the input rows `rows` (a LongTensor, any of them outside
    [0, bins)): zero outside, as the conv's padding makes the channels"""
    inside = (rows >= 0) & (rows < bins)
    if table is not None:
        kept = table.double()[rows.clamp(0, bins - 1)]
        if defect != 'embedding_unpadded_frequency':
            kept = kept * inside[:, None]
        return kept[:, 0], kept[:, 1]
    period = out_bins(bins, stride) if defect == 'angle_from_output' else bins
    args = rows.double() * torch.pi * 2 / period
    sin, cos = torch.sin(args), torch.cos(args)
    if defect != 'embedding_unpadded_frequency':
        sin, cos = sin * inside, cos * inside
    return sin, cos


def tap_input(x, stride, kf, kt, defect=None, table=None):
    """cat(x, sin, cos) at tap (kf, kt) of every output pixel:
    (B, C + 2, F', T'), zero where the tap is outside the map"""
    batch, channels, bins, frames = x.shape
    sf, st = (1, stride) if defect == 'stride_on_time' else (stride, 1)
    rows_out = out_bins(bins, sf, defect)
    frames_out = (frames - 1) // st + 1
    rows = sf * torch.arange(rows_out) + kf - 1
    columns = st * torch.arange(frames_out) + kt - 1
    row_in = (rows >= 0) & (rows < bins)
    column_in = (columns >= 0) & (columns < frames)
    out = x.new_zeros(batch, channels + 2, rows_out, frames_out)
    picked = x[:, :, rows.clamp(0, bins - 1)][
        :, :, :, columns.clamp(0, frames - 1)]
    # (a choice and not a product: the padding is zero whatever the clamped
    # index holds, a non-finite value included)
    mask = row_in[:, None] & column_in[None, :]
    out[:, :channels] = torch.where(mask, picked, torch.zeros_like(picked))
    at = torch.arange(rows_out) if defect == 'embedding_at_output_row' \
        else rows
    sin, cos = embedding_rows(bins, at, sf, defect, table)
    out[:, channels] = (sin[:, None] * column_in[None, :].double())[None]
    out[:, channels + 1] = (cos[:, None] * column_in[None, :].double())[None]
    return out


def forward_weight(weight, channels, defect):
    """The weight as a wrong forward reads it"""
    weight = weight.clone()
    if defect == 'embedding_weights_first_channels':
        weight[:, channels:] = weight[:, :2]
    if defect == 'k_block_dropped' and channels >= 2 * KC:
        weight[:, KC:2 * KC] = 0.
    if defect == 'k_block_twice' and channels >= 2 * KC:
        weight[:, KC:2 * KC] *= 2.
    return weight


def pre_activation(x, weight, bias, stride, defect=None, table=None):
    x, weight, bias = x.double(), weight.double(), bias.double()
    weight = forward_weight(weight, x.shape[1], defect)
    z = None
    for kf in range(3):
        for kt in range(3):
            term = torch.einsum(
                'oc,bcft->boft', weight[:, :, kf, kt],
                tap_input(x, stride, kf, kt, defect, table))
            z = term if z is None else z + term
    z = z + bias[None, :, None, None]
    if defect == 'row_block_overwritten' and z.shape[1] >= 32:
        z[:, :16] = z[:, 16:32].clone()
    return z


def layer(x, weight, bias, stride, activation, defect=None, table=None):
    return activate(
        pre_activation(x, weight, bias, stride, defect, table), activation)


def reaching(f, stride, defect=None):
    """[(kf, output row)] of the taps that reach the input row f, the output
    row not yet held against the map: s f' + kf - 1 = f"""
    if stride == 1:
        return [(kf, f + 1 - kf) for kf in range(3)]
    j, odd = divmod(f, 2)
    if defect == 'gx_parities_exchanged':
        odd = 1 - odd
    return [(0, j + 1), (2, j)] if odd else [(1, j)]


def input_gradient(gz, weight, bins, stride, defect=None):
    """gx (B, C, F, T) in gather form, an input row at a time"""
    batch, _, rows_out, frames = gz.shape
    channels = weight.shape[1] - 2
    weight = weight[:, :channels].clone()
    if defect == 'k_block_dropped' and weight.shape[0] >= 2 * KC:
        weight[KC:2 * KC] = 0.
    if defect == 'k_block_twice' and weight.shape[0] >= 2 * KC:
        weight[KC:2 * KC] *= 2.
    gx = gz.new_zeros(batch, channels, bins, frames)
    # (B F', O, T): the rows of the map as they lie in memory
    flat = gz.transpose(1, 2).reshape(batch * rows_out, gz.shape[1], frames)
    for f in range(bins):
        for kf, source in reaching(f, stride, defect):
            if source < 0:
                continue
            if source < rows_out:
                row = gz[:, :, source]
            elif defect == 'gx_row_past_end':
                # the row after the last of a batch row: the first of the
                # next, and nothing after the last batch row
                row = torch.stack([
                    flat[b * rows_out + source]
                    if b * rows_out + source < batch * rows_out
                    else torch.zeros_like(flat[0]) for b in range(batch)])
            else:
                continue
            for kt in range(3):
                # gx[t] += W[kt] gz[t + 1 - kt]
                shifted = torch.zeros_like(row)
                lo, hi = max(0, kt - 1), min(frames, frames + kt - 1)
                shifted[:, :, lo:hi] = row[:, :, lo + 1 - kt:hi + 1 - kt]
                gx[:, :, f] += torch.einsum(
                    'oc,bot->bct', weight[:, :, kf, kt], shifted)
    if defect == 'row_block_overwritten' and channels >= 32:
        gx[:, :16] = gx[:, 16:32].clone()
    return gx


def layer_backward(x, weight, y, upstream, stride, activation, defect=None,
                   table=None):
    """(gx, gW, gb) from the upstream gradient, the output and the input"""
    x, weight, y = x.double(), weight.double(), y.double()
    upstream = upstream.double()
    channels = x.shape[1]
    if activation == 'relu':
        # torch's threshold_backward (tests/fdisc_oracle.py, layer_backward)
        gz = torch.where(y <= 0., torch.zeros_like(upstream), upstream)
    elif activation == 'sigmoid':
        gz = upstream * y * (1. - y)
    else:
        gz = upstream
    grad_weight = torch.zeros_like(weight)
    for kf in range(3):
        for kt in range(3):
            grad_weight[:, :, kf, kt] = torch.einsum(
                'boft,bcft->oc', gz,
                tap_input(x, stride, kf, kt, defect, table))
    if defect == 'gw_later_blocks_dropped' and channels > 16:
        grad_weight[:, 16:channels] = 0.
    if defect == 'gw_embedding_dropped':
        grad_weight[:, channels:] = 0.
    grad_x = input_gradient(gz, weight, x.shape[2], stride, defect)
    return grad_x.contiguous(), grad_weight.contiguous(), gz.sum((0, 2, 3))


###############################################################################
# The stack at a resolution
###############################################################################


def plan(n_fft):
    """[(stride, channels, out_channels)] of the six layers: the first
    log2(n_fft / 64) halve the frequency axis, the layer after each doubles
    the channels, 16 at first and 256 at most; the last has one"""
    halvings = int(math.log2(n_fft // 64))
    layers, channels, out_channels = [], 1, 16
    for index in range(5):
        stride = 2 if index < halvings else 1
        layers.append((stride, channels, out_channels))
        channels, out_channels = out_channels, min(stride * out_channels, 256)
    return layers + [(1, channels, 1)]


def shapes(n_fft):
    """{key: shape} of the trained parameters, in the state_dict's order"""
    out = {}
    for index, (_, channels, out_channels) in enumerate(plan(n_fft)):
        out[f'layers.{index}.1.bias'] = (out_channels,)
        out[f'layers.{index}.1.weight_g'] = (out_channels, 1, 1, 1)
        out[f'layers.{index}.1.weight_v'] = (out_channels, channels + 2, 3, 3)
    return out


def parameters(n_fft):
    """{key: fp32 tensor}, stored nowhere: weight_v in [-.5, .5), bias in
    [-.125, .125), weight_g in [.5, 1.25): positive, and away from |v|, so
    that weight norm shows"""
    return conv_oracle.hashed_parameters(
        shapes(n_fft), 100 * int(math.log2(n_fft)))


STACK_FRAMES = 4


def stack_input(n_fft):
    """The fixed (2, 1, n_fft / 2 + 1, 4) map: decibel-like, -40 +- 32 in
    multiples of 2^-6"""
    bins = n_fft // 2 + 1
    value = hashed(BATCH * bins * STACK_FRAMES, 9000 + n_fft)
    return (64. * value - 72.).float().reshape(BATCH, 1, bins, STACK_FRAMES)


def coefficients(shapes_of_outputs):
    """The fixed linear functional, fdisc_oracle.coefficients' formula at the
    shapes of the five maps and, last, the logits: in [-.5, .5) for the maps
    and in [0, 1) for the logits"""
    out = []
    for index, shape in enumerate(shapes_of_outputs):
        last = index == len(shapes_of_outputs) - 1
        mixed = (torch.arange(math.prod(shape), dtype=torch.int64) +
                 7919 * (index + 1)) * 2654435761 % 2 ** 32
        out.append((mixed.double() / 2 ** 32 - (0. if last else .5))
                   .float().reshape(tuple(shape)))
    return out


def listed(named, count=6):
    return [tuple(named[f'layers.{i}.1.{key}']
                  for key in ('weight_g', 'weight_v', 'bias'))
            for i in range(count)]


def stack(x, parameters, strides, defect=None):
    """x (B, 1, F, T); parameters: [(weight_g, weight_v, bias)] of the six
    layers -> (logits, [five maps], what the backward needs)"""
    saved, outputs = [], []
    for index, ((g, v, bias), stride) in enumerate(zip(parameters, strides)):
        activation = 'sigmoid' if index == len(strides) - 1 else 'relu'
        weight = weight_norm(g, v)
        y = layer(x, weight, bias, stride, activation, defect)
        saved.append((x.double(), weight, y, stride, activation))
        outputs.append(y)
        x = y
    return outputs[-1], outputs[:-1], saved


def stack_backward(saved, parameters, upstreams, defect=None):
    """upstreams: the gradient at each of the six outputs (the maps, then the
    logits) -> (gradient in x, [(g_g, g_v, g_b)])"""
    carried, gradients = None, []
    for (x, weight, y, stride, activation), (g, v, _), upstream in zip(
            reversed(saved), reversed(parameters), reversed(upstreams)):
        total = upstream.double() if carried is None \
            else upstream.double() + carried
        carried, grad_weight, grad_bias = layer_backward(
            x, weight, y, total, stride, activation, defect)
        gradients.append(
            weight_norm_backward(grad_weight, g, v) + (grad_bias,))
    return carried, gradients[::-1]


###############################################################################
# The inputs of the cases, the truth and the figures
###############################################################################

SEEDS = {}


def inputs(name):
    """fp32: x Gaussian (16 channels or more) or 20 N(0, 1) - 40, decibel-like
    (one channel); weight and bias from Conv2d's default init; upstream
    Gaussian"""
    channels, out_channels, bins, frames, stride, _ = CASES[name]
    index = list(CASES).index(name)
    generator = torch.Generator().manual_seed(
        SEEDS.get(name, 0) * 1000 + 50 + index)
    x = torch.randn(BATCH, channels, bins, frames, generator=generator)
    if channels == 1:
        x = 20. * x - 40.
    upstream = torch.randn(
        BATCH, out_channels, out_bins(bins, stride), frames,
        generator=generator)
    weight, bias = conv_oracle.conv_parameters(
        torch.nn.Conv2d, SEEDS.get(name, 0) * 1000 + 550 + index,
        channels + 2, out_channels, 3)
    return x, weight, bias, upstream


def reference_fp32(x, weight, bias, stride, activation, dtype=torch.float32,
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
        stride=(stride, 1), dilation=1, padding=(1, 1))
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


def integer_case(name, which):
    """The case in integers of [-4, 4] (tests/test_gpu_fdisc_strided_exact.py):
    'x' has the embedding channels' weights zero, 'table' only them nonzero
    under an integer (F, 2) table; a sigmoid case runs with activation 'none'
    -> (x, weight, bias, upstream, table, stride, activation)"""
    channels, out_channels, bins, frames, stride, activation = CASES[name]
    generator = torch.Generator().manual_seed(
        17 + list(CASES).index(name) + 100 * (which == 'table'))
    x = integers((BATCH, channels, bins, frames), generator)
    weight = integers((out_channels, channels + 2, 3, 3), generator)
    if which == 'x':
        weight[:, channels:] = 0.
        table = None
    else:
        weight[:, :channels] = 0.
        table = integers((bins, 2), generator)
    bias = integers((out_channels,), generator)
    upstream = integers(
        (BATCH, out_channels, out_bins(bins, stride), frames), generator)
    if activation == 'sigmoid':
        activation = 'none'
    return x, weight, bias, upstream, table, stride, activation

"""What the float64 oracles of the conv-layer families share
(tests/{fdisc,fdisc_strided,dconv,pconv,gconv}_oracle.py): the figure of a
comparison and the gate on it, the closed-form and the seeded inputs, weight
norm and its adjoint, the conv as a sum over taps of a padded source with its
hand-written adjoint, and the truth of a case with its fragile mask. A family
module states what is its own (cases, geometry, padding, taps, defects, stacks)
and re-exports these names for its tests.
"""
import math

import torch

QUANTITIES = ('forward', 'gx', 'gW', 'gb')

###############################################################################
# Figures, gates and inputs
###############################################################################


def figure(got, want):
    """The largest error relative to the RMS of the true quantity"""
    want = want.double()
    return ((got.double() - want).abs().max() /
            want.pow(2).mean().sqrt()).item()


def gate(recorded, quantity):
    """4 x the largest recorded figure of the quantity over the table: the
    project's margin for one more rounding order"""
    index = QUANTITIES.index(quantity)
    return 4. * max(figures_[index] for figures_ in recorded.values())


def hashed(count, salt):
    """count multiples of 2^-12 in [0, 1): a multiplicative hash of the index.
    A closed form of integers, exact in fp32, the same on every machine (no
    RNG, no libm)"""
    mixed = (torch.arange(count, dtype=torch.int64) + 7919 * (salt + 1)) \
        * 2654435761 % 2 ** 32
    return (mixed >> 20).double() / 4096.


def hashed_parameters(shapes, salt):
    """{key: fp32 tensor} of a state_dict's {key: shape}, entry i hashed with
    salt + i: weight_v in [-.5, .5), bias in [-.125, .125), weight_g in
    [.5, 1.25): positive, and away from |v|, so that weight norm shows"""
    out = {}
    for index, (key, shape) in enumerate(shapes.items()):
        value = hashed(math.prod(shape), salt + index)
        if key.endswith('weight_g'):
            value = .75 * value + .5
        elif key.endswith('bias'):
            value = (value - .5) / 4.
        else:
            value = value - .5
        out[key] = value.float().reshape(shape)
    return out


def hashed_coefficients(shapes_of_maps, salt):
    """The fixed linear functional of a stack's tests: one fp32 tensor per map
    (the last is the logits), map i hashed with salt + i, in [-.5, .5) for the
    maps and in [0, 1) for the logits, whose bias gradient would otherwise be
    a cancelling sum (tests/fdisc_oracle.py, coefficients)"""
    out = []
    for index, shape in enumerate(shapes_of_maps):
        value = hashed(math.prod(shape), salt + index)
        if index < len(shapes_of_maps) - 1:
            value = value - .5
        out.append(value.float().reshape(tuple(shape)))
    return out


def integers(shape, generator, low=-4, high=4):
    return torch.randint(
        low, high + 1, shape, generator=generator).to(torch.float32)


def conv_parameters(conv, seed, *sizes):
    """(weight, bias) of the default initialisation of `conv` (Conv1d or
    Conv2d) at `sizes`, fp32, seeded without touching the global generator"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        module = conv(*sizes)
    return module.weight.detach().clone(), module.bias.detach().clone()


###############################################################################
# The activations
###############################################################################


def activate(z, activation):
    if activation == 'relu':
        return z.clamp(min=0.)
    if activation == 'sigmoid':
        return 1. / (1. + torch.exp(-z))
    assert activation == 'none'
    return z


def leaky(z, slope, defect=None):
    if defect == 'slope_on_positive':
        return torch.where(z > 0., z * slope, z)
    return torch.where(z > 0., z, z * slope)


###############################################################################
# Weight norm (torch._weight_norm, dim 0)
###############################################################################


def _norm(v, defect=None):
    if defect == 'norm_whole_tensor':
        return v.norm().expand(v.shape[0])
    return v.flatten(1).norm(dim=1)


def weight_norm(g, v, defect=None):
    g, v = g.double(), v.double()
    shape = (-1,) + (1,) * (v.ndim - 1)
    return v * (g.reshape(-1) / _norm(v, defect)).reshape(shape)


def weight_norm_backward(grad_w, g, v, defect=None):
    """(g_g like g, g_v)"""
    grad_w, gd, v = grad_w.double(), g.double().reshape(-1), v.double()
    shape = (-1,) + (1,) * (v.ndim - 1)
    norm = _norm(v, defect)
    if defect == 'norm_whole_tensor':
        dot = (grad_w * v).flatten(1).sum(1)
        grad_g = dot / norm
        grad_v = grad_w * (gd / norm).reshape(shape) - \
            v * ((gd * dot).sum() / norm[0] ** 3)
        return grad_g.reshape(g.shape), grad_v
    dot = (grad_w * v).flatten(1).sum(1)
    grad_v = (gd / norm).reshape(shape) * (
        grad_w - v * (dot / norm ** 2).reshape(shape))
    return (dot / norm).reshape(g.shape), grad_v


def weight_norm_inputs(shape):
    generator = torch.Generator().manual_seed(shape[0] * 100 + shape[1])
    g = torch.rand(shape[0], 1, 1, 1, generator=generator) + .5
    v = torch.randn(shape, generator=generator)
    upstream = torch.randn(shape, generator=generator)
    return g, v, upstream


def weight_norm_figures(run, shape):
    """(w, g_g, g_v): the figures of `run`, (g, v, upstream) -> (w, g_g, g_v),
    against the oracle on the seeded inputs of the shape"""
    g, v, upstream = weight_norm_inputs(shape)
    w, grad_g, grad_v = run(g, v, upstream)
    assert grad_g.shape == g.shape
    want_g, want_v = weight_norm_backward(upstream, g, v)
    return (figure(w, weight_norm(g, v)), figure(grad_g, want_g),
            figure(grad_v, want_v))


def weight_norm_fp32_figures(shape):
    """The figures of torch._weight_norm with autograd in fp32 on this CPU"""
    def run(g, v, upstream):
        leaf_g, leaf_v = g.clone().requires_grad_(True), \
            v.clone().requires_grad_(True)
        w = torch._weight_norm(leaf_v, leaf_g, 0)
        w.backward(upstream)
        return w.detach(), leaf_g.grad, leaf_v.grad
    return weight_norm_figures(run, shape)


###############################################################################
# The conv: a sum over taps (kh, kw, rows, columns) of the float64 `source`,
# the input with its padding; rows and columns are the slices of the source
# that the tap reads, one element an output pixel
###############################################################################


def conv_forward(source, weight, taps):
    """z (B, O, H', W') without the bias"""
    z = None
    for kh, kw, rows, columns in taps:
        term = torch.einsum(
            'oc,bchw->bohw', weight[:, :, kh, kw], source[:, :, rows, columns])
        z = term if z is None else z + term
    return z


def conv_adjoint(source, weight, gz, taps, scatters=None, gz_of_weight=None):
    """(the gradient in the padded source, gW) of gz. The two hooks plant
    defects: a tap for which `scatters(kh, kw)` is false leaves the source's
    gradient alone, and gW contracts `gz_of_weight` in place of gz."""
    spread = torch.zeros_like(source)
    grad_weight = torch.zeros_like(weight)
    kept = gz if gz_of_weight is None else gz_of_weight
    for kh, kw, rows, columns in taps:
        if scatters is None or scatters(kh, kw):
            spread[:, :, rows, columns] += torch.einsum(
                'oc,bohw->bchw', weight[:, :, kh, kw], gz)
        grad_weight[:, :, kh, kw] = torch.einsum(
            'bohw,bchw->oc', kept, source[:, :, rows, columns])
    return spread, grad_weight


###############################################################################
# The truth of a case
###############################################################################


class Truths:
    """The cases of a family in float64, each computed once and shared: the
    inputs (the upstream gradient zero at the fragile elements), y, gx, gW, gb
    and the fragile mask. An element is fragile where its pre-activation lies
    within 64 x the largest fp32-vs-float64 error of the case around zero
    under an activation with a kink there: the two sides of the mask cannot be
    told apart in fp32, so it carries no upstream gradient.

    The family says, for a case `name`: inputs(name) -> (x, weight, bias,
    upstream) in fp32; pre_activation(name, x, weight, bias) in float64;
    kinked(name); activate(name, z); backward(name, x, weight, y, upstream)
    -> (gx, gW, gb); reference(name, x, weight, bias, dtype, upstream), the
    reference's own arithmetic -> (z, y, (gx, gW, gb) or None)."""

    def __init__(self, inputs, pre_activation, kinked, activate, backward,
                 reference):
        self.inputs, self.pre_activation = inputs, pre_activation
        self.kinked, self.activate = kinked, activate
        self.backward, self.reference = backward, reference
        self.kept = {}

    def truth(self, name):
        if name not in self.kept:
            x, weight, bias, upstream = self.inputs(name)
            z = self.pre_activation(name, x, weight, bias)
            z32, _, _ = self.reference(
                name, x, weight, bias, torch.float32, None)
            error = (z32.double() - z).abs().max()
            fragile = (z.abs() < 64. * error) if self.kinked(name) \
                else torch.zeros_like(z, dtype=torch.bool)
            upstream = torch.where(
                fragile, torch.zeros_like(upstream), upstream)
            y = self.activate(name, z)
            gx, gw, gb = self.backward(name, x, weight, y, upstream)
            self.kept[name] = {
                'x': x, 'weight': weight, 'bias': bias, 'upstream': upstream,
                'z': z, 'forward': y, 'gx': gx, 'gW': gw, 'gb': gb,
                'fragile': fragile}
        return self.kept[name]

    def figures(self, name, forward, gx, gw, gb):
        """The four figures of a result against the truth of the case"""
        want = self.truth(name)
        return tuple(figure(got, want[quantity]) for got, quantity in zip(
            (forward, gx, gw, gb), QUANTITIES))

    def fp32_figures(self, name):
        """The figures of the reference's own arithmetic in fp32 on this CPU"""
        want = self.truth(name)
        _, y, gradients = self.reference(
            name, want['x'], want['weight'], want['bias'], torch.float32,
            want['upstream'])
        return self.figures(name, y, *gradients)


###############################################################################
# A stack against its golden
###############################################################################


def golden_coefficients(kept, coefficients):
    """The functional of a golden stack: the closed form `coefficients`,
    mended where the golden says"""
    for index, where, value in zip(*(c.tolist() for c in kept['mended'])):
        coefficients[index].view(-1)[where] = value
    return coefficients


def stack_figures(golden, kept, logits, maps, grad_x, want_x, gradients):
    """[(label, quantity, figure)] of a stack's results against its golden
    `kept`: the comparison of the GPU tests. `maps` without the logits;
    `gradients` {key: tensor}."""
    out = [('logits', 'forward', figure(logits, kept['logits']))]
    wanted = kept['maps'].split(kept['map_counts'])
    for index, (got, want) in enumerate(zip(maps, wanted)):
        out.append((f'map{index}', 'forward', figure(
            got.contiguous().flatten()[::golden['map_stride']], want)))
    out.append(('gx', 'gx', figure(grad_x, want_x)))
    keys = [key for key, _ in kept['gradient_counts']]
    wanted = kept['gradients'].split(
        [count for _, count in kept['gradient_counts']])
    for key, want in zip(keys, wanted):
        step = golden['gradient_stride'] if key.endswith('weight_v') else 1
        out.append((key, 'gb' if key.endswith('bias') else 'gW',
                    figure(gradients[key].flatten()[::step], want)))
    return out

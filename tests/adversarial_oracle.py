"""The project's own statement of the adversarial losses
(promonet/train/loss.py:11-53), in torch on the CPU, written from the
formulas:

  feature matching   sum over pairs of mean |real - fake|; with omit_first
                     without each discriminator's first pair; gradient to the
                     fake maps only, -sign(real - fake) / numel, 0 where equal
  discriminator      sum_k mean (1 - real_k)^2 + sum_k mean fake_k^2, or with
                     hinge sum_k mean max(1 - real_k, 0) + sum_k mean
                     max(1 + fake_k, 0)
  generator          sum_k mean (1 - output_k)^2, or with hinge sum_k mean
                     max(1 - output_k, 0)
  max(x, 0) passes the gradient at x = 0, as torch.clamp(min=0) does.

Three things: the float64 functions with their analytic gradients (the
yardstick); `gradient_fp32`, the fp32 restatement of the backward kernel
(c = g / (float)numel in one fp32 division, at most one multiplication that
rounds, the result rounded to the input's dtype); and `chunked_mean`, the
fp32 restatement of the forward kernel's order of summation, which the gate
of the Gaussian test is held against.
"""
import torch

ABS_DIFF, SQ_ONE_MINUS, SQ, HINGE_ONE_MINUS, HINGE_ONE_PLUS = range(5)
OPS = (ABS_DIFF, SQ_ONE_MINUS, SQ, HINGE_ONE_MINUS, HINGE_ONE_PLUS)
THREADS, VEC = 256, 8       # the kernel's workgroup and elements a thread


def term(op, a, b=None):
    """op applied elementwise, in a's dtype"""
    if op == ABS_DIFF:
        return (a - b).abs()
    if op == SQ_ONE_MINUS:
        return (1. - a) * (1. - a)
    if op == SQ:
        return a * a
    if op == HINGE_ONE_MINUS:
        return torch.clamp(1. - a, min=0.)
    assert op == HINGE_ONE_PLUS
    return torch.clamp(1. + a, min=0.)


def derivative(op, a, b=None):
    """d term / d a (d term / d b for ABS_DIFF), in a's dtype"""
    if op == ABS_DIFF:
        return -torch.sign(a - b)
    if op == SQ_ONE_MINUS:
        return 2. * (a - 1.)
    if op == SQ:
        return 2. * a
    if op == HINGE_ONE_MINUS:
        return -(1. - a >= 0.).to(a.dtype)
    assert op == HINGE_ONE_PLUS
    return (1. + a >= 0.).to(a.dtype)


###############################################################################
# float64: the yardstick
###############################################################################


def multi_mean(ops, a, b=None):
    """(means (K) float64, total float64): the sum of the terms over numel,
    the means added in list order"""
    means = []
    for index, (op, tensor) in enumerate(zip(ops, a)):
        other = None if op != ABS_DIFF else b[index].double()
        means.append(term(op, tensor.double(), other).sum() / tensor.numel())
    total = torch.zeros((), dtype=torch.float64)
    for mean in means:
        total = total + mean
    return torch.stack(means), total


def logit_ops(count, hinge, both):
    first = HINGE_ONE_MINUS if hinge else SQ_ONE_MINUS
    second = HINGE_ONE_PLUS if hinge else SQ
    return (first,) * count + (second,) * count * both


def flatten(feature_maps, omit_first):
    return [m for maps in feature_maps for m in maps[int(omit_first):]]


def feature_matching(real_feature_maps, fake_feature_maps, omit_first=False):
    real = flatten(real_feature_maps, omit_first)
    fake = flatten(fake_feature_maps, omit_first)
    return multi_mean((ABS_DIFF,) * len(real), real, fake)[1]


def discriminator(real_outputs, fake_outputs, hinge=False):
    count = len(real_outputs)
    means, total = multi_mean(
        logit_ops(count, hinge, True),
        list(real_outputs) + list(fake_outputs))
    return total, list(means[:count]), list(means[count:])


def generator(discriminator_outputs, hinge=False):
    means, total = multi_mean(
        logit_ops(len(discriminator_outputs), hinge, False),
        discriminator_outputs)
    return total, list(means)


def feature_matching_gradient(real_feature_maps, fake_feature_maps,
                              omit_first=False):
    """d loss / d fake, nested as the input; zeros for an omitted map"""
    return [[
        torch.zeros_like(fake, dtype=torch.float64)
        if omit_first and index == 0 else
        derivative(ABS_DIFF, real.double(), fake.double()) / fake.numel()
        for index, (real, fake) in enumerate(zip(reals, fakes))]
        for reals, fakes in zip(real_feature_maps, fake_feature_maps)]


def logit_gradient(ops, tensors):
    return [derivative(op, t.double()) / t.numel()
            for op, t in zip(ops, tensors)]


def discriminator_gradient(real_outputs, fake_outputs, hinge=False):
    count = len(real_outputs)
    gradients = logit_gradient(
        logit_ops(count, hinge, True),
        list(real_outputs) + list(fake_outputs))
    return gradients[:count], gradients[count:]


def generator_gradient(discriminator_outputs, hinge=False):
    return logit_gradient(
        logit_ops(len(discriminator_outputs), hinge, False),
        discriminator_outputs)


###############################################################################
# fp32: the kernels' own arithmetic
###############################################################################


def gradient_fp32(op, a, b=None, g=1.):
    """The backward kernel: c = g / (float)numel, then c times the derivative
    with one rounding at most, rounded once more to a's dtype"""
    c = torch.tensor(g, dtype=torch.float32) / \
        torch.tensor(a.numel(), dtype=torch.float32)
    x = a.float()
    if op == ABS_DIFF:
        d = x - b.float()
        zero = torch.zeros_like(x)
        out = torch.where(d > 0, -c, torch.where(d < 0, c, zero))
    elif op == SQ_ONE_MINUS:
        out = (2. * (x - 1.)) * c
    elif op == SQ:
        out = (2. * x) * c
    elif op == HINGE_ONE_MINUS:
        out = torch.where(1. - x >= 0, -c, torch.zeros_like(x))
    else:
        out = torch.where(1. + x >= 0, c, torch.zeros_like(x))
    return out.to(a.dtype)


def chunked_mean(op, a, b, chunk):
    """The forward kernel's order, in fp32: a chunk is `chunk` elements of
    the flat tensor; thread t of 256 adds the terms of elements (256 j + t) 8
    .. + 7, j ascending, one by one; a wave sums its 64 threads as a
    butterfly (xor 32, 16, .. 1), the four waves add in order. The partials
    are summed in ascending order in double and divided by numel in double;
    the result is that double (the kernel rounds it once, `.float()`)."""
    rounds = chunk // (THREADS * VEC)
    assert rounds * THREADS * VEC == chunk
    terms = term(op, a.float().flatten(),
                 None if b is None else b.float().flatten())
    chunks = -(-terms.numel() // chunk)
    padded = torch.zeros(chunks * chunk, dtype=torch.float32)
    padded[:terms.numel()] = terms
    # (chunks, 256 threads, the thread's rounds x 8 terms in its order)
    per_thread = padded.view(chunks, rounds, THREADS, VEC).permute(
        0, 2, 1, 3).reshape(chunks, THREADS, rounds * VEC)
    sums = torch.zeros(chunks, THREADS, dtype=torch.float32)
    for index in range(rounds * VEC):
        sums = sums + per_thread[:, :, index]
    waves = sums.view(chunks, THREADS // 64, 64)
    lanes = torch.arange(64)
    for mask in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, :, lanes ^ mask]
    partials = waves[:, 0, 0]
    for wave in range(1, THREADS // 64):
        partials = partials + waves[:, wave, 0]
    total = torch.zeros((), dtype=torch.float64)
    for partial in partials.double():
        total = total + partial
    return total / a.numel()


###############################################################################
# Inputs
###############################################################################


def grid(shape, step, seed, dtype=torch.float32):
    """Multiples of `step` in [-2, 2], exact in fp32, f16 and bf16"""
    generator = torch.Generator().manual_seed(seed)
    steps = round(2 / step)
    return (torch.randint(
        -steps, steps + 1, shape, generator=generator) * step).to(dtype)


def gaussian(shape, seed, dtype=torch.float32):
    generator = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=generator).to(dtype)

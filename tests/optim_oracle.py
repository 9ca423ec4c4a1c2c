"""The project's own statement of the optimizer step (pm_optim.h) in torch on
the CPU, written from the contract:

  statistics   max, min, mean = sum / numel, norm = sqrt(sum of squares) and
               the count of NaN / +-inf elements over a list of gradients. A
               non-finite element adds nothing to the other four. The sums:
               every tensor is cut into chunks; thread t of 256 adds elements
               (256 j + t) 8 .. + 7, j ascending, one by one in fp32; a wave
               sums its 64 threads as a butterfly (xor 32 .. 1), the four
               waves add in order; the chunks of the whole list are added in
               ascending order in double and rounded once.
  control      found_inf, inv_scale = (float)(1.0 / (double)scale), the clip
               coefficient in the reference's order, and unless found_inf
               step += 1, b1pow *= beta1, b2pow *= beta2 (Python floats are the
               device's doubles).
  update       every fp32 product and sum a separate torch op:
                 g = (grad inv_scale) coef
                 p = p (float)(1 - lr wd)
                 m = m + (float)(1 - beta1) (g - m)
                 v = v (float)beta2 + (float)(1 - beta2) (g g)
                 d = sqrt(v) / (float)sqrt(1 - b2pow) + (float)eps
                 p = p + (float)(-lr / (1 - b1pow)) (m / d)
  scaler       torch.amp.GradScaler.update()'s rule.

The fp32 square root is taken in float64 and rounded once: that IS the
correctly rounded fp32 root (53 >= 2 x 24 + 2 bits, so the second rounding
cannot change it), on every host. torch.sqrt on fp32 CPU tensors is not
relied on: on the MI355X host's CPU it was 1 ulp off in about 20 of 65 000
elements, where the device's root was the correctly rounded one.
tests/test_cpu_optim.py checks root and quotient against their exact
definitions.
"""
import math

import torch

THREADS, VEC = 256, 8       # the kernel's workgroup and elements a thread


def f32(value):
    """A double rounded once to fp32, as a 0-d tensor"""
    return torch.tensor(value, dtype=torch.float64).float()


###############################################################################
# Statistics
###############################################################################


def chunk_partials(values, chunk):
    """The fp32 partial sums of a flat fp32 tensor, one a chunk, in the
    kernel's order"""
    rounds = chunk // (THREADS * VEC)
    assert rounds * THREADS * VEC == chunk
    chunks = -(-values.numel() // chunk)
    padded = torch.zeros(chunks * chunk, dtype=torch.float32)
    padded[:values.numel()] = values
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
    return partials


def ordered_sum(partials):
    """fp32 partials added in ascending order in double"""
    total = 0.
    for partial in partials.double().tolist():
        total += partial
    return total


def grad_stats(gradients, chunk):
    """{'max', 'min', 'mean', 'norm', 'norm_sq', 'nonfinite'} as 0-d fp32
    tensors; the gradients are read as stored and converted to fp32"""
    values = [g.detach().float().flatten() for g in gradients]
    finite = [torch.isfinite(v) for v in values]
    kept = torch.cat([v[f] for v, f in zip(values, finite)])
    zeroed = [torch.where(f, v, torch.zeros_like(v))
              for v, f in zip(values, finite)]
    sums = ordered_sum(torch.cat([chunk_partials(z, chunk) for z in zeroed]))
    squares = ordered_sum(
        torch.cat([chunk_partials(z * z, chunk) for z in zeroed]))
    numel = sum(v.numel() for v in values)
    infinity = torch.tensor(math.inf)
    return {
        'max': kept.max() if kept.numel() else -infinity,
        'min': kept.min() if kept.numel() else infinity,
        'mean': f32(sums / numel),
        'norm': f32(math.sqrt(squares)),
        'norm_sq': f32(squares),
        'nonfinite': f32(float(numel - kept.numel()))}


def grad_stats_float64(gradients):
    """The yardstick: (mean, norm, norm_sq, mean of magnitudes) in float64"""
    values = torch.cat([g.detach().double().flatten() for g in gradients])
    values = values[torch.isfinite(values)]
    total = sum(g.numel() for g in gradients)
    return (values.sum() / total, values.square().sum().sqrt(),
            values.square().sum(), values.abs().sum() / total)


###############################################################################
# The control block and the optimizer's state
###############################################################################


class State:
    """{step, beta1^step, beta2^step}: the powers multiplied up step by step"""

    def __init__(self, beta1, beta2, step=0):
        self.beta1, self.beta2 = beta1, beta2
        self.step, self.b1pow, self.b2pow = 0, 1., 1.
        for _ in range(step):
            self.advance()

    def advance(self):
        self.step += 1
        self.b1pow *= self.beta1
        self.b2pow *= self.beta2


def control(stats, grad_scale=None, found_inf=0., clip=None):
    """(found_inf, inv_scale, coef): a bool and two 0-d fp32 tensors"""
    found = bool(stats['nonfinite'] != 0) or found_inf != 0
    inv_scale = f32(1.) if grad_scale is None else f32(
        1. / float(f32(grad_scale)))
    coef = f32(1.)
    magnitude = torch.maximum(stats['max'], stats['min'].abs())
    if clip is not None and float(magnitude) > clip:
        total = magnitude * inv_scale
        coef = torch.minimum(f32(clip) / (total + f32(1e-6)), f32(1.))
    return found, inv_scale, coef


###############################################################################
# The update
###############################################################################


def constants(state, lr, eps, weight_decay):
    """The seven fp32 constants, formed in double from the state after its
    advance"""
    return {
        'decay': f32(1. - lr * weight_decay),
        'one_minus_beta1': f32(1. - state.beta1),
        'beta2': f32(state.beta2),
        'one_minus_beta2': f32(1. - state.beta2),
        'bias2': f32(math.sqrt(1. - state.b2pow)),
        'eps': f32(eps),
        'step': f32(-lr / (1. - state.b1pow))}


def sqrt(x):
    """The correctly rounded fp32 square root (see the top of the file)"""
    return torch.sqrt(x.double()).float()


def update(c, inv_scale, coef, gradient, p, m, v):
    """(p, m, v) after the update of fp32 tensors; `gradient` as stored"""
    g = (gradient.float() * inv_scale) * coef
    p = p * c['decay']
    m = m + c['one_minus_beta1'] * (g - m)
    v = v * c['beta2'] + c['one_minus_beta2'] * (g * g)
    d = sqrt(v) / c['bias2'] + c['eps']
    p = p + c['step'] * (m / d)
    return p, m, v


class AdamW:
    """The two passes over lists of CPU tensors: `params` fp32, replaced by
    every step, with their moments; `last` is the last step's statistics and
    control block"""

    def __init__(self, params, chunk, lr=2e-4, betas=(.8, .99), eps=1e-9,
                 weight_decay=1e-2, clip=None):
        self.params = [p.detach().clone() for p in params]
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.state = State(*betas)
        self.chunk, self.lr, self.eps = chunk, lr, eps
        self.weight_decay, self.clip = weight_decay, clip
        self.last = None

    def step(self, gradients, grad_scale=None, found_inf=0.):
        """`gradients` as stored (fp32, f16 or bf16); a None leaves its
        parameter out. Returns found_inf."""
        present = [k for k, g in enumerate(gradients) if g is not None]
        stats = grad_stats([gradients[k] for k in present], self.chunk)
        found, inv_scale, coef = control(
            stats, grad_scale, found_inf, self.clip)
        self.last = dict(stats, found_inf=f32(float(found)),
                         inv_scale=inv_scale, coef=coef)
        if found:
            return True
        self.state.advance()
        c = constants(self.state, self.lr, self.eps, self.weight_decay)
        for k in present:
            self.params[k], self.exp_avg[k], self.exp_avg_sq[k] = update(
                c, inv_scale, coef, gradients[k], self.params[k],
                self.exp_avg[k], self.exp_avg_sq[k])
        return False


###############################################################################
# The scaler
###############################################################################


def scaler_update(scale, tracker, found_inf, growth=2., backoff=.5,
                  interval=2000):
    """(scale, tracker) after GradScaler.update(): scale a Python float that
    holds an fp32 value, the products in double and rounded once"""
    if found_inf:
        return float(f32(scale * backoff)), 0
    tracker += 1
    if tracker == interval:
        grown = float(f32(scale * growth))
        return (scale if math.isinf(grown) else grown), 0
    return scale, tracker


###############################################################################
# Inputs
###############################################################################


def gaussian(shape, seed, scale=1.):
    generator = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=generator) * scale


def decades(shape, seed):
    """Gaussian times 10^U{-6..0}, element by element"""
    generator = torch.Generator().manual_seed(seed)
    exponent = torch.randint(-6, 1, shape, generator=generator)
    return torch.randn(shape, generator=generator) * 10. ** exponent

"""CPU oracle of the loudness-editing utilities (promonet/preprocess/
loudness.py:114-193), restated in our own words, and a CPU model of the
device limiter's three phases (promonet_amd/csrc/pm_limit.h).

TEST INFRASTRUCTURE ONLY; never imported by the product.

`limit_literal` is the reference's loop (:114-141) on torch fp32 scalars, one
sample a step; `limit_rows` is the same recurrence in numpy fp32 with every
rounding written out, vectorised over rows; `chunked` is the kernel's
algorithm. The tests hold all three equal bit for bit.
"""
import functools

import numpy as np
import torch

DEFAULTS = dict(delay=40, attack_coef=.9, release_coef=.9995, threshold=.99)
CLASSES = ('quiet', 'bursts', 'saturated', 'spike', 'edges', 'settle')
REST = np.float32(0.99999976)       # 1 - 4 ulp: the gain's other fixed point


def limit_literal(audio, delay=40, attack_coef=.9, release_coef=.9995,
                  threshold=.99):
    """loudness.py:114-141 for audio (1, T) fp32: (output (1, T), gain
    (T + delay - 1)). The operand types are the reference's: samples and the
    envelope are 0-d fp32 tensors, the coefficients Python floats, the gain a
    Python float until the first limiting event makes it a tensor. The
    reference's ring buffer of `delay` samples (:120-128, :139) hands back the
    sample of delay - 1 steps ago, zero before there is one; here that is an
    index. Its first delay - 1 outputs are cut off (:141)."""
    lag = delay - 1
    padded = torch.cat([audio[0], torch.zeros(lag)])        # :117
    output = torch.zeros(len(padded))
    gains = torch.zeros(len(padded))
    envelope, gain = 0, 1.                                  # :119, :122
    for step, sample in enumerate(padded):
        envelope = max(abs(sample), envelope * release_coef)            # :131
        target = threshold / envelope if envelope > threshold else 1.   # :134
        gain = gain * attack_coef + target * (1 - attack_coef)          # :135-136
        gains[step] = gain
        if step >= lag:
            output[step] = padded[step - lag] * gain                    # :139
    return output[None, lag:], gains


def coefficients(delay=40, attack_coef=.9, release_coef=.9995, threshold=.99):
    """(delay, a, b, r, th): the fp32 roundings the loop works with; b is
    1 - attack_coef taken in double, then rounded"""
    return (int(delay), np.float32(attack_coef), np.float32(1 - attack_coef),
            np.float32(release_coef), np.float32(threshold))


def limit_rows(audio, **parameters):
    """The recurrence in numpy fp32, one rounding per operation, for audio
    (B, T): (output (B, T), gain (B, T + delay - 1))"""
    delay, a, b, r, th = coefficients(**parameters)
    x = np.asarray(audio, dtype=np.float32)
    rows, samples = x.shape
    lag = delay - 1
    padded = np.concatenate([x, np.zeros((rows, lag), np.float32)], 1)
    gains = np.zeros((rows, samples + lag), np.float32)
    e = np.zeros(rows, np.float32)
    g = np.ones(rows, np.float32)
    one = np.float32(1)
    with np.errstate(divide='ignore'):
        for n in range(samples + lag):
            e = np.maximum(np.abs(padded[:, n]), e * r)
            # scalar / tensor is a reciprocal, then a product
            t = np.where(e > th, (one / e) * th, one).astype(np.float32)
            g = g * a + t * b
            gains[:, n] = g
    output = padded[:, :samples] * gains[:, lag:]
    return torch.from_numpy(output), torch.from_numpy(gains)


def chunked(audio, L, **parameters):
    """The device algorithm on the CPU for audio (1, T), chunks of L steps:
    (output, gain, serial steps). Phase 1: every chunk's envelope from e = 0.
    Phase 2: the carries in order, kept only above th, laid over the chunks
    while they dominate; then g, walked only through chunks that limit or that
    it enters away from a fixed point. Phase 3: the output."""
    delay, a, b, r, th = coefficients(**parameters)
    x = np.asarray(audio, dtype=np.float32)[0]
    lag = delay - 1
    steps = len(x) + lag
    padded = np.concatenate([x, np.zeros(lag, np.float32)])
    starts = range(0, steps, L)
    zero, one = np.float32(0), np.float32(1)
    # 1
    local = np.zeros(steps, np.float32)
    for start in starts:
        e = zero
        for n in range(start, min(start + L, steps)):
            e = max(np.abs(padded[n]), e * r)
            local[n] = e
    # 2: carries
    serial = 0
    e, carry = local.copy(), zero
    for start in starts:
        stop = min(start + L, steps)
        leave = local[stop - 1]
        if carry > th:
            alive = True
            for n in range(start, stop):
                carry = carry * r
                serial += 1
                if not (carry > local[n] and carry > th):
                    alive = False
                    break
                e[n] = carry
            if alive:
                leave = carry
        carry = leave if leave > th else zero
    # 2: the gain
    with np.errstate(divide='ignore'):
        tb = np.where(e > th, ((one / e) * th) * b, b).astype(np.float32)
    gains = np.zeros(steps, np.float32)
    g = one
    for start in starts:
        stop = min(start + L, steps)
        if (e[start:stop] > th).any() or g * a + b != g:
            for n in range(start, stop):
                g = g * a + tb[n]
                gains[n] = g
                serial += 1
        else:
            gains[start:stop] = g
    # 3
    output = padded[:len(x)] * gains[lag:]
    return torch.from_numpy(output)[None], torch.from_numpy(gains), serial


def shift64(audio, value):
    """loudness.py:179-193 in float64 and closed form: gain = 2^(value / 10)
    per frame, interpolated to the samples as torch's linear mode with
    align_corners=False does (src = max(0, (n + .5) F / N - .5)). audio (B, N);
    value a scalar or (1, F) / (B, F). Returns float64."""
    audio = audio.to(torch.float64)
    if not isinstance(value, torch.Tensor) or value.numel() == 1:
        return audio * 2. ** (float(value) / 10)
    gain = 2. ** (value.to(torch.float64) / 10)
    frames, samples = gain.shape[-1], audio.shape[-1]
    n = torch.arange(samples, dtype=torch.float64)
    src = ((n + .5) * frames / samples - .5).clamp(min=0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp(max=frames - 1)
    w = src - i0
    return audio * ((1 - w) * gain[..., i0] + w * gain[..., i1])


def relative_units(got, want):
    """The largest relative error in units of 2^-24 (want: float64)"""
    error = (got.to(torch.float64) - want).abs()
    scale = want.abs().clamp(min=1e-30)
    return (error / scale).max().item() * 2. ** 24


def shift_inputs(frames, samples, seed=0, rows=1):
    """Audio uniform in +-1 (never exactly 0) and a contour of +-12 dB"""
    gen = torch.Generator().manual_seed(7000 + 31 * frames + samples + seed)
    audio = torch.rand(rows, samples, generator=gen) * 2 - 1
    audio = torch.where(audio == 0, torch.ones_like(audio), audio)
    value = torch.rand(rows, frames, generator=gen) * 24 - 12
    return audio, value


@functools.lru_cache(maxsize=None)
def inputs(chunk, tile, delay=40):
    """The six seeded input classes of the limiter, name -> (1, T) fp32, for a
    kernel of `chunk` steps a lane and `tile` steps a workgroup pass"""
    T = 2 * tile + 256
    gen = torch.Generator().manual_seed(20240607)

    def normal(sigma, length=T):
        return torch.randn(length, generator=gen) * sigma

    out = {}
    out['quiet'] = torch.rand(T, generator=gen) * 1.96 - .98
    bursts = normal(.25)
    bursts[300:320] *= 8
    bursts[tile + 37] = 3.
    bursts[tile + 400:tile + 800] *= .01
    bursts[2 * tile - 10:2 * tile + 10] *= 8
    out['bursts'] = bursts
    sign = torch.where(torch.rand(T, generator=gen) < .5, -1., 1.)
    out['saturated'] = (1 + 3 * torch.rand(T, generator=gen)) * sign
    spike = torch.zeros(6011)
    spike[10] = 8.
    out['spike'] = spike
    edges = normal(.1)
    for index in (0, chunk - 1, chunk, tile - 1, tile, T - 1, T - 20,
                  T - delay - 1):
        edges[index] = 1.5
    out['edges'] = edges
    settle = normal(.2)
    settle[100] = 1.
    assert (settle.abs() > .99).sum() == 1
    out['settle'] = settle
    assert tuple(out) == CLASSES
    return {name: value[None].contiguous() for name, value in out.items()}


@functools.lru_cache(maxsize=None)
def literal(name, length, chunk, tile, **parameters):
    """`limit_literal` of a class cut to `length` samples (None: all of it),
    computed once; treat the result as read-only"""
    audio = inputs(chunk, tile)[name]
    audio = audio if length is None else audio[:, :length]
    return limit_literal(audio, **parameters)

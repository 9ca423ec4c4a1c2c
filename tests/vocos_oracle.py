"""Vocos in plain CPU fp32 torch: the restatement the GPU tests compare with.

Line numbers refer to the reference's promonet/model/vocos.py. Every step is
spelled out with torch primitives (conv1d, layer_norm, linear, erf GELU,
irfft, an explicit overlap-add), so it does not depend on the reference
package. scripts/make_golden_vocos.py pins it against the reference itself
(tests/golden/vocos.pt).
"""
import math

import torch
import torch.nn.functional as F

CHANNELS = 512
POINTWISE = 1536
N_FFT = 1024
HOP = 256
PAD = (N_FFT - HOP) // 2                                   # vocos.py:186


def random_state_vocos(seed=0, num_features=80, global_channels=256,
                       layers=8, channels=CHANNELS, hidden=POINTWISE,
                       magnitude_shift=0.):
    """Vocos state dict (keys without the `model.` prefix) with the
    reference's init scheme from a seeded torch.Generator: conv_pre / cond /
    head.out as torch's default Conv1d / Linear init (U(+-1/sqrt(fan_in))),
    embed / dwconv / pwconv1 / pwconv2 truncated normal std 0.02 with zero
    bias (vocos.py:86-90), LayerNorms (1, 0), gamma 1 / layers, periodic
    Hann window. `magnitude_shift` is added to the head's log-magnitude bias
    (rows 0..512 of head.out.bias) to scale the output."""
    gen = torch.Generator().manual_seed(seed)

    def uniform(shape, fan_in):
        bound = 1. / math.sqrt(fan_in)
        return (torch.rand(shape, generator=gen) * 2 - 1) * bound

    def trunc(shape):
        return torch.nn.init.trunc_normal_(
            torch.empty(shape), std=0.02, generator=gen)

    state = {}
    state['conv_pre.weight'] = uniform((channels, num_features, 7),
                                       num_features * 7)
    state['conv_pre.bias'] = uniform((channels,), num_features * 7)
    state['backbone.embed.weight'] = trunc((channels, channels, 7))
    state['backbone.embed.bias'] = torch.zeros(channels)
    state['backbone.norm.weight'] = torch.ones(channels)
    state['backbone.norm.bias'] = torch.zeros(channels)
    for i in range(layers):
        p = f'backbone.convnext.{i}.'
        state[p + 'dwconv.weight'] = trunc((channels, 1, 7))
        state[p + 'dwconv.bias'] = torch.zeros(channels)
        state[p + 'norm.weight'] = torch.ones(channels)
        state[p + 'norm.bias'] = torch.zeros(channels)
        state[p + 'pwconv1.weight'] = trunc((hidden, channels))
        state[p + 'pwconv1.bias'] = torch.zeros(hidden)
        state[p + 'pwconv2.weight'] = trunc((channels, hidden))
        state[p + 'pwconv2.bias'] = torch.zeros(channels)
        state[p + 'gamma'] = torch.full((channels,), 1. / layers)
    state['backbone.final_layer_norm.weight'] = torch.ones(channels)
    state['backbone.final_layer_norm.bias'] = torch.zeros(channels)
    state['head.out.weight'] = uniform((N_FFT + 2, channels), channels)
    bias = uniform((N_FFT + 2,), channels)
    bias[:N_FFT // 2 + 1] += magnitude_shift
    state['head.out.bias'] = bias
    state['head.istft.window'] = torch.hann_window(N_FFT)
    state['cond.weight'] = uniform((channels, global_channels, 1),
                                   global_channels)
    state['cond.bias'] = uniform((channels,), global_channels)
    return state


def layers_of(state):
    return len({k.split('.')[2] for k in state
                if k.startswith('backbone.convnext.')})


def convnext_block(x, state, prefix):
    """vocos.py:135-146: x (B, C, T)"""
    residual = x
    x = F.conv1d(x, state[prefix + 'dwconv.weight'],
                 state[prefix + 'dwconv.bias'], padding=3, groups=x.shape[1])
    x = x.transpose(1, 2)
    x = F.layer_norm(x, (x.shape[-1],), state[prefix + 'norm.weight'],
                     state[prefix + 'norm.bias'], 1e-6)
    x = F.linear(x, state[prefix + 'pwconv1.weight'],
                 state[prefix + 'pwconv1.bias'])
    x = F.gelu(x)                                   # erf form
    x = F.linear(x, state[prefix + 'pwconv2.weight'],
                 state[prefix + 'pwconv2.bias'])
    x = state[prefix + 'gamma'] * x
    return residual + x.transpose(1, 2)


def istft(spec, window):
    """vocos.py:188-206: complex (B, 513, T) -> (B, 256 T)"""
    frames = spec.shape[-1]
    ifft = torch.fft.irfft(spec, N_FFT, dim=1, norm='backward')
    ifft = ifft * window[None, :, None]
    length = (frames - 1) * HOP + N_FFT
    y = torch.zeros(spec.shape[0], length)
    envelope = torch.zeros(length)
    square = window.square()
    for t in range(frames):                         # fold: frame order
        y[:, t * HOP:t * HOP + N_FFT] += ifft[:, :, t]
        envelope[t * HOP:t * HOP + N_FFT] += square
    return y[:, PAD:-PAD] / envelope[PAD:-PAD]


def head(x, state):
    """vocos.py:163-172: x (B, C, T) -> (B, 1, 256 T)"""
    x = F.linear(x.transpose(1, 2), state['head.out.weight'],
                 state['head.out.bias']).transpose(1, 2)
    mag, p = x.chunk(2, dim=1)
    mag = torch.clip(torch.exp(mag), max=1e2)
    spec = mag * (torch.cos(p) + 1j * torch.sin(p))
    return istft(spec, state['head.istft.window']).unsqueeze(1)


def vocos(x, g, state):
    """Vocos.forward(x, g) (vocos.py:41-54): x (B, F, T), g (B, G, 1)."""
    x = F.conv1d(x, state['conv_pre.weight'], state['conv_pre.bias'],
                 padding=3)
    if g is not None:
        x = x + F.conv1d(g, state['cond.weight'], state['cond.bias'])
    x = F.conv1d(x, state['backbone.embed.weight'],
                 state['backbone.embed.bias'], padding=3)
    x = F.layer_norm(x.transpose(1, 2), (x.shape[1],),
                     state['backbone.norm.weight'],
                     state['backbone.norm.bias'], 1e-6).transpose(1, 2)
    for i in range(layers_of(state)):
        x = convnext_block(x, state, f'backbone.convnext.{i}.')
    x = F.layer_norm(x.transpose(1, 2), (x.shape[1],),
                     state['backbone.final_layer_norm.weight'],
                     state['backbone.final_layer_norm.bias'],
                     1e-6).transpose(1, 2)
    return head(x, state)


def global_features(speakers, table):
    """MelGenerator.prepare_global_features under the baseline config (no
    augmentation ratios, generator.py:49-70): (B, 256, 1)."""
    return table[speakers].unsqueeze(-1)

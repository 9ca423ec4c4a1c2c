"""Vocos vocoder running on the MI355X HIP engine.

Drop-in for `promonet.model.Vocos` (promonet/model/vocos.py:12-54, selected
by config/baselines/vocos.py): same constructor arguments, same
`forward(x, g=None)`, the same `state_dict()` keys, shapes and default
initialisation, so a reference checkpoint loads unchanged. The forward pass
is one engine call (`pm_vocos_forward`): input convs, the fused ConvNeXt
blocks, the spectral head and the inverse STFT; there is no PyTorch compute
path. Not in the reference: `forward(..., lengths=)` runs a ragged batch of
zero-padded utterances (`pm_vocos_forward_ragged`), each equal to its
stand-alone synthesis bit for bit.
"""
import torch

import promonet_amd
from promonet_amd import _lib
from .engine import EngineModule, device_lengths, global_features

# COMPUTE_DTYPE values Vocos honours; 'checkpoint' is the mode that holds 1e-4
# at a trained checkpoint's output scale (config.py)
VOCOS_DTYPES = {'checkpoint': 'fp32', 'fp32': 'fp32', 'f32': 'fp32',
                'f16': 'f16', 'fp16': 'f16', 'bf16': 'bf16'}


def resolve_dtype(name):
    if name not in VOCOS_DTYPES:
        raise ValueError(
            f'COMPUTE_DTYPE {name!r} is not a Vocos mode: one of '
            f'{sorted(VOCOS_DTYPES)}')
    return VOCOS_DTYPES[name]


def check_lengths(lengths, batch, frames, device=None):
    """`lengths` of a ragged (batch, ..., frames) input as an int32 tensor, on
    `device` if one is given. Values that arrive on the host (a list or a CPU
    tensor) must lie in [1, frames]; a device tensor is trusted: reading it
    back would stall the stream."""
    given = torch.as_tensor(lengths)
    if given.dtype.is_floating_point or given.dtype == torch.bool:
        raise ValueError('lengths must be integers')
    lengths = device_lengths(
        given, batch, given.device if device is None else device)
    if not given.is_cuda and (
            int(given.min()) < 1 or int(given.max()) > frames):
        raise ValueError(
            f'lengths must be in [1, {frames}] (the frames of the input)')
    return lengths


class ConvNeXtBlock(torch.nn.Module):
    """Parameters of vocos.py:113-133 (forward is fused into the engine)."""

    def __init__(self, dim, layer_scale_init_value):
        super().__init__()
        self.dwconv = torch.nn.Conv1d(dim, dim, 7, padding=3, groups=dim)
        self.norm = torch.nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = torch.nn.Linear(
            dim, promonet_amd.VOCOS_POINTWISE_CHANNELS)
        self.act = torch.nn.GELU()
        self.pwconv2 = torch.nn.Linear(
            promonet_amd.VOCOS_POINTWISE_CHANNELS, dim)
        self.gamma = torch.nn.Parameter(
            layer_scale_init_value * torch.ones(dim))


class VocosBackbone(torch.nn.Module):
    """Parameters of vocos.py:62-98, with its truncated-normal init."""

    def __init__(self, input_channels, dim, num_layers):
        super().__init__()
        self.input_channels = input_channels
        self.embed = torch.nn.Conv1d(input_channels, dim, 7, padding=3)
        self.norm = torch.nn.LayerNorm(dim, eps=1e-6)
        self.convnext = torch.nn.ModuleList([
            ConvNeXtBlock(dim, 1 / num_layers) for _ in range(num_layers)])
        self.final_layer_norm = torch.nn.LayerNorm(dim, eps=1e-6)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, (torch.nn.Conv1d, torch.nn.Linear)):
            torch.nn.init.trunc_normal_(m.weight, std=0.02)
            torch.nn.init.constant_(m.bias, 0)


class ISTFT(torch.nn.Module):
    """vocos.py:175-183: only the periodic Hann `window` buffer."""

    def __init__(self, n_fft, hop_length, win_length):
        super().__init__()
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.win_length = win_length
        self.register_buffer('window', torch.hann_window(win_length))


class ISTFTHead(torch.nn.Module):
    """vocos.py:154-161"""

    def __init__(self, dim, n_fft, hop_length):
        super().__init__()
        self.out = torch.nn.Linear(dim, n_fft + 2)
        self.istft = ISTFT(n_fft, hop_length, n_fft)


class Vocos(EngineModule):

    ABI = 'vocos'

    def __init__(self, initial_channel, gin_channels):
        super().__init__()
        self.initial_channel = initial_channel
        self.gin_channels = gin_channels
        self.compute_dtype = promonet_amd.COMPUTE_DTYPE
        self.conv_pre = torch.nn.Conv1d(
            initial_channel, promonet_amd.VOCOS_CHANNELS, 7, 1, padding='same')
        self.backbone = VocosBackbone(
            promonet_amd.VOCOS_CHANNELS, promonet_amd.VOCOS_CHANNELS,
            promonet_amd.VOCOS_LAYERS)
        self.head = ISTFTHead(
            promonet_amd.VOCOS_CHANNELS, promonet_amd.NUM_FFT,
            promonet_amd.HOPSIZE)
        self.cond = torch.nn.Conv1d(
            gin_channels, promonet_amd.VOCOS_CHANNELS, 1)
        for parameter in self.parameters():
            parameter.requires_grad_(False)

    ###########################################################################
    # Engine (handle lifetime, workspace and stream guard: engine.py)
    ###########################################################################

    def _key(self):
        return resolve_dtype(self.compute_dtype)

    def _create(self, lib, handle):
        return lib.pm_vocos_create(
            self.initial_channel, self.gin_channels,
            promonet_amd.VOCOS_CHANNELS,
            self.backbone.convnext[0].pwconv1.out_features
            if len(self.backbone.convnext) else
            promonet_amd.VOCOS_POINTWISE_CHANNELS,
            len(self.backbone.convnext), self.head.istft.n_fft,
            self.head.istft.hop_length, _lib.DTYPES[self._key()], handle)

    ###########################################################################
    # Forward (vocos.py:41-54)
    ###########################################################################

    def forward(self, x, g=None, lengths=None):
        """x (B, F, T) features, g (B|1, G, 1) global features or None ->
        audio (B, 1, 256 T). `lengths` (B,) frames (not in the reference):
        ragged batch of zero-padded utterances, each synthesised as if alone;
        the audio past 256 * lengths[b] is zero. Values on the host (a list
        or a CPU tensor) are range-checked; a device tensor is trusted and
        never read back."""
        _lib.require_gpu(x)
        engine = self.engine()
        x = x.to(torch.float32).contiguous()
        batch, channels, frames = x.shape
        if channels != self.initial_channel:
            raise ValueError(
                f'expected {self.initial_channel} feature channels, got '
                f'{channels}')
        pointer, gbatch = None, 1
        if g is not None:
            g = global_features(g, batch, self.gin_channels, x.device)
            pointer, gbatch = _lib.ptr(g), g.shape[0]
        out = torch.empty(
            batch, 1, frames * self.head.istft.hop_length,
            dtype=torch.float32, device=x.device)
        if lengths is None:
            self._call(
                'pm_vocos_forward', engine, _lib.ptr(x), pointer, gbatch,
                _lib.ptr(out), batch=batch, frames=frames, device=x.device)
        else:
            lengths = check_lengths(lengths, batch, frames, x.device)
            self._call(
                'pm_vocos_forward_ragged', engine, _lib.ptr(x), pointer,
                gbatch, _lib.ptr(lengths, torch.int32), _lib.ptr(out),
                batch=batch, frames=frames, device=x.device,
                workspace_bytes='pm_vocos_ragged_workspace_bytes')
        return out

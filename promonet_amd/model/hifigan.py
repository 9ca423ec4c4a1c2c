"""HiFi-GAN vocoder running on the MI355X HIP engine.

Drop-in for `promonet.model.HiFiGAN` (promonet/model/hifigan.py:13-77):
same constructor arguments, same `forward(x, g, p)` signature, same
`state_dict()` keys / shapes (weight-normed layers keep `weight_g` and
`weight_v`), so a reference `generator-*.pt` loads unchanged. The forward
pass is one call into `libpromonet_hip.so` (`pm_hifigan_forward`); there is
no PyTorch compute path and no CPU fallback.
"""
import ctypes
import math

import torch

import promonet_amd
from promonet_amd import _lib
from .core import attach
from .engine import EngineModule, device_lengths, global_features


def checkpoint_schedule(stages):
    """The operand types 'checkpoint' (config.py) stands for, one per upsampling
    stage: f16 everywhere; in the LAST stage the activations split into hi + lo
    ('f16a2': its Blocks two MFMAs per step, its upsampler fully split), and
    the upsampler in front of the second-to-last stage fully split as well
    ('f16ux'). scripts/checkpoint_schedule.py measures the candidates."""
    if stages == 1:
        return ['f16a2']
    return ['f16'] * (stages - 2) + ['f16ux', 'f16a2']


class HiFiGAN(EngineModule):

    ABI = 'hifigan'

    def __init__(self, initial_channel, gin_channels):
        super().__init__()
        self.initial_channel = initial_channel
        self.gin_channels = gin_channels
        self.channels = promonet_amd.HIFIGAN_UPSAMPLE_INITIAL_SIZE
        self.rates = list(promonet_amd.HIFIGAN_UPSAMPLE_RATES)
        self.kernels = list(promonet_amd.HIFIGAN_UPSAMPLE_KERNEL_SIZES)
        self.res_kernels = list(promonet_amd.HIFIGAN_RESBLOCK_KERNEL_SIZES)
        self.res_dilations = [
            list(d) for d in promonet_amd.HIFIGAN_RESBLOCK_DILATION_SIZES]
        self.compute_dtype = promonet_amd.COMPUTE_DTYPE
        self.hopsize = math.prod(self.rates)

        for key, tensor in self._initial_state().items():
            attach(self, key, tensor)

    ###########################################################################
    # Parameters (reference init: hifigan.py:19-61, 220-223)
    ###########################################################################

    def _initial_state(self):
        state = {}

        def default_conv(prefix, cout, cin, k, bias=True):
            # torch.nn.Conv1d default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
            bound = 1. / math.sqrt(cin * k)
            state[f'{prefix}.weight'] = torch.empty(
                cout, cin, k).uniform_(-bound, bound)
            if bias:
                state[f'{prefix}.bias'] = torch.empty(
                    cout).uniform_(-bound, bound)

        def weight_normed(prefix, shape, nbias, fan_in):
            v = torch.randn(*shape) * .01
            bound = 1. / math.sqrt(fan_in)
            state[f'{prefix}.bias'] = torch.empty(nbias).uniform_(-bound, bound)
            state[f'{prefix}.weight_g'] = torch.linalg.vector_norm(
                v, dim=(1, 2), keepdim=True)
            state[f'{prefix}.weight_v'] = v

        c0 = self.channels
        default_conv('input_feature_conv', c0, self.initial_channel, 7)
        default_conv('input_speaker_conv', c0, self.gin_channels, 1)
        for i, (r, k) in enumerate(zip(self.rates, self.kernels)):
            cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
            weight_normed(
                f'model.{i}.model.1', (cin, cout, k), cout, cout * k)
            for j, ks in enumerate(self.res_kernels):
                for name in ('convs1', 'convs2'):
                    for n in range(len(self.res_dilations[j])):
                        weight_normed(
                            f'model.{i}.model.2.model.{j}.{name}.{n}',
                            (cout, cout, ks), cout, cout * ks)
        n = len(self.rates)
        default_conv(f'model.{n + 1}', 1, c0 // 2 ** n, 7, bias=False)
        return state

    ###########################################################################
    # Engine (handle lifetime, workspace and stream guard: engine.py)
    ###########################################################################

    def _key(self):
        return self.compute_dtype

    def _create(self, lib, handle):
        config = _lib.HifiganConfig()
        config.num_features = self.initial_channel
        config.global_channels = self.gin_channels
        config.initial_channels = self.channels
        config.num_stages = len(self.rates)
        for i, (r, k) in enumerate(zip(self.rates, self.kernels)):
            config.upsample_rates[i] = r
            config.upsample_kernel_sizes[i] = k
        config.num_resblocks = len(self.res_kernels)
        config.num_dilations = len(self.res_dilations[0])
        for j, k in enumerate(self.res_kernels):
            config.resblock_kernel_sizes[j] = k
            if len(self.res_dilations[j]) != config.num_dilations:
                raise ValueError('ragged dilation lists are not supported')
            for n, d in enumerate(self.res_dilations[j]):
                config.resblock_dilations[j][n] = d
        # 'checkpoint' / 'bf16' / 'f16' / 'fp32' / 'f16x3', or one operand type
        # per upsampling stage joined by '+' ('bf16+bf16+f16+f16': the input
        # conv takes the first)
        per_stage = str(self.compute_dtype).split('+')
        if per_stage == ['checkpoint']:
            per_stage = checkpoint_schedule(len(self.rates))
        if len(per_stage) not in (1, len(self.rates)):
            raise ValueError(
                f'COMPUTE_DTYPE {self.compute_dtype!r}: one operand type, or '
                f'one per stage ({len(self.rates)})')
        config.compute_dtype = _lib.DTYPES[per_stage[0]]
        if len(per_stage) > 1:
            for i, name in enumerate(per_stage):
                config.stage_compute_dtype[i] = 1 + _lib.DTYPES[name]
        return lib.pm_hifigan_create(ctypes.byref(config), handle)

    ###########################################################################
    # Forward
    ###########################################################################

    def forward(self, x, g, p=None):
        """x (B, C, T) features, g (B|1, G, 1) globals -> (B, 1, T * hop).

        `p` (previous samples) is accepted and ignored, as in the reference
        (promonet/model/hifigan.py:63)."""
        return self._run(x, g, channels_last=False)

    def forward_channels_last(self, x_cl, g, lengths=None):
        """x_cl (B, T, C_pad) as written by `pm_prepare_features`; `lengths`
        (B,) frames makes the batch ragged: every utterance is synthesised
        as if alone, the audio past its end is zero."""
        return self._run(x_cl, g, channels_last=True, lengths=lengths)

    def _run(self, x, g, channels_last, lengths=None):
        _lib.require_gpu(x)
        engine = self.engine()
        x = x.to(torch.float32).contiguous()
        batch = x.shape[0]
        frames = x.shape[1] if channels_last else x.shape[2]
        g = global_features(g, batch, self.gin_channels, x.device)
        if not channels_last and x.shape[1] != self.initial_channel:
            raise ValueError(
                f'expected {self.initial_channel} feature channels, '
                f'got {x.shape[1]}')
        out = torch.empty(
            batch, 1, frames * self.hopsize, dtype=torch.float32,
            device=x.device)
        if lengths is not None:
            lengths = device_lengths(lengths, batch, x.device)
            self._call(
                'pm_hifigan_forward_ragged', engine, _lib.ptr(x),
                int(channels_last), _lib.ptr(g), g.shape[0],
                _lib.ptr(lengths, torch.int32), _lib.ptr(out), batch=batch,
                frames=frames, device=x.device)
        else:
            self._call(
                'pm_hifigan_forward_cl' if channels_last
                else 'pm_hifigan_forward', engine, _lib.ptr(x), _lib.ptr(g),
                g.shape[0], _lib.ptr(out), batch=batch, frames=frames,
                device=x.device)
        return out

    def remove_weight_norm(self):
        """No-op: the engine folds weight norm once at load
        (reference: hifigan.py:72-77 only matters for TorchScript export)."""

"""The spectrograms at the entrance of the spectral discriminators on the HIP
kernels (pm_disc_spec.h), differentiable in the audio, and the conv stacks of
the FARGAN discriminator (pm_fdisc.h, pm_fdisc_strided.h), differentiable in
the maps and the parameters.

API of the three `spectrogram` methods of `promonet.model.discriminator`
(promonet/model/discriminator.py): DiscriminatorR (:129-143),
DiscriminatorCMB (:175-192) and SpecDiscriminatorBase (:278-299), and of
DiscriminatorMagFree (:320-389). The conv stacks of DiscriminatorMagFree are
in (`frequency_conv`, `weight_norm`, `DiscriminatorMagFree`), and so are those
of DiscriminatorCMB (:146-208) and DiscriminatorR (:96-127) on the kernels of
pm_dconv.h (`band_conv`, `DiscriminatorCMB`, `DiscriminatorR`) and that of
DiscriminatorP (:57-93) on the kernels of pm_pconv.h (`period_conv`,
`period_fold_conv`, `DiscriminatorP`), under the aggregate `Discriminator`
(:13-49); the stack of DiscriminatorS stays on torch. Neither direction syncs
with the host, and both capture into a graph on one stream.
"""
import math

import torch

from promonet_amd import _lib, config
from promonet_amd.loss import _check_sizes, _flat, _named_window, _twiddle

DEFAULT_BANDS = ((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75),
                 (0.75, 1.0))


###############################################################################
# The two calls
###############################################################################


class _Sizes(tuple):
    """(mode, fft_size, hop_size, win_length, pad)"""

    def frames(self, samples):
        _, fft_size, hop_size, _, pad = self
        return 1 + (samples + 2 * pad - fft_size) // hop_size

    def shape(self, batch, samples):
        bins, frames = self[1] // 2 + 1, self.frames(samples)
        if self[0] == _lib.DISC_SPEC_CMB:
            return batch, frames, bins
        return batch, bins, frames


def _sizes(mode, resolution, samples):
    """Checked sizes of a call; ValueError before any device work"""
    try:
        fft_size, hop_size, win_length = (int(v) for v in resolution)
    except (TypeError, ValueError):
        raise ValueError(
            f'resolution {resolution!r}: must be (n_fft, hop_length, '
            'win_length)') from None
    _check_sizes(fft_size, hop_size, win_length)
    pad = fft_size // 2 if mode == _lib.DISC_SPEC_DB else \
        int((fft_size - hop_size) / 2)
    if samples <= pad:
        raise ValueError(
            f'{samples} samples: reflect padding needs more than {pad}')
    if samples + 2 * pad < fft_size:
        raise ValueError(
            f'{samples} samples padded by {pad} on both sides are less than '
            f'one frame of {fft_size}')
    return _Sizes((mode, fft_size, hop_size, win_length, pad))


def _tables(device, sizes):
    mode, fft_size, _, win_length, _ = sizes
    # (torch.stft's window=None is win_length ones, centred in fft_size)
    name = 'hann_window' if mode == _lib.DISC_SPEC_DB else 'ones'
    return (_named_window(device, name, win_length, fft_size),
            _twiddle(device, fft_size))


def _workspace_of(size, device):
    return torch.empty(size, dtype=torch.uint8, device=device)


def _workspace(lib, sizes, flat, backward):
    return _workspace_of(lib.pm_disc_spec_workspace_bytes(
        sizes[0], *flat.shape, *sizes[1:], int(backward)), flat.device)


def _forward_call(flat, window, twiddle, sizes):
    """out in the mode's layout and, for DB, stats (2) = max, floor"""
    lib = _lib.lib()
    mode = sizes[0]
    out = torch.empty(sizes.shape(*flat.shape), device=flat.device)
    stats = workspace = None
    with torch.cuda.device(flat.device):
        if mode == _lib.DISC_SPEC_DB:
            stats = torch.empty(2, device=flat.device)
            workspace = _workspace(lib, sizes, flat, False)
        _lib.check(lib.pm_disc_spec_forward(
            mode, _lib.ptr(flat), _lib.ptr(window), _lib.ptr(twiddle),
            _lib.ptr(out), _lib.ptr(stats), *flat.shape, *sizes[1:],
            None if workspace is None else workspace.data_ptr(),
            0 if workspace is None else workspace.numel(), _lib.stream()))
    return out, stats


def _backward_call(flat, window, twiddle, sizes, upstream, out=None,
                   stats=None, into=None, scale=None):
    """grad_x (B, T) = scale * d <upstream, out> / d flat, or `into` += that"""
    lib = _lib.lib()
    result = torch.empty_like(flat) if into is None else into
    with torch.cuda.device(flat.device):
        workspace = _workspace(lib, sizes, flat, True)
        _lib.check(lib.pm_disc_spec_backward(
            sizes[0], _lib.ptr(flat), _lib.ptr(window), _lib.ptr(twiddle),
            _lib.ptr(upstream), _lib.ptr(out), _lib.ptr(stats),
            _lib.ptr(scale), _lib.ptr(result), int(into is not None),
            *flat.shape, *sizes[1:], workspace.data_ptr(), workspace.numel(),
            _lib.stream()))
    return result


class _Spectrogram(torch.autograd.Function):
    """backward: the transform again with the upstream gradient as the factor
    of the bin gradient, then the adjoint; DB reads the saved output and its
    (max, floor)."""

    @staticmethod
    def forward(ctx, flat, window, twiddle, sizes):
        out, stats = _forward_call(flat, window, twiddle, sizes)
        if sizes[0] == _lib.DISC_SPEC_DB:
            ctx.save_for_backward(flat, window, twiddle, out, stats)
        else:
            ctx.save_for_backward(flat, window, twiddle)
        ctx.sizes = sizes
        return out

    @staticmethod
    def backward(ctx, grad):
        flat, window, twiddle, *saved = ctx.saved_tensors
        grad = grad.to(torch.float32).contiguous()
        return _backward_call(
            flat, window, twiddle, ctx.sizes, grad, *saved), None, None, None


def _spectrogram(audio, mode, resolution):
    flat = _flat(audio, 'audio')
    sizes = _sizes(mode, resolution, flat.shape[1])
    _lib.require_gpu(flat)
    return _Spectrogram.apply(flat, *_tables(flat.device, sizes), sizes)


###############################################################################
# Public interface
###############################################################################


def spectrogram_resolution(audio, resolution):
    """DiscriminatorR.spectrogram: audio (B, 1, T) or (B, T) on the device,
    resolution (n_fft, hop_length, win_length) -> |STFT| (B, 1, n_fft / 2 + 1,
    frames) fp32, the audio reflect padded by (n_fft - hop_length) / 2 and the
    frames not centred, under a window of win_length ones."""
    return _spectrogram(audio, _lib.DISC_SPEC_R, resolution)[:, None]


def band_edges(bands=DEFAULT_BANDS):
    """The reference's band edges: int(f * (NUM_FFT // 2 + 1))"""
    bins = config.NUM_FFT // 2 + 1
    return [(int(low * bins), int(high * bins)) for low, high in bands]


def _multiband(audio, window_length, hop_size, edges):
    bins = window_length // 2 + 1
    for low, high in edges:
        if not 0 <= low <= high <= bins:
            raise ValueError(
                f'band ({low}, {high}): must lie within the {bins} bins')
    magnitude = _spectrogram(
        audio, _lib.DISC_SPEC_CMB,
        (window_length, hop_size, window_length))[:, None]
    return [magnitude[..., low:high] for low, high in edges]


def spectrogram_multiband(audio, bands=DEFAULT_BANDS):
    """DiscriminatorCMB.spectrogram: |STFT| with n_fft = win_length =
    WINDOW_SIZE and hop HOPSIZE as (B, 1, frames, bins), returned as the list
    of its bands [..., b0:b1], views of that one tensor. `bands` are fractions
    of the NUM_FFT // 2 + 1 bins."""
    return _multiband(
        audio, config.WINDOW_SIZE, config.HOPSIZE, band_edges(bands))


def spectrogram_decibel(audio, resolution):
    """SpecDiscriminatorBase.spectrogram: torch's centred STFT under a
    periodic Hann window, then amplitude_to_DB(multiplier=20, amin=1e-5,
    db_multiplier=0, top_db=80) of the 3-D magnitudes: 20 log10 max(|X|,
    1e-5), no lower than 80 dB under the maximum of the WHOLE batch ->
    (B, n_fft / 2 + 1, frames) fp32. The gradient passes through both branches
    of that maximum."""
    return _spectrogram(audio, _lib.DISC_SPEC_DB, resolution)


###############################################################################
# What the conv stacks share
###############################################################################


def _require_float(**tensors):
    for name, tensor in tensors.items():
        if not isinstance(tensor, torch.Tensor) or \
                not tensor.is_floating_point():
            raise ValueError(f'{name} must be a float tensor')


def _check_slope(slope):
    if isinstance(slope, bool) or not isinstance(slope, (int, float)) or \
            not math.isfinite(slope) or not 0. < slope <= 1.:
        raise ValueError(f'slope {slope!r}: must be finite and in (0, 1]')
    return float(slope)


def _check_pixels(name, tensor, pixels):
    """(the kernels count pixels in 32 bits)"""
    if pixels > 2 ** 31 - 1:
        raise ValueError(
            f'{name} {tuple(tensor.shape)}: more than 2^31 - 1 pixels')


def _map_order(tensor):
    """The memory order of the kernels: a map of several channels is
    channels_last, in memory (B, H, W, C); one channel is (B, H, W) either
    way, and the audio is (B, T)"""
    if tensor.ndim != 4 or tensor.shape[1] == 1:
        return tensor.contiguous()
    return tensor.contiguous(memory_format=torch.channels_last)


def _empty_map(shape, device):
    return torch.empty(
        shape, device=device, dtype=torch.float32,
        memory_format=torch.channels_last if shape[1] > 1
        else torch.contiguous_format)


def _address(tensor):
    """Of a map in the kernels' memory order (_lib.ptr takes plain contiguous
    tensors alone), or None"""
    return None if tensor is None else tensor.data_ptr()


class _ConvLayer(torch.autograd.Function):
    """One conv layer of a stack on its three C entries. `entries` = (forward,
    backward, workspace_bytes of _lib, the shape of the output from `sizes`);
    `sizes` are the ints of the workspace query, `scalars` what the two calls
    take after them (the dilation and the activation, or the slope), `tables`
    the tensors they take after the weight and the bias (the frequency
    embedding). backward: gx, gW and gb from the upstream gradient, the saved
    output and the saved input."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, x, weight, bias, entries, sizes, scalars, *tables):
        lib = _lib.lib()
        x, weight, bias = _map_order(x), weight.contiguous(), bias.contiguous()
        y = _empty_map(entries[3](*sizes), x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(lib, entries[0])(
                _address(x), _lib.ptr(weight), _lib.ptr(bias),
                *map(_lib.ptr, tables), _address(y), *sizes, *scalars,
                _lib.stream()))
        ctx.save_for_backward(x, weight, y, *tables)
        ctx.entries, ctx.sizes, ctx.scalars = entries, sizes, scalars
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad):
        lib = _lib.lib()
        x, weight, y, *tables = ctx.saved_tensors
        grad = _map_order(grad.to(torch.float32))
        need_x, need_weight, need_bias = ctx.needs_input_grad[:3]
        grad_x = torch.empty_like(x) if need_x else None
        grad_weight = grad_bias = workspace = None
        with torch.cuda.device(x.device):
            if need_weight or need_bias:
                grad_weight = torch.empty_like(weight)
                grad_bias = torch.empty(weight.shape[0], device=x.device)
                workspace = _workspace_of(
                    getattr(lib, ctx.entries[2])(*ctx.sizes), x.device)
            _lib.check(getattr(lib, ctx.entries[1])(
                _address(grad), _address(y), _address(x), _lib.ptr(weight),
                *map(_lib.ptr, tables), _address(grad_x),
                _lib.ptr(grad_weight), _lib.ptr(grad_bias), *ctx.sizes,
                *ctx.scalars, _address(workspace),
                0 if workspace is None else workspace.numel(), _lib.stream()))
        return (grad_x, grad_weight if need_weight else None,
                grad_bias if need_bias else None, None, None, None,
                *(None for _ in tables))


class _WeightNorm(torch.autograd.Function):

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, g, v):
        lib = _lib.lib()
        g, v = g.contiguous(), v.contiguous()
        w = torch.empty_like(v)
        with torch.cuda.device(v.device):
            _lib.check(lib.pm_fdisc_weight_norm_forward(
                _lib.ptr(g), _lib.ptr(v), _lib.ptr(w), v.shape[0],
                v[0].numel(), _lib.stream()))
        ctx.save_for_backward(g, v)
        return w

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad):
        lib = _lib.lib()
        g, v = ctx.saved_tensors
        grad = grad.to(torch.float32).contiguous()
        grad_g, grad_v = torch.empty_like(g), torch.empty_like(v)
        with torch.cuda.device(v.device):
            _lib.check(lib.pm_fdisc_weight_norm_backward(
                _lib.ptr(grad), _lib.ptr(g), _lib.ptr(v), _lib.ptr(grad_g),
                _lib.ptr(grad_v), v.shape[0], v[0].numel(), _lib.stream()))
        return grad_g, grad_v


def weight_norm(g, v):
    """torch._weight_norm(v, g, 0): w = g v / |v| with the norm of each output
    channel over its other axes. g (O, 1, ...) or (O), v (O, ...) on the
    device -> w like v, fp32, differentiable in both."""
    _require_float(g=g, v=v)
    if v.ndim < 2 or not v.numel() or g.numel() != v.shape[0] or \
            g.shape[:1] != v.shape[:1]:
        raise ValueError(
            f'g {tuple(g.shape)}, v {tuple(v.shape)}: one g per output '
            'channel of v')
    _lib.require_gpu(v)
    return _WeightNorm.apply(g.to(torch.float32), v.to(torch.float32))


class _NormedConv2d(torch.nn.Module):
    """The parameters of a weight-normed Conv2d(channels, out_channels,
    kernel_size), under the names torch.nn.utils.weight_norm gives; its
    stride or dilation is an attribute that its stack sets"""

    def __init__(self, channels, out_channels, kernel_size):
        super().__init__()
        conv = torch.nn.Conv2d(channels, out_channels, kernel_size)
        weight = conv.weight.detach()
        # (in the order weight_norm leaves them: bias, weight_g, weight_v)
        self.bias = torch.nn.Parameter(conv.bias.detach().clone())
        self.weight_g = torch.nn.Parameter(
            weight.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1))
        self.weight_v = torch.nn.Parameter(weight.clone())

    def weight(self):
        return weight_norm(self.weight_g, self.weight_v)


def _is_normed_conv(conv):
    """Is `conv` a weight-normed Conv2d with a bias, as the reference's are?"""
    return isinstance(conv, torch.nn.Conv2d) and conv.bias is not None and \
        isinstance(getattr(conv, 'weight_g', None), torch.Tensor) and \
        isinstance(getattr(conv, 'weight_v', None), torch.Tensor)


def _normed(conv):
    return weight_norm(conv.weight_g, conv.weight_v)


###############################################################################
# The conv stacks of DiscriminatorMagFree
###############################################################################

DILATIONS = (1, 2, 4, 8, 16)
RESOLUTIONS = (64, 128, 256, 512, 1024, 2048)
# (channels, out_channels, frequency stride) of the layers that the reference
# builds over its six resolutions beside the narrow ones, 1 or 16 channels on
# either side at stride 1 (magfree_plan): the kernels of pm_fdisc_strided.h
STRIDED_FORMS = frozenset(
    [(1, 16, 2)] +
    [(c, 2 * c, s) for c in (16, 32, 64, 128) for s in (1, 2)] +
    [(c, c, 1) for c in (32, 64, 128)] +
    [(c, 1, 1) for c in (32, 64, 128, 256)])
_TABLES = {}


def _embedding_table(device, bins):
    """(bins, 2) fp32 = sin, cos of FrequencyPositionalEmbedding (:381-389),
    by its own expression on the device; cached per device and size"""
    key = (str(device), bins)
    if key not in _TABLES:
        args = torch.arange(
            0, bins, dtype=torch.float32, device=device) * torch.pi * 2 / bins
        _TABLES[key] = torch.stack(
            (torch.sin(args), torch.cos(args)), dim=1).contiguous()
    return _TABLES[key]


def _layer_sizes(x, weight, bias, dilation, activation, stride=1):
    """((B, C, O, F, T), (d, act)) of a checked call of a narrow form, or
    ((B, C, O, F, T, s), (act,)) of one of STRIDED_FORMS; ValueError
    otherwise"""
    _require_float(x=x, weight=weight, bias=bias)
    if isinstance(stride, bool) or stride not in (1, 2):
        raise ValueError(f'stride {stride!r}: must be 1 or 2')
    if x.ndim != 4 or not x.numel():
        raise ValueError(
            f'x {tuple(x.shape)}: must be (B, C, F, T) with no empty axis')
    batch, channels, bins, frames = x.shape
    if weight.ndim != 4 or tuple(weight.shape[1:]) != (channels + 2, 3, 3):
        raise ValueError(
            f'weight {tuple(weight.shape)}: must be (O, {channels + 2}, 3, 3)')
    out_channels = weight.shape[0]
    narrow = stride == 1 and channels in (1, 16) and \
        out_channels in (1, 16) and (channels, out_channels) != (1, 1)
    if not narrow and (channels, out_channels, stride) not in STRIDED_FORMS:
        raise ValueError(
            f'channels {channels} -> {out_channels} at stride {stride}: no '
            'layer of the six stacks has that form (1 or 16 channels on '
            'either side at stride 1, not 1 on both, or one of '
            'STRIDED_FORMS)')
    if tuple(bias.shape) != (out_channels,):
        raise ValueError(
            f'bias {tuple(bias.shape)}: must be ({out_channels},)')
    if isinstance(dilation, (tuple, list)):
        if len(dilation) != 2 or dilation[1] != 1:
            raise ValueError(f'dilation {dilation!r}: must be (d, 1)')
        dilation = dilation[0]
    if dilation not in DILATIONS:
        raise ValueError(f'dilation {dilation!r}: must be one of {DILATIONS}')
    if activation not in _lib.FDISC_ACTIVATIONS:
        raise ValueError(
            f'activation {activation!r}: must be one of '
            f'{tuple(_lib.FDISC_ACTIVATIONS)}')
    if narrow:
        return (batch, channels, out_channels, bins, frames), \
            (int(dilation), _lib.FDISC_ACTIVATIONS[activation])
    if dilation != 1:
        raise ValueError(
            f'dilation {dilation!r}: a strided or wider layer has none')
    return (batch, channels, out_channels, bins, frames, int(stride)), \
        (_lib.FDISC_ACTIVATIONS[activation],)


_FREQUENCY_ENTRIES = (
    'pm_fdisc_conv_forward', 'pm_fdisc_conv_backward',
    'pm_fdisc_workspace_bytes',
    lambda batch, channels, out_channels, bins, frames:
        (batch, out_channels, bins, frames))


_STRIDED_ENTRIES = (
    'pm_fdisc_layer_forward', 'pm_fdisc_layer_backward',
    'pm_fdisc_layer_workspace_bytes',
    lambda batch, channels, out_channels, bins, frames, stride:
        (batch, out_channels, (bins - 1) // stride + 1, frames))


def frequency_conv(x, weight, bias, dilation=1, activation='relu', table=None,
                   stride=1):
    """One layer of DiscriminatorMagFree (:343-369) without its weight norm:
    act(conv2d(cat(x, sin, cos), weight, bias, stride (s, 1), dilation (d, 1),
    padding (d, 1))), sin and cos of 2 pi f / F being the two channels of
    FrequencyPositionalEmbedding on the layer's input. x (B, C, F, T) on the
    device, weight (O, C + 2, 3, 3), bias (O); activation 'relu', 'sigmoid' or
    'none'. With stride 1 and C, O in {1, 16} (not 1 on both sides) the
    dilation is one of DILATIONS; any other (C, O, stride) is one of
    STRIDED_FORMS and has dilation 1. Returns (B, O, (F - 1) // s + 1, T)
    fp32; with 16 or more channels it is channels_last in memory, as is the
    gradient in x. Differentiable in x, weight and bias. Other float dtypes
    are cast to fp32 and their gradients return in their dtype. `table` (F, 2)
    replaces sin and cos (the tests' integer embedding)."""
    sizes, scalars = _layer_sizes(
        x, weight, bias, dilation, activation, stride)
    if table is not None and tuple(table.shape) != (sizes[3], 2):
        raise ValueError(f'table {tuple(table.shape)}: must be (F, 2)')
    _lib.require_gpu(x)
    if table is None:
        table = _embedding_table(x.device, sizes[3])
    return _ConvLayer.apply(
        x.to(torch.float32), weight.to(torch.float32),
        bias.to(torch.float32),
        _FREQUENCY_ENTRIES if len(sizes) == 5 else _STRIDED_ENTRIES, sizes,
        scalars, table)


def magfree_plan(n_fft):
    """The six layers of DiscriminatorMagFree at a resolution, as (frequency
    stride, frequency dilation, channels, out_channels), restating what
    create_3x3_conv_plan(6, s, s, 0, 0) with s = log2(n_fft / 64) (:397-487,
    `configs` :302-319) and the channel rule of :342-357 give: the first s
    layers halve the frequency axis and double the channels (16 at first, 256
    at most), every other layer has stride 1, no layer is dilated, nothing
    happens on the time axis, and the last layer has one output channel."""
    if n_fft not in RESOLUTIONS:
        raise ValueError(f'n_fft {n_fft!r}: must be one of {RESOLUTIONS}')
    halvings = int(math.log2(n_fft // 64))
    layers, channels, out_channels = [], 1, 16
    for index in range(5):
        stride = 2 if index < halvings else 1
        layers.append((stride, 1, channels, out_channels))
        channels, out_channels = out_channels, min(stride * out_channels, 256)
    return layers + [(1, 1, channels, 1)]


class FrequencyPositionalEmbedding(torch.nn.Identity):
    """Slot 0 of a layer, as in the reference: no parameters. The kernels
    add the embedding themselves."""


def _frequency_module(channels, out_channels, dilation, stride=1):
    """Slot 1 of a layer: the parameters of its conv over the map and the two
    channels of the embedding"""
    conv = _NormedConv2d(channels + 2, out_channels, 3)
    conv.dilation = dilation
    conv.stride = stride
    return conv


class DiscriminatorMagFree(torch.nn.Module):
    """promonet.model.discriminator.DiscriminatorMagFree (:320-389) on the
    device: the decibel spectrogram, then six weight-normed 3x3 convs over
    (frequency, time) with the frequency embedding, 1 -> 16 -> ... -> 16 -> 1,
    ReLU after five and a sigmoid after the last. The state_dict has the
    reference's keys and shapes. `filterbank` is carried for the checkpoint
    only (the reference's forward never reads it) and starts as zeros.

    `strided=True` builds any of the six resolutions: at 128 ... 2048 the
    reference's layers halve the frequency axis and widen to 32 ... 256
    channels (magfree_plan, STRIDED_FORMS). Without it only n_fft = 64, whose
    stack is stride 1 and 16 channels throughout, is accepted and the others
    raise a ValueError. The keyword exists for that reason alone: the refusal
    was the interface while those layers had no kernel and the tests of that
    time pin it; a later change that may touch them flips the default."""

    def __init__(self, resolution, strided=False):
        super().__init__()
        self.resolution = tuple(int(v) for v in resolution)
        plan = magfree_plan(self.resolution[0])
        if not strided and any(stride != 1 or out_channels > 16
                               for stride, _, _, out_channels in plan):
            raise ValueError(
                f'n_fft {self.resolution[0]}: the layers of this resolution '
                'have a frequency stride of 2 and up to 256 channels; pass '
                'strided=True to build them (n_fft 64 alone is all stride 1 '
                'and 16 channels)')
        layers = []
        for stride, dilation, channels, out_channels in plan:
            last = out_channels == 1
            layers.append(torch.nn.Sequential(
                FrequencyPositionalEmbedding(),
                _frequency_module(channels, out_channels, dilation, stride),
                torch.nn.Sigmoid() if last else torch.nn.ReLU()))
        self.layers = torch.nn.ModuleList(layers)
        bins = self.resolution[0] // 2 + 1
        self.filterbank = torch.nn.Parameter(
            torch.zeros(bins, bins), requires_grad=False)

    def stack(self, x):
        """The six layers on x (B, 1, F, T): (logits (B, 1, F', T), [five
        maps]), F' the bins that the strided layers leave"""
        maps = []
        for layer in self.layers:
            conv = layer[1]
            x = frequency_conv(
                x, conv.weight(), conv.bias, conv.dilation,
                'sigmoid' if isinstance(layer[2], torch.nn.Sigmoid)
                else 'relu', stride=conv.stride)
            maps.append(x)
        return maps[-1], maps[:-1]

    def forward(self, audio):
        """audio (B, 1, T) -> (logits flattened to (B, F frames), the five
        feature maps), as SpecDiscriminatorBase.forward (:259-266)"""
        logits, maps = self.stack(
            spectrogram_decibel(audio, self.resolution).unsqueeze(1))
        return torch.flatten(logits, 1, -1), maps


def _stack_layers(self):
    """[(conv, dilation, activation, stride)] where every layer of a
    reference-style module has a form the kernels compute, or None"""
    layers, channels = [], 1
    for layer in getattr(self, 'layers', ()):
        if not isinstance(layer, torch.nn.Sequential) or len(layer) != 3:
            return None
        embedding, conv, activation = layer
        if type(embedding).__name__ != 'FrequencyPositionalEmbedding' or \
                not _is_normed_conv(conv):
            return None
        if conv.kernel_size != (3, 3) or conv.stride[1] != 1 or \
                conv.groups != 1 or conv.padding_mode != 'zeros' or \
                conv.dilation[1] != 1 or conv.dilation[0] not in DILATIONS or \
                tuple(conv.padding) != (conv.dilation[0], 1) or \
                conv.in_channels != channels + 2:
            return None
        narrow = conv.stride[0] == 1 and channels in (1, 16) and \
            conv.out_channels in (1, 16) and \
            (channels, conv.out_channels) != (1, 1)
        strided = conv.dilation[0] == 1 and \
            (channels, conv.out_channels, conv.stride[0]) in STRIDED_FORMS
        if not narrow and not strided:
            return None
        if isinstance(activation, torch.nn.ReLU):
            name = 'relu'
        elif isinstance(activation, torch.nn.Sigmoid):
            name = 'sigmoid'
        else:
            return None
        layers.append((conv, conv.dilation[0], name, conv.stride[0]))
        channels = conv.out_channels
    return layers or None


def _wrap_forward(original):
    def forward(self, x):
        layers = _stack_layers(self) if x.is_cuda else None
        if layers is None:
            return original(self, x)
        x = spectrogram_decibel(x, self.resolution).unsqueeze(1)
        output = []
        for conv, dilation, activation, stride in layers:
            x = frequency_conv(
                x, _normed(conv), conv.bias, dilation, activation,
                stride=stride)
            output.append(x)
        return torch.flatten(output[-1], 1, -1), output[:-1]
    forward.original = original
    return forward


###############################################################################
# The conv stacks of DiscriminatorCMB and DiscriminatorR
###############################################################################

# (channels, out_channels, kernel_width, stride): the whole reference
BAND_FORMS = ((1, 32, 9, 1), (32, 32, 9, 2), (32, 32, 3, 1), (32, 1, 3, 1))


def _band_sizes(x, weight, bias, stride, slope):
    """((B, C, O, H, W, kw, s), (slope,)) of a checked call; ValueError
    otherwise"""
    _require_float(x=x, weight=weight, bias=bias)
    if x.ndim != 4 or not x.numel():
        raise ValueError(
            f'x {tuple(x.shape)}: must be (B, C, H, W) with no empty axis')
    batch, channels, height, width = x.shape
    if isinstance(stride, (tuple, list)):
        if len(stride) != 2 or stride[0] != 1:
            raise ValueError(f'stride {stride!r}: must be (1, s)')
        stride = stride[1]
    if weight.ndim != 4 or weight.shape[2] != 3 or \
            (weight.shape[1], weight.shape[0], weight.shape[3], stride) \
            not in BAND_FORMS:
        raise ValueError(
            f'weight {tuple(weight.shape)} at stride {stride!r}: (channels, '
            f'out_channels, kernel_width, stride) must be one of {BAND_FORMS} '
            'with a kernel height of 3')
    if weight.shape[1] != channels:
        raise ValueError(
            f'x {tuple(x.shape)}: weight {tuple(weight.shape)} takes '
            f'{weight.shape[1]} channels')
    out_channels = weight.shape[0]
    if tuple(bias.shape) != (out_channels,):
        raise ValueError(
            f'bias {tuple(bias.shape)}: must be ({out_channels},)')
    slope = _check_slope(slope)
    _check_pixels('x', x, batch * height * width)
    return (batch, channels, out_channels, height, width, weight.shape[3],
            int(stride)), (slope,)


_BAND_ENTRIES = (
    'pm_dconv_forward', 'pm_dconv_backward', 'pm_dconv_workspace_bytes',
    lambda batch, channels, out_channels, height, width, kernel_width, stride:
        (batch, out_channels, height, (width - 1) // stride + 1))


def band_conv(x, weight, bias, stride=1, slope=1.0):
    """One layer of DiscriminatorCMB.band_convs / conv_post (:146-208) and of
    DiscriminatorR.convs / conv_post (:96-127) without its weight norm:
    leaky_relu(conv2d(x, weight, bias, stride (1, stride), padding (1, (kw -
    1) / 2)), slope). x (B, C, H, W) on the device, weight (O, C, 3, kw), bias
    (O), with (C, O, kw, stride) one of BAND_FORMS; slope in (0, 1], 1 being
    no activation. Returns (B, O, H, (W - 1) // stride + 1) fp32; with 32
    channels it is channels_last in memory, as is the gradient in x; a
    one-channel x that is not contiguous (a band of the spectrogram) is copied
    once. Differentiable in x, weight and bias. Other float dtypes are cast to
    fp32 and their gradients return in their dtype."""
    sizes, scalars = _band_sizes(x, weight, bias, stride, slope)
    _lib.require_gpu(x)
    return _ConvLayer.apply(
        x.to(torch.float32), weight.to(torch.float32),
        bias.to(torch.float32), _BAND_ENTRIES, sizes, scalars)


def _band_module(channels, out_channels, kernel_width, stride):
    conv = _NormedConv2d(channels, out_channels, (3, kernel_width))
    conv.stride = stride
    return conv


def _apply_band(conv, x, slope):
    return band_conv(x, conv.weight(), conv.bias, conv.stride, slope)


class DiscriminatorCMB(torch.nn.Module):
    """promonet.model.discriminator.DiscriminatorCMB (:146-208) on the device:
    the magnitude spectrogram in bands, five weight-normed convs a band under
    LeakyReLU(0.1), the bands' last maps joined on the width axis, and a 32 ->
    1 conv without activation. The state_dict has the reference's keys and
    shapes."""

    def __init__(self, bands=DEFAULT_BANDS):
        super().__init__()
        self.bands = tuple(tuple(band) for band in bands)
        self.band_convs = torch.nn.ModuleList([
            torch.nn.ModuleList([
                torch.nn.Sequential(
                    _band_module(*form), torch.nn.LeakyReLU(0.1))
                for form in BAND_FORMS[:1] + BAND_FORMS[1:2] * 3 +
                BAND_FORMS[2:3]])
            for _ in self.bands])
        self.conv_post = _band_module(*BAND_FORMS[3])

    def stack(self, bands_list):
        """The band tensors (B, 1, frames, bins of the band) -> (logits (B,
        1, frames, joined width), the 26 maps in the reference's order)"""
        last, maps = [], []
        for band, convs in zip(bands_list, self.band_convs):
            for layer in convs:
                band = _apply_band(layer[0], band, layer[1].negative_slope)
                maps.append(band)
            last.append(band)
        logits = _apply_band(self.conv_post, torch.cat(last, dim=-1), 1.)
        maps.append(logits)
        return logits, maps

    def forward(self, audio):
        """audio (B, 1, T) -> (logits flattened, the 26 maps)"""
        logits, maps = self.stack(spectrogram_multiband(audio, self.bands))
        return torch.flatten(logits, 1, -1), maps


class DiscriminatorR(torch.nn.Module):
    """promonet.model.discriminator.DiscriminatorR (:96-127) on the device:
    the magnitude spectrogram (B, 1, bins, frames), five weight-normed convs
    under leaky_relu(0.2), the maps taken after the activation, and a 32 -> 1
    conv without activation. The state_dict has the reference's keys and
    shapes."""

    SLOPE = 0.2

    def __init__(self, resolution):
        super().__init__()
        self.resolution = tuple(int(v) for v in resolution)
        self.convs = torch.nn.ModuleList([
            _band_module(*form)
            for form in BAND_FORMS[:1] + BAND_FORMS[1:2] * 3 +
            BAND_FORMS[2:3]])
        self.conv_post = _band_module(*BAND_FORMS[3])

    def stack(self, x):
        """x (B, 1, bins, frames) -> (logits (B, 1, bins, width), the six
        maps)"""
        maps = []
        for conv in self.convs:
            x = _apply_band(conv, x, self.SLOPE)
            maps.append(x)
        logits = _apply_band(self.conv_post, x, 1.)
        maps.append(logits)
        return logits, maps

    def forward(self, audio):
        """audio (B, 1, T) -> (logits flattened, the six maps)"""
        logits, maps = self.stack(
            spectrogram_resolution(audio, self.resolution))
        return torch.flatten(logits, 1, -1), maps


def _band_form(conv, channels):
    """The stride of a weight-normed Conv2d of one of BAND_FORMS that takes
    `channels` channels, or None"""
    if not _is_normed_conv(conv):
        return None
    kernel_width = conv.kernel_size[1]
    if conv.kernel_size[0] != 3 or conv.stride[0] != 1 or \
            tuple(conv.dilation) != (1, 1) or conv.groups != 1 or \
            conv.padding_mode != 'zeros' or conv.in_channels != channels or \
            tuple(conv.padding) != (1, (kernel_width - 1) // 2) or \
            (channels, conv.out_channels, kernel_width, conv.stride[1]) \
            not in BAND_FORMS:
        return None
    return conv.stride[1]


def _cmb_layers(self):
    """([[(conv, stride, slope)] a band], conv_post) where every layer of a
    reference-style DiscriminatorCMB has a form the kernels compute, or None"""
    stacks = []
    try:
        for convs in self.band_convs:
            layers, channels = [], 1
            for layer in convs:
                if not isinstance(layer, torch.nn.Sequential) or \
                        len(layer) != 2 or \
                        not isinstance(layer[1], torch.nn.LeakyReLU) or \
                        not 0. < layer[1].negative_slope <= 1.:
                    return None
                stride = _band_form(layer[0], channels)
                if stride is None:
                    return None
                layers.append((layer[0], stride, layer[1].negative_slope))
                channels = layer[0].out_channels
            if not layers or channels != 32:
                return None
            stacks.append(layers)
        if not stacks or _band_form(self.conv_post, 32) is None or \
                self.conv_post.out_channels != 1:
            return None
    except (AttributeError, TypeError):
        return None
    return stacks, self.conv_post


def _wrap_cmb_forward(original):
    def forward(self, x):
        found = _cmb_layers(self) if x.is_cuda else None
        if found is None:
            return original(self, x)
        stacks, post = found
        last, maps = [], []
        for band, layers in zip(self.spectrogram(x), stacks):
            for conv, stride, slope in layers:
                band = band_conv(band, _normed(conv), conv.bias, stride, slope)
                maps.append(band)
            last.append(band)
        logits = band_conv(
            torch.cat(last, dim=-1), _normed(post), post.bias, 1, 1.)
        maps.append(logits)
        return torch.flatten(logits, 1, -1), maps
    forward.original = original
    return forward


def _r_layers(self):
    """([(conv, stride)], conv_post) of a reference-style DiscriminatorR whose
    layers all have a form the kernels compute, or None"""
    layers, channels = [], 1
    try:
        for conv in self.convs:
            stride = _band_form(conv, channels)
            if stride is None:
                return None
            layers.append((conv, stride))
            channels = conv.out_channels
        if not layers or channels != 32 or \
                _band_form(self.conv_post, 32) is None or \
                self.conv_post.out_channels != 1:
            return None
    except (AttributeError, TypeError):
        return None
    return layers, self.conv_post


def _wrap_r_forward(original):
    def forward(self, audio):
        found = _r_layers(self) if audio.is_cuda else None
        if found is None:
            return original(self, audio)
        layers, post = found
        x, maps = self.spectrogram(audio), []
        for conv, stride in layers:
            x = band_conv(
                x, _normed(conv), conv.bias, stride, DiscriminatorR.SLOPE)
            maps.append(x)
        logits = band_conv(x, _normed(post), post.bias, 1, 1.)
        maps.append(logits)
        return torch.flatten(logits, 1, -1), maps
    forward.original = original
    return forward


###############################################################################
# The conv stack of DiscriminatorP, and the aggregate Discriminator
###############################################################################

# (channels, out_channels, kernel, stride): the whole reference, in the order
# of the layers, conv_post last
PERIOD_FORMS = ((1, 32, 5, 3), (32, 128, 5, 3), (128, 512, 5, 3),
                (512, 1024, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1))
PERIODS = (2, 3, 5, 7, 11)


def _check_period(period):
    if isinstance(period, bool) or not isinstance(period, int) or \
            not 1 <= period <= 64:
        raise ValueError(f'period {period!r}: must be an int in 1 ... 64')
    return period


def _check_parameters(weight, bias, forms, stride):
    """The form of a checked (weight, bias) at a stride; ValueError
    otherwise"""
    _require_float(weight=weight, bias=bias)
    if isinstance(stride, (tuple, list)):
        if len(stride) != 2 or stride[1] != 1:
            raise ValueError(f'stride {stride!r}: must be (s, 1)')
        stride = stride[0]
    if weight.ndim != 4 or weight.shape[3] != 1 or \
            (weight.shape[1], weight.shape[0], weight.shape[2], stride) \
            not in forms:
        raise ValueError(
            f'weight {tuple(weight.shape)} at stride {stride!r}: (channels, '
            f'out_channels, kernel, stride) must be one of {forms} with a '
            'kernel width of 1')
    if tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(
            f'bias {tuple(bias.shape)}: must be ({weight.shape[0]},)')
    return weight.shape[1], weight.shape[0], weight.shape[2], int(stride)


def _period_sizes(x, weight, bias, stride, slope):
    """((B, C, O, H, P, k, s), (slope,)) of a checked call; ValueError
    otherwise"""
    _require_float(x=x)
    if x.ndim != 4 or not x.numel():
        raise ValueError(
            f'x {tuple(x.shape)}: must be (B, C, H, P) with no empty axis')
    form = _check_parameters(weight, bias, PERIOD_FORMS, stride)
    batch, channels, height, period = x.shape
    if form[0] != channels:
        raise ValueError(
            f'x {tuple(x.shape)}: weight {tuple(weight.shape)} takes '
            f'{form[0]} channels')
    _check_period(period)
    slope = _check_slope(slope)
    _check_pixels('x', x, batch * height * period)
    return (batch, channels, form[1], height, period, form[2], form[3]), \
        (slope,)


def _fold_sizes(audio, weight, bias, period, slope):
    """((B, T, P), (slope,)) of a checked call; ValueError otherwise"""
    _require_float(audio=audio)
    if not (audio.ndim == 2 or (audio.ndim == 3 and audio.shape[1] == 1)) or \
            not audio.numel():
        raise ValueError(
            f'audio {tuple(audio.shape)}: must be (B, 1, T) or (B, T) with '
            'no empty axis')
    _check_parameters(weight, bias, PERIOD_FORMS[:1], 3)
    period = _check_period(period)
    slope = _check_slope(slope)
    batch, samples = audio.shape[0], audio.shape[-1]
    pad = (period - samples % period) % period
    if samples <= pad:
        raise ValueError(
            f'{samples} samples: reflect padding needs more than {pad}')
    _check_pixels('audio', audio, batch * (samples + pad))
    return (batch, samples, period), (slope,)


_PERIOD_ENTRIES = (
    'pm_pconv_forward', 'pm_pconv_backward', 'pm_pconv_workspace_bytes',
    lambda batch, channels, out_channels, height, period, kernel, stride:
        (batch, out_channels, (height - 1) // stride + 1, period))
# the first layer on the audio (B, T): the gradient in the audio holds the
# adjoint of the reflection
_FOLD_ENTRIES = (
    'pm_pconv_fold_forward', 'pm_pconv_fold_backward',
    'pm_pconv_fold_workspace_bytes',
    lambda batch, samples, period:
        (batch, 32, (-(-samples // period) - 1) // 3 + 1, period))


def period_conv(x, weight, bias, stride=1, slope=1.0):
    """One layer of DiscriminatorP.convs / conv_post (:57-93) without its
    weight norm: leaky_relu(conv2d(x, weight, bias, stride (stride, 1),
    padding ((k - 1) / 2, 0)), slope). x (B, C, H, P) on the device, P the
    period (1 ... 64), weight (O, C, k, 1), bias (O), with (C, O, k, stride)
    one of PERIOD_FORMS; slope in (0, 1], 1 being no activation. Returns (B,
    O, (H - 1) // stride + 1, P) fp32; with more than one channel it is
    channels_last in memory, as is the gradient in x. Differentiable in x,
    weight and bias. Other float dtypes are cast to fp32 and their gradients
    return in their dtype."""
    sizes, scalars = _period_sizes(x, weight, bias, stride, slope)
    _lib.require_gpu(x)
    return _ConvLayer.apply(
        x.to(torch.float32), weight.to(torch.float32),
        bias.to(torch.float32), _PERIOD_ENTRIES, sizes, scalars)


def period_fold_conv(audio, weight, bias, period, slope=1.0):
    """The first layer of DiscriminatorP on the audio itself: the reference's
    right reflect pad to a multiple of the period, its view as (B, 1, ceil(T
    / period), period) and period_conv at (1, 32, 5, 3), without the padded
    copy. audio (B, 1, T) or (B, T) on the device, weight (32, 1, 5, 1), bias
    (32). Returns (B, 32, Ho, period) fp32, channels_last. Differentiable in
    the audio (the gradient has the audio's shape and holds the adjoint of the
    reflection), weight and bias."""
    sizes, scalars = _fold_sizes(audio, weight, bias, period, slope)
    _lib.require_gpu(audio)
    return _ConvLayer.apply(
        audio.to(torch.float32).reshape(sizes[0], sizes[1]),
        weight.to(torch.float32), bias.to(torch.float32), _FOLD_ENTRIES,
        sizes, scalars)


def _period_module(channels, out_channels, kernel, stride):
    conv = _NormedConv2d(channels, out_channels, (kernel, 1))
    conv.stride = stride
    return conv


class DiscriminatorP(torch.nn.Module):
    """promonet.model.discriminator.DiscriminatorP (:57-93) on the device:
    the audio folded by the period, five weight-normed convs along the folded
    axis under leaky_relu(LRELU_SLOPE), the maps taken after the activation, and a
    1024 -> 1 conv without activation. The state_dict has the reference's
    keys and shapes."""

    def __init__(self, period):
        super().__init__()
        self.period = _check_period(period)
        self.convs = torch.nn.ModuleList(
            [_period_module(*form) for form in PERIOD_FORMS[:5]])
        self.conv_post = _period_module(*PERIOD_FORMS[5])

    def stack(self, audio):
        """audio (B, 1, T) -> (logits (B, 1, H, period), the six maps)"""
        first = self.convs[0]
        # (refused before the weight norm's device work)
        _fold_sizes(audio, first.weight_v, first.bias, self.period, 1.)
        x = period_fold_conv(
            audio, first.weight(), first.bias, self.period, config.LRELU_SLOPE)
        maps = [x]
        for conv in self.convs[1:]:
            x = period_conv(
                x, conv.weight(), conv.bias, conv.stride, config.LRELU_SLOPE)
            maps.append(x)
        logits = period_conv(
            x, self.conv_post.weight(), self.conv_post.bias, 1, 1.)
        maps.append(logits)
        return logits, maps

    def forward(self, audio):
        """audio (B, 1, T) -> (logits flattened, the six maps)"""
        logits, maps = self.stack(audio)
        return torch.flatten(logits, 1, -1), maps


class Discriminator(torch.nn.Module):
    """promonet.model.discriminator.Discriminator (:13-49) over the members
    that run on the device, in the reference's order: DiscriminatorP at each
    of `periods`, DiscriminatorR at each of `resolutions`, DiscriminatorCMB,
    DiscriminatorMagFree at each n_fft of `fargan`. The defaults are the
    reference's default configuration, whose checkpoint loads with
    strict=True; periods=(), complex_multiband=False, fargan=RESOLUTIONS is
    that of the two configurations with FARGAN_DISCRIMINATOR."""

    def __init__(self, periods=PERIODS, complex_multiband=True,
                 resolutions=(), fargan=()):
        super().__init__()
        members = [DiscriminatorP(period) for period in periods]
        members += [DiscriminatorR(resolution) for resolution in resolutions]
        if complex_multiband:
            members.append(DiscriminatorCMB())
        members += [DiscriminatorMagFree([n, n // 4, n], strided=True)
                    for n in fargan]
        self.discriminators = torch.nn.ModuleList(members)

    def forward(self, y, y_hat, **kwargs):
        """(logits real, logits fake, maps real, maps fake), a list entry a
        member"""
        logits_real, logits_fake, maps_real, maps_fake = [], [], [], []
        for member in self.discriminators:
            logits, maps = member(y, **kwargs)
            logits_real.append(logits)
            maps_real.append(maps)
            logits, maps = member(y_hat, **kwargs)
            logits_fake.append(logits)
            maps_fake.append(maps)
        return logits_real, logits_fake, maps_real, maps_fake


def _period_form(conv, form):
    """Is `conv` a weight-normed Conv2d of `form`, the stride and the padding
    on the height?"""
    channels, out_channels, kernel, stride = form
    return _is_normed_conv(conv) and conv.in_channels == channels and \
        conv.out_channels == out_channels and \
        tuple(conv.kernel_size) == (kernel, 1) and \
        tuple(conv.stride) == (stride, 1) and \
        tuple(conv.padding) == ((kernel - 1) // 2, 0) and \
        tuple(conv.dilation) == (1, 1) and conv.groups == 1 and \
        conv.padding_mode == 'zeros'


def _p_layers(self):
    """(convs, conv_post, period) of a reference-style DiscriminatorP whose
    layers are the six PERIOD_FORMS, or None"""
    try:
        convs = list(self.convs)
        period = self.period
        if len(convs) != 5 or isinstance(period, bool) or \
                not isinstance(period, int) or not 1 <= period <= 64 or \
                not all(_period_form(conv, form)
                        for conv, form in zip(convs, PERIOD_FORMS)) or \
                not _period_form(self.conv_post, PERIOD_FORMS[5]):
            return None
    except (AttributeError, TypeError):
        return None
    return convs, self.conv_post, period


def _wrap_p_forward(original):
    def forward(self, x):
        found = _p_layers(self) if x.is_cuda and x.ndim == 3 and \
            x.shape[1] == 1 else None
        if found is None:
            return original(self, x)
        convs, post, period = found
        pad = (period - x.shape[-1] % period) % period
        if x.shape[-1] <= pad:
            return original(self, x)
        x = period_fold_conv(
            x, _normed(convs[0]), convs[0].bias, period, config.LRELU_SLOPE)
        maps = [x]
        for conv in convs[1:]:
            x = period_conv(
                x, _normed(conv), conv.bias, conv.stride[0], config.LRELU_SLOPE)
            maps.append(x)
        logits = period_conv(x, _normed(post), post.bias, 1, 1.)
        maps.append(logits)
        return torch.flatten(logits, 1, -1), maps
    forward.original = original
    return forward


###############################################################################
# The wrappers promonet_amd.patch installs
###############################################################################


def _wrap(original, on_device):
    def spectrogram(self, x):
        if not x.is_cuda:
            return original(self, x)
        return on_device(self, x)
    spectrogram.original = original
    return spectrogram


def patch_module(module):
    """Replace the three spectrogram methods of a `model.discriminator`
    module, where it has them, and the `forward` of SpecDiscriminatorBase,
    where it has one; a tensor that is not on a GPU goes to the original
    method, and so does a module whose layers are not weight-normed 3x3 convs
    under the frequency embedding, each followed by ReLU or Sigmoid, of
    stride 1 with a frequency dilation of 1 ... 16 and 1 or 16 channels or of
    one of STRIDED_FORMS with no dilation. The `forward` of
    DiscriminatorCMB and of DiscriminatorR is replaced in the same way, where
    the class has one, for modules whose layers all have one of BAND_FORMS,
    and so is the `forward` of DiscriminatorP for modules whose layers are the
    six PERIOD_FORMS (a stride or a padding on the other axis goes to the
    original)."""
    wrappers = {
        'DiscriminatorR': lambda self, x: spectrogram_resolution(
            x, self.resolution),
        'DiscriminatorCMB': lambda self, x: _multiband(
            x, self.window_length, self.hop_size, self.bands),
        'SpecDiscriminatorBase': lambda self, x: spectrogram_decibel(
            x, self.resolution)}
    for name, on_device in wrappers.items():
        cls = getattr(module, name, None)
        if cls is None or hasattr(cls.spectrogram, 'original'):
            continue
        cls.spectrogram = _wrap(cls.spectrogram, on_device)
    base = getattr(module, 'SpecDiscriminatorBase', None)
    forward = getattr(base, 'forward', None)
    if forward is not None and not hasattr(forward, 'original'):
        base.forward = _wrap_forward(forward)
    # DiscriminatorCMB.forward and DiscriminatorR.forward, where the class has
    # one: on the device when every layer is a weight-normed Conv2d of one of
    # BAND_FORMS (in CMB inside Sequential(conv, LeakyReLU)), else the original
    # and DiscriminatorP.forward for the six PERIOD_FORMS
    for name, wrap in (('DiscriminatorCMB', _wrap_cmb_forward),
                       ('DiscriminatorR', _wrap_r_forward),
                       ('DiscriminatorP', _wrap_p_forward)):
        cls = getattr(module, name, None)
        forward = getattr(cls, 'forward', None)
        if forward is not None and not hasattr(forward, 'original'):
            cls.forward = wrap(forward)

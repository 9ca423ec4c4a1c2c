"""HiFi-GAN for training: the generator differentiable in its input and its
parameters, the convs of its MRF Blocks on the HIP kernels of pm_gconv.h in
both directions.

`block_conv` is one conv of `promonet.model.hifigan.Block` (:198-210) with its
input activation and its residual add; `Block` and `ResidualBlock` are the
reference's modules on it (:128-210); `HiFiGANTrainable` is the whole vocoder
(:13-77) with the state_dict of `promonet_amd.model.HiFiGAN`, whose forward
keeps nothing for a backward. The input, speaker and output convs and the four
upsamplers (3 % of the arithmetic) run on torch ops here, on weights from the
device's weight norm; a stage converts its map to channels_last once, at its
border. Neither direction syncs with the host, and a layer captures into a
graph on one stream. There is no CPU fallback.
"""
import math

import torch

import promonet_amd
from promonet_amd import _lib, config
from .discriminator import (
    _check_slope, _require_float, _workspace_of, weight_norm)

# the forms of pm_gconv_*: channels in and out are equal
CHANNELS = (32, 64, 128, 256)
KERNELS = (3, 7, 11)
DILATIONS = (1, 3, 5)


###############################################################################
# One conv of a Block
###############################################################################


def _rows(tensor):
    """(B, C, T) of any strides -> (B, T, C) contiguous: the kernels' memory
    order. No copy where the tensor is a view of such memory already."""
    return tensor.transpose(1, 2).contiguous()


def channels_last(tensor):
    """(B, C, T) as a view of (B, T, C) memory: what block_conv returns, and
    takes without a copy"""
    return _rows(tensor).transpose(1, 2)


class _BlockConv(torch.autograd.Function):
    """pm_gconv_forward / _backward. backward: gx, gW and gb from the upstream
    gradient and the saved input; the gradient of the residual is the upstream
    gradient itself."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, x, weight, bias, residual, dilation, slope):
        lib = _lib.lib()
        x, weight, bias = _rows(x), weight.contiguous(), bias.contiguous()
        if residual is not None:
            residual = _rows(residual)
        batch, frames, channels = x.shape
        sizes = (batch, channels, frames, weight.shape[2], dilation)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.pm_gconv_forward(
                _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias),
                _lib.ptr(residual), _lib.ptr(y), *sizes, slope,
                _lib.stream()))
        ctx.save_for_backward(x, weight)
        ctx.sizes, ctx.slope = sizes, slope
        return y.transpose(1, 2)

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad):
        lib = _lib.lib()
        x, weight = ctx.saved_tensors
        need_x, need_weight, need_bias, need_residual = \
            ctx.needs_input_grad[:4]
        upstream = _rows(grad.to(torch.float32))
        grad_x = torch.empty_like(x) if need_x else None
        grad_weight = grad_bias = workspace = None
        with torch.cuda.device(x.device):
            if need_weight or need_bias:
                grad_weight = torch.empty_like(weight)
                grad_bias = torch.empty(weight.shape[0], device=x.device)
                workspace = _workspace_of(
                    lib.pm_gconv_workspace_bytes(*ctx.sizes), x.device)
            if need_x or need_weight or need_bias:
                _lib.check(lib.pm_gconv_backward(
                    _lib.ptr(upstream), _lib.ptr(x), _lib.ptr(weight),
                    _lib.ptr(grad_x), _lib.ptr(grad_weight),
                    _lib.ptr(grad_bias), *ctx.sizes, ctx.slope,
                    None if workspace is None else workspace.data_ptr(),
                    0 if workspace is None else workspace.numel(),
                    _lib.stream()))
        return (None if grad_x is None else grad_x.transpose(1, 2),
                grad_weight if need_weight else None,
                grad_bias if need_bias else None,
                grad if need_residual else None, None, None)


def _block_sizes(x, weight, bias, dilation, slope, residual):
    """(dilation, slope) of a checked call; ValueError otherwise"""
    _require_float(x=x, weight=weight, bias=bias)
    if x.ndim != 3 or not x.numel():
        raise ValueError(
            f'x {tuple(x.shape)}: must be (B, C, T) with no empty axis')
    batch, channels, frames = x.shape
    if weight.ndim != 3 or weight.shape[0] != weight.shape[1] or \
            weight.shape[0] not in CHANNELS or weight.shape[2] not in KERNELS:
        raise ValueError(
            f'weight {tuple(weight.shape)}: must be (C, C, k) with C one of '
            f'{CHANNELS} and k one of {KERNELS}')
    if weight.shape[1] != channels:
        raise ValueError(
            f'x {tuple(x.shape)}: weight {tuple(weight.shape)} takes '
            f'{weight.shape[1]} channels')
    if tuple(bias.shape) != (channels,):
        raise ValueError(f'bias {tuple(bias.shape)}: must be ({channels},)')
    if isinstance(dilation, bool) or dilation not in DILATIONS:
        raise ValueError(f'dilation {dilation!r}: must be one of {DILATIONS}')
    slope = _check_slope(slope)
    if residual is not None:
        _require_float(residual=residual)
        if residual.shape != x.shape:
            raise ValueError(
                f'residual {tuple(residual.shape)}: must have the shape of x '
                f'{tuple(x.shape)}')
    # (the kernels count pixels in 32 bits)
    if batch * frames > 2 ** 31 - 1:
        raise ValueError(f'x {tuple(x.shape)}: more than 2^31 - 1 pixels')
    return int(dilation), slope


def block_conv(x, weight, bias, dilation=1, slope=config.LRELU_SLOPE,
               residual=None):
    """One conv of Block (:198-210) without its weight norm, with its input
    activation and its residual add:
        conv1d(leaky_relu(x, slope), weight, bias, dilation=dilation,
               padding=(k - 1) dilation / 2) [+ residual].
    x and residual (B, C, T) on the device, of any strides; weight (C, C, k),
    bias (C), with C one of CHANNELS, k one of KERNELS and the dilation one of
    DILATIONS; slope in (0, 1], 1 being no activation. Returns (B, C, T) fp32,
    a view of channels_last memory (B, T, C), as is the gradient in x; such a
    view passes from layer to layer without a copy. Differentiable in x,
    weight, bias and residual. Other float dtypes are cast to fp32 (autocast
    computes in fp32) and their gradients return in their dtype. There is no
    CPU fallback."""
    dilation, slope = _block_sizes(x, weight, bias, dilation, slope, residual)
    _lib.require_gpu(x)
    return _BlockConv.apply(
        x.to(torch.float32), weight.to(torch.float32), bias.to(torch.float32),
        None if residual is None else residual.to(torch.float32), dilation,
        slope)


###############################################################################
# The modules
###############################################################################


class _Normed(torch.nn.Module):
    """The parameters of a weight-normed conv under the names
    torch.nn.utils.weight_norm gives, initialised as the reference's
    (init_weights, :220-223: v ~ N(0, .01), g = |v|; the bias torch's
    default). `shape` is that of the weight, `fan_in` of the bias bound."""

    def __init__(self, shape, biases, fan_in):
        super().__init__()
        v = torch.randn(*shape) * .01
        bound = 1. / math.sqrt(fan_in)
        # (in the order weight_norm leaves them: bias, weight_g, weight_v)
        self.bias = torch.nn.Parameter(
            torch.empty(biases).uniform_(-bound, bound))
        self.weight_g = torch.nn.Parameter(
            torch.linalg.vector_norm(v, dim=(1, 2), keepdim=True))
        self.weight_v = torch.nn.Parameter(v)

    def weight(self):
        return weight_norm(self.weight_g, self.weight_v)


def _check_form(channels, kernel_size, dilations):
    if channels not in CHANNELS or kernel_size not in KERNELS or \
            not dilations or any(d not in DILATIONS for d in dilations):
        raise ValueError(
            f'channels {channels!r}, kernel_size {kernel_size!r}, dilation '
            f'{dilations!r}: must be of {CHANNELS}, {KERNELS} and {DILATIONS}')


class Block(torch.nn.Module):
    """promonet.model.hifigan.Block (:157-218) on the device: per dilation d,
    x = c2(leaky(c1(leaky(x)))) + x with c1 dilated by d and c2 by 1, two
    block_conv calls with the add fused into the second. The state_dict has
    the reference's keys and shapes."""

    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.dilation = tuple(int(d) for d in dilation)
        _check_form(channels, kernel_size, self.dilation)
        shape = (channels, channels, kernel_size)
        self.convs1, self.convs2 = (
            torch.nn.ModuleList([
                _Normed(shape, channels, channels * kernel_size)
                for _ in self.dilation])
            for _ in range(2))

    def forward(self, x):
        slope = config.LRELU_SLOPE
        for c1, c2, d in zip(self.convs1, self.convs2, self.dilation):
            xt = block_conv(x, c1.weight(), c1.bias, d, slope)
            x = block_conv(xt, c2.weight(), c2.bias, 1, slope, residual=x)
        return x


class ResidualBlock(torch.nn.Module):
    """promonet.model.hifigan.ResidualBlock (:128-149): the sum of the Blocks
    of HIFIGAN_RESBLOCK_KERNEL_SIZES / _DILATION_SIZES on one input, divided
    by their number. The input is brought to channels_last once."""

    def __init__(self, channels):
        super().__init__()
        self.model = torch.nn.ModuleList([
            Block(channels, kernel_size, dilation)
            for kernel_size, dilation in zip(
                promonet_amd.HIFIGAN_RESBLOCK_KERNEL_SIZES,
                promonet_amd.HIFIGAN_RESBLOCK_DILATION_SIZES)])

    def forward(self, x):
        _require_float(x=x)
        if x.ndim != 3:
            raise ValueError(f'x {tuple(x.shape)}: must be (B, C, T)')
        x = channels_last(x)
        xs = None
        for layer in self.model:
            xs = layer(x) if xs is None else xs + layer(x)
        return xs / len(self.model)


class _Plain(torch.nn.Module):
    """The parameters of a torch.nn.Conv1d(channels, out_channels, kernel)
    under its names and its default initialisation"""

    def __init__(self, out_channels, channels, kernel, bias=True):
        super().__init__()
        bound = 1. / math.sqrt(channels * kernel)
        self.weight = torch.nn.Parameter(torch.empty(
            out_channels, channels, kernel).uniform_(-bound, bound))
        if bias:
            self.bias = torch.nn.Parameter(
                torch.empty(out_channels).uniform_(-bound, bound))


class _Stage(torch.nn.Module):
    """The keys of MultiReceptiveFieldFusion (:84-120): model.1 the
    weight-normed ConvTranspose1d, model.2 the ResidualBlock"""

    def __init__(self, channels, out_channels, kernel, rate):
        super().__init__()
        if kernel < rate or (kernel - rate) % 2:
            raise ValueError(
                f'upsampler rate {rate} kernel {kernel}: the padding (k - r) '
                '/ 2 must be a whole number')
        self.rate, self.padding = rate, (kernel - rate) // 2
        self.model = torch.nn.ModuleDict({
            '1': _Normed((channels, out_channels, kernel), out_channels,
                         out_channels * kernel),
            '2': ResidualBlock(out_channels)})

    def forward(self, x):
        upsampler = self.model['1']
        x = torch.nn.functional.conv_transpose1d(
            torch.nn.functional.leaky_relu(x, config.LRELU_SLOPE),
            upsampler.weight(), upsampler.bias, stride=self.rate,
            padding=self.padding)
        return self.model['2'](x)


class HiFiGANTrainable(torch.nn.Module):
    """promonet.model.HiFiGAN (:13-77) for training. The state_dict has the
    keys, the order and the shapes of `promonet_amd.model.HiFiGAN`, and loads
    into it and from it with strict=True; every parameter requires grad. The
    convs of the Blocks run on block_conv; the input, speaker and output convs
    and the upsamplers on torch ops in fp32."""

    def __init__(self, initial_channel, gin_channels):
        super().__init__()
        channels = promonet_amd.HIFIGAN_UPSAMPLE_INITIAL_SIZE
        rates = list(promonet_amd.HIFIGAN_UPSAMPLE_RATES)
        kernels = list(promonet_amd.HIFIGAN_UPSAMPLE_KERNEL_SIZES)
        self.hopsize = math.prod(rates)
        self.input_feature_conv = _Plain(channels, initial_channel, 7)
        self.input_speaker_conv = _Plain(channels, gin_channels, 1)
        model = {}
        for index, (rate, kernel) in enumerate(zip(rates, kernels)):
            model[str(index)] = _Stage(
                channels // 2 ** index, channels // 2 ** (index + 1), kernel,
                rate)
        self.stages = len(rates)
        model[str(self.stages + 1)] = _Plain(
            1, channels // 2 ** self.stages, 7, bias=False)
        self.model = torch.nn.ModuleDict(model)

    def forward(self, x, g, p=None):
        """x (B, C, T) features, g (B|1, G, 1) globals -> (B, 1, T * hop),
        differentiable in x, g and every parameter. `p` is accepted and
        ignored, as in the reference (:63)."""
        _require_float(x=x, g=g)
        _lib.require_gpu(x)
        functional = torch.nn.functional
        with torch.autocast('cuda', enabled=False):
            x, g = x.to(torch.float32), g.to(torch.float32)
            x = functional.conv1d(
                x, self.input_feature_conv.weight,
                self.input_feature_conv.bias, padding=3)
            x = x + functional.conv1d(
                g, self.input_speaker_conv.weight,
                self.input_speaker_conv.bias)
            for index in range(self.stages):
                x = self.model[str(index)](x)
            x = functional.leaky_relu(x, config.LRELU_SLOPE)
            x = functional.conv1d(
                x, self.model[str(self.stages + 1)].weight, None, padding=3)
            return torch.tanh(x)


###############################################################################
# The wrapper promonet_amd.patch installs
###############################################################################


def _conv_form(conv, activation, channels, kernel):
    """(dilation, slope) of a weight-normed Conv1d of a form of pm_gconv_*
    under its LeakyReLU, or None"""
    if not isinstance(conv, torch.nn.Conv1d) or conv.bias is None or \
            not isinstance(getattr(conv, 'weight_g', None), torch.Tensor) or \
            not isinstance(getattr(conv, 'weight_v', None), torch.Tensor) or \
            not isinstance(activation, torch.nn.LeakyReLU):
        return None
    dilation, slope = conv.dilation[0], activation.negative_slope
    if conv.in_channels != channels or conv.out_channels != channels or \
            tuple(conv.kernel_size) != (kernel,) or \
            tuple(conv.stride) != (1,) or dilation not in DILATIONS or \
            tuple(conv.padding) != ((kernel - 1) // 2 * dilation,) or \
            conv.groups != 1 or conv.padding_mode != 'zeros' or \
            not (math.isfinite(slope) and 0. < slope <= 1.):
        return None
    return dilation, float(slope)


def _block_layers(self):
    """[(c1, d1, slope1, c2, d2, slope2)] of a reference-style Block whose
    convs all have a form the kernels compute, or None"""
    try:
        lists = [list(getattr(self, name)) for name in (
            'convs1', 'convs2', 'activations1', 'activations2')]
        if not lists[0] or len(set(map(len, lists))) != 1:
            return None
        channels = lists[0][0].in_channels
        kernel = lists[0][0].kernel_size[0]
        if channels not in CHANNELS or kernel not in KERNELS:
            return None
        layers = []
        for c1, c2, a1, a2 in zip(*lists):
            first = _conv_form(c1, a1, channels, kernel)
            second = _conv_form(c2, a2, channels, kernel)
            if first is None or second is None:
                return None
            layers.append((c1, *first, c2, *second))
    except (AttributeError, TypeError, IndexError):
        return None
    return layers


def _wrap_block_forward(original):
    def forward(self, x):
        found = _block_layers(self) \
            if isinstance(x, torch.Tensor) and x.is_cuda and x.ndim == 3 and \
            x.is_floating_point() and x.numel() and \
            torch.is_grad_enabled() else None
        if found is None:
            return original(self, x)
        for c1, d1, slope1, c2, d2, slope2 in found:
            xt = block_conv(
                x, weight_norm(c1.weight_g, c1.weight_v), c1.bias, d1, slope1)
            x = block_conv(
                xt, weight_norm(c2.weight_g, c2.weight_v), c2.bias, d2,
                slope2, residual=x)
        return x
    forward.original = original
    return forward


def patch_module(module):
    """Replace the `forward` of the Block of a `model.hifigan` module, where
    it has one: on the device with autograd on, a Block whose convs are all
    weight-normed Conv1d of a form of pm_gconv_* under LeakyReLU runs on
    block_conv; anything else goes to the original, which is kept and wrapped
    once."""
    cls = getattr(module, 'Block', None)
    forward = getattr(cls, 'forward', None)
    if forward is not None and not hasattr(forward, 'original'):
        cls.forward = _wrap_block_forward(forward)

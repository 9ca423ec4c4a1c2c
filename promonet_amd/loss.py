"""Training-side losses on the HIP kernels.

API of `promonet.loss` (promonet/train/loss.py): the adversarial losses
`feature_matching`, `discriminator` and `generator` (:11-53) as one
multi-tensor mean each (pm_adv.h), and `stft`, `SpectralConvergence`,
`MultiResolutionSpectralConvergence` and `signal` (:61-162), differentiable in
the prediction through HIP backward passes (pm_loss.h), the target a constant.
Neither direction syncs with the host, and both capture into a graph on one
stream.
"""
import ctypes

import numpy as np
import torch

from promonet_amd import _lib, config

MIN_FFT, MAX_FFT = 64, 2560


###############################################################################
# Tables
###############################################################################


def _check_sizes(fft_size, hop_size, win_length, samples=None):
    rest = fft_size // 5 if fft_size % 5 == 0 else fft_size
    if (not MIN_FFT <= fft_size <= MAX_FFT) or rest & (rest - 1):
        raise ValueError(
            f'fft_size {fft_size}: must be 2^a or 5 * 2^a with '
            f'{MIN_FFT} <= fft_size <= {MAX_FFT}')
    if not 1 <= hop_size <= fft_size:
        raise ValueError(
            f'hop_size {hop_size}: must be between 1 and fft_size {fft_size}')
    if not 1 <= win_length <= fft_size:
        raise ValueError(
            f'win_length {win_length}: must be between 1 and fft_size '
            f'{fft_size}')
    if samples is not None and samples <= fft_size // 2:
        raise ValueError(
            f'{samples} samples: reflect padding needs more than '
            f'fft_size / 2 = {fft_size // 2}')


def _check_window(name):
    if not isinstance(name, str) or not callable(getattr(torch, name, None)):
        raise ValueError(
            f'window {name!r}: must name a window function of torch, such '
            'as hann_window')


def _twiddle(device, fft_size):
    """(fft_size, 2) = (cos, -sin)(2 pi m / fft_size), rounded from float64;
    built once per device and size."""
    cache = _twiddle.__dict__.setdefault('cache', {})
    key = (device, fft_size)
    if key not in cache:
        angle = 2. * np.pi * np.arange(fft_size, dtype=np.float64) / fft_size
        table = np.stack([np.cos(angle), -np.sin(angle)], 1).astype(np.float32)
        cache[key] = torch.from_numpy(table).to(device).contiguous()
    return cache[key]


def _named_window(device, name, win_length, fft_size):
    """getattr(torch, name)(win_length) in float64 on the host, centred in
    fft_size zeros, as fp32 on the device; once per device, name and size."""
    cache = _named_window.__dict__.setdefault('cache', {})
    key = (device, name, win_length, fft_size)
    if key not in cache:
        _check_window(name)
        window = getattr(torch, name)(win_length, dtype=torch.float64)
        left = (fft_size - win_length) // 2
        table = torch.zeros(fft_size, dtype=torch.float64)
        table[left:left + win_length] = window
        cache[key] = table.to(torch.float32).to(device).contiguous()
    return cache[key]


def _padded_window(window, fft_size):
    """A caller's window tensor centred in fft_size zeros, on its device (no
    host copy: the call stays asynchronous)."""
    left = (fft_size - window.numel()) // 2
    return torch.nn.functional.pad(
        window.to(torch.float32),
        (left, fft_size - window.numel() - left)).contiguous()


def _flat(x, name):
    """(B, 1, T) or (B, T), any float dtype -> contiguous fp32 (B, T)"""
    if x.ndim == 3 and x.shape[1] == 1:
        x = x[:, 0]
    if x.ndim != 2:
        raise ValueError(f'{name} must be (B, 1, T) or (B, T), got '
                         f'{tuple(x.shape)}')
    if not x.is_floating_point():
        raise ValueError(f'{name} must be a float tensor, got {x.dtype}')
    return x.to(torch.float32).contiguous()


def _constant(tensor, name):
    """The target carries no gradient: say so before any work is queued."""
    if torch.is_grad_enabled() and tensor.requires_grad:
        raise NotImplementedError(
            f'no gradient with respect to {name}: the target is a constant '
            '(detach it)')


###############################################################################
# The three stages
###############################################################################


def _stft_call(flat, window, twiddle, fft_size, hop_size, upstream=None,
               want_s=True, want_gradient=False):
    lib = _lib.lib()
    batch, samples = flat.shape
    shape = (batch, fft_size // 2 + 1, 1 + samples // hop_size)
    s = torch.empty(shape, device=flat.device) if want_s else None
    gradient = torch.empty(
        shape + (2,), device=flat.device) if want_gradient else None
    with torch.cuda.device(flat.device):
        _lib.check(lib.pm_sc_stft(
            _lib.ptr(flat), _lib.ptr(window), _lib.ptr(twiddle),
            _lib.ptr(upstream), _lib.ptr(s), _lib.ptr(gradient), batch,
            samples, fft_size, hop_size, _lib.stream()))
    return s, gradient


def _forward_call(x, y, window, twiddle, fft_size, hop_size, with_gradient):
    """sums (3) = S1, S2, S1 / S2 and the workspace (G first), or None"""
    lib = _lib.lib()
    batch, samples = x.shape
    sums = torch.empty(3, device=x.device)
    with torch.cuda.device(x.device):
        size = lib.pm_sc_forward_workspace_bytes(
            batch, samples, fft_size, hop_size, int(with_gradient))
        workspace = torch.empty(size, dtype=torch.uint8, device=x.device)
        _lib.check(lib.pm_sc_forward(
            _lib.ptr(x), _lib.ptr(y), _lib.ptr(window), _lib.ptr(twiddle),
            _lib.ptr(sums), batch, samples, fft_size, hop_size,
            int(with_gradient), workspace.data_ptr(), workspace.numel(),
            _lib.stream()))
    return sums, workspace if with_gradient else None


def _adjoint_call(gradient, window, twiddle, scale, grad_x, fft_size,
                  hop_size, accumulate):
    """grad_x (B, T) = (or +=) scale * adjoint(G); `gradient` is any
    contiguous device buffer that begins with G (B, bins, frames, 2) fp32"""
    lib = _lib.lib()
    batch, samples = grad_x.shape
    with torch.cuda.device(grad_x.device):
        size = lib.pm_sc_adjoint_workspace_bytes(
            batch, samples, fft_size, hop_size)
        workspace = torch.empty(size, dtype=torch.uint8, device=grad_x.device)
        _lib.check(lib.pm_sc_adjoint(
            gradient.data_ptr(), _lib.ptr(window), _lib.ptr(twiddle),
            _lib.ptr(scale), _lib.ptr(grad_x), batch, samples, fft_size,
            hop_size, int(accumulate), workspace.data_ptr(),
            workspace.numel(), _lib.stream()))


class _Stft(torch.autograd.Function):
    """s = sqrt(max(|STFT(x)|, 1e-7)); backward: the transform again with the
    upstream gradient as the factor of G, then the adjoint."""

    @staticmethod
    def forward(ctx, flat, window, twiddle, fft_size, hop_size):
        ctx.save_for_backward(flat, window, twiddle)
        ctx.sizes = fft_size, hop_size
        return _stft_call(flat, window, twiddle, fft_size, hop_size)[0]

    @staticmethod
    def backward(ctx, grad):
        flat, window, twiddle = ctx.saved_tensors
        fft_size, hop_size = ctx.sizes
        if ctx.needs_input_grad[1]:
            raise NotImplementedError(
                'promonet_amd.loss.stft has no gradient with respect to the '
                'window')
        grad = grad.to(torch.float32).contiguous()
        _, gradient = _stft_call(
            flat, window, twiddle, fft_size, hop_size, upstream=grad,
            want_s=False, want_gradient=True)
        result = torch.empty_like(flat)
        _adjoint_call(gradient, window, twiddle, torch.ones_like(grad[0, 0, :1]),
                      result, fft_size, hop_size, False)
        return result, None, None, None, None


class _SpectralConvergence(torch.autograd.Function):
    """The mean over `resolutions` of S1 / S2. The forward keeps every
    resolution's G; the backward runs the adjoints into one grad_x in stream
    order, each scaled by grad_out / (S2 * resolutions) on the device."""

    @staticmethod
    def forward(ctx, x, y, resolutions, *tables):
        with_gradient = ctx.needs_input_grad[0]
        sums, kept = [], []
        for i, (fft_size, hop_size) in enumerate(resolutions):
            window, twiddle = tables[2 * i], tables[2 * i + 1]
            total, workspace = _forward_call(
                x, y, window, twiddle, fft_size, hop_size, with_gradient)
            sums.append(total)
            kept.append(workspace)
        sums = torch.stack(sums)
        ctx.resolutions, ctx.tables = resolutions, tables
        ctx.kept, ctx.shape = kept, x.shape
        ctx.save_for_backward(sums)
        return sums[:, 2].mean()

    @staticmethod
    def backward(ctx, grad):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError(
                'the spectral-convergence loss has no gradient with respect '
                'to the target y: it is a constant (detach it)')
        sums, = ctx.saved_tensors
        count = len(ctx.resolutions)
        scales = (grad.to(torch.float32) / (sums[:, 1] * count)).contiguous()
        result = torch.empty(ctx.shape, device=sums.device)
        for i, (fft_size, hop_size) in enumerate(ctx.resolutions):
            _adjoint_call(
                ctx.kept[i], ctx.tables[2 * i], ctx.tables[2 * i + 1],
                scales[i:i + 1], result, fft_size, hop_size, i > 0)
        return (result, None, None) + (None,) * len(ctx.tables)


###############################################################################
# Public interface
###############################################################################


def stft(x, fft_size, hop_size, win_length, window):
    """sqrt(max(|STFT(x)|, 1e-7)) (loss.py:61-80): x (B, T) on the device,
    window a tensor of win_length values -> (B, fft_size / 2 + 1, frames)
    fp32, frames = 1 + T // hop_size, with torch.stft's center=True reflect
    padding."""
    flat = _flat(x, 'x')
    if window.numel() != win_length:
        raise ValueError(
            f'window has {window.numel()} values, win_length is {win_length}')
    _check_sizes(fft_size, hop_size, win_length, flat.shape[1])
    _constant(window, 'the window')
    _lib.require_gpu(flat)
    table = _padded_window(window.to(flat.device), fft_size)
    twiddle = _twiddle(flat.device, fft_size)
    if torch.is_grad_enabled() and x.requires_grad:
        return _Stft.apply(flat, table, twiddle, fft_size, hop_size)
    return _stft_call(flat, table, twiddle, fft_size, hop_size)[0]


def _spectral_convergence(x, y, resolutions, tables):
    x_flat, y_flat = _flat(x, 'x'), _flat(y, 'y')
    if x_flat.shape != y_flat.shape:
        raise ValueError(
            f'x {tuple(x.shape)} and y {tuple(y.shape)} differ in shape')
    for fft_size, hop_size in resolutions:
        _check_sizes(fft_size, hop_size, fft_size, x_flat.shape[1])
    _constant(y, 'y')
    _lib.require_gpu(x_flat)
    _lib.require_gpu(y_flat)
    return _SpectralConvergence.apply(x_flat, y_flat, resolutions, *tables)


class SpectralConvergence(torch.nn.Module):
    """sum |s_y - s_x| / sum s_y over the whole batch (loss.py:83-121)"""

    def __init__(
        self,
        device,
        fft_size=1024,
        shift_size=120,
        win_length=600,
        window='hann_window'
    ):
        super().__init__()
        _check_sizes(fft_size, shift_size, win_length)
        _check_window(window)
        device = torch.device(device)
        self.fft_size = fft_size
        self.shift_size = shift_size
        self.win_length = win_length
        self.tables = (
            _named_window(device, window, win_length, fft_size),
            _twiddle(device, fft_size))

    def forward(self, x, y):
        """x predicted, y target, (B, 1, T) or (B, T) -> 0-d device tensor"""
        return _spectral_convergence(
            x, y, ((self.fft_size, self.shift_size),), self.tables)


class MultiResolutionSpectralConvergence(torch.nn.Module):
    """The mean of SpectralConvergence over resolutions (loss.py:124-150)"""

    def __init__(
        self,
        device,
        fft_sizes=[2560, 1280, 640, 320, 160, 80],
        hop_sizes=[640, 320, 160, 80, 40, 20],
        win_lengths=[2560, 1280, 640, 320, 160, 80],
        window='hann_window'
    ):
        super().__init__()
        self.stft_losses = torch.nn.ModuleList([
            SpectralConvergence(device, fs, ss, wl, window)
            for fs, ss, wl in zip(fft_sizes, hop_sizes, win_lengths)])

    def forward(self, x, y):
        losses = self.stft_losses
        if not len(losses):
            raise ValueError('no resolutions')
        return _spectral_convergence(
            x, y, tuple((l.fft_size, l.shift_size) for l in losses),
            tuple(t for l in losses for t in l.tables))


class _Signal(torch.autograd.Function):

    @staticmethod
    def forward(ctx, y_true, y_pred):
        lib = _lib.lib()
        rows, samples = y_pred.shape
        out = torch.empty(1, device=y_pred.device)
        with torch.cuda.device(y_pred.device):
            size = lib.pm_signal_loss_workspace_bytes(rows)
            stats = torch.empty(size, dtype=torch.uint8, device=y_pred.device)
            _lib.check(lib.pm_signal_loss(
                _lib.ptr(y_true), _lib.ptr(y_pred), _lib.ptr(out), rows,
                samples, stats.data_ptr(), stats.numel(), _lib.stream()))
        ctx.save_for_backward(y_true, y_pred, stats)
        return out[0]

    @staticmethod
    def backward(ctx, grad):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError(
                'promonet_amd.loss.signal has no gradient with respect to '
                'y_true: the target is a constant (detach it)')
        y_true, y_pred, stats = ctx.saved_tensors
        lib = _lib.lib()
        rows, samples = y_pred.shape
        grad = grad.to(torch.float32).reshape(1).contiguous()
        result = torch.empty_like(y_pred)
        with torch.cuda.device(y_pred.device):
            _lib.check(lib.pm_signal_loss_backward(
                _lib.ptr(y_true), _lib.ptr(y_pred), _lib.ptr(grad),
                _lib.ptr(result), rows, samples, stats.data_ptr(),
                stats.numel(), _lib.stream()))
        return None, result


def signal(y_true, y_pred):
    """Waveform loss (loss.py:158-162): the mean over rows of 1 - <p, t>, p
    and t the rows (last axis) over (1e-15 + their L2 norm)."""
    if y_true.shape != y_pred.shape or y_pred.ndim < 1:
        raise ValueError(
            f'y_true {tuple(y_true.shape)} and y_pred {tuple(y_pred.shape)} '
            'must have the same shape')
    if not y_pred.numel():
        raise ValueError('signal needs at least one sample')
    _constant(y_true, 'y_true')
    _lib.require_gpu(y_pred)
    _lib.require_gpu(y_true)
    samples = y_pred.shape[-1]
    return _Signal.apply(
        y_true.reshape(-1, samples).to(torch.float32).contiguous(),
        y_pred.reshape(-1, samples).to(torch.float32).contiguous())


###############################################################################
# Adversarial losses: one multi-tensor mean a call
###############################################################################


_ADV_DTYPES = {torch.float32: _lib.PM_F32, torch.float16: _lib.PM_F16,
               torch.bfloat16: _lib.PM_BF16}
_DENSE_FORMATS = {4: (torch.channels_last,), 5: (torch.channels_last_3d,)}


def _dense(tensor):
    """Whether the tensor fills its memory in one of torch's memory formats
    (a mean does not depend on the order of its elements)"""
    return tensor.is_contiguous() or any(
        tensor.is_contiguous(memory_format=memory_format)
        for memory_format in _DENSE_FORMATS.get(tensor.ndim, ()))


def _adv_tensor(tensor, name):
    if not isinstance(tensor, torch.Tensor) or \
            not tensor.is_floating_point():
        raise ValueError(f'{name} must be a float tensor')
    if not tensor.numel():
        raise ValueError(f'{name} is empty')


def _adv_single(tensor):
    """fp32 / f16 / bf16 as stored, anything else as fp32; dense"""
    if tensor.dtype not in _ADV_DTYPES:
        tensor = tensor.to(torch.float32)
    return tensor if _dense(tensor) else tensor.contiguous()


def _adv_pair(real, fake):
    """A pair shares one dtype and one order in memory"""
    if real.dtype != fake.dtype or real.dtype not in _ADV_DTYPES:
        real, fake = real.to(torch.float32), fake.to(torch.float32)
    if real.stride() != fake.stride() or not _dense(fake):
        real, fake = real.contiguous(), fake.contiguous()
    return real, fake


def _adv_lists(first, second, names):
    if len(first) != len(second):
        raise ValueError(
            f'{names[0]} has {len(first)} entries, {names[1]} '
            f'{len(second)}')
    if not len(first):
        raise ValueError(f'{names[0]} is empty')
    for index, (one, other) in enumerate(zip(first, second)):
        _adv_tensor(one, f'{names[0]}[{index}]')
        _adv_tensor(other, f'{names[1]}[{index}]')
        if one.shape != other.shape:
            raise ValueError(
                f'{names[0]}[{index}] {tuple(one.shape)} and '
                f'{names[1]}[{index}] {tuple(other.shape)} differ in shape')


def _adv_arrays(a, b, ops):
    """The host arrays of pm_multi_mean for tensors a, b (or None)"""
    count = len(a)
    pointers = ctypes.c_void_p * count
    return (
        pointers(*(t.data_ptr() for t in a)),
        pointers(*(t.data_ptr() for t in b)) if b else None,
        (ctypes.c_longlong * count)(*(t.numel() for t in a)),
        (ctypes.c_int * count)(*ops),
        (ctypes.c_int * count)(*(_ADV_DTYPES[t.dtype] for t in a)))


class _MultiMean(torch.autograd.Function):
    """(total, means) of op_k over tensor k of a flattened list: `count`
    tensors a, then (feature matching) their `count` partners b. The means
    are for logging and carry no gradient."""

    @staticmethod
    def forward(ctx, ops, count, *tensors):
        lib = _lib.lib()
        a, b = tensors[:count], tensors[count:]
        arrays = _adv_arrays(a, b, ops)
        device = a[0].device
        out = torch.empty(count + 1, device=device)
        with torch.cuda.device(device):
            size = lib.pm_multi_mean_workspace_bytes(arrays[2], count)
            workspace = torch.empty(size, dtype=torch.uint8, device=device)
            _lib.check(lib.pm_multi_mean(
                *arrays, count, _lib.ptr(out), workspace.data_ptr(), size,
                _lib.stream()))
        ctx.ops, ctx.count = ops, count
        ctx.save_for_backward(*tensors)
        total, means = out[count], out[:count]
        ctx.mark_non_differentiable(means)
        return total, means

    @staticmethod
    def backward(ctx, grad, _):
        lib = _lib.lib()
        ops, count = ctx.ops, ctx.count
        tensors = ctx.saved_tensors
        a, b = tensors[:count], tensors[count:]
        # (torch.empty_like keeps the strides of a dense tensor)
        grads = [
            torch.empty_like(t)
            if ctx.needs_input_grad[2 + i] and
            (i >= count) == (ops[i % count] == _lib.ADV_ABS_DIFF) else None
            for i, t in enumerate(tensors)]
        if any(g is not None for g in grads):
            grad = grad.to(torch.float32).reshape(1).contiguous()
            pointers = ctypes.c_void_p * count
            grad_a = pointers(*(
                None if g is None else g.data_ptr() for g in grads[:count]))
            grad_b = pointers(*(
                None if g is None else g.data_ptr()
                for g in grads[count:])) if b else None
            with torch.cuda.device(grad.device):
                _lib.check(lib.pm_multi_mean_backward(
                    *_adv_arrays(a, b, ops), count, _lib.ptr(grad), grad_a,
                    grad_b, None, 0, _lib.stream()))
        return (None, None) + tuple(grads)


def _multi_mean(ops, a, b=()):
    for tensor in tuple(a) + tuple(b):
        _lib.require_gpu(tensor)
    total, means = _MultiMean.apply(tuple(ops), len(a), *a, *b)
    return total, list(means.unbind())


def feature_matching(real_feature_maps, fake_feature_maps):
    """Feature matching loss (loss.py:11-26): the sum over every pair of maps
    of mean |real - fake|, as a 0-d fp32 device tensor. Lists (one per
    discriminator) of lists of maps; FEATURE_MATCHING_OMIT_FIRST skips each
    discriminator's first map. fp32, f16 and bf16 maps are read as stored.
    The gradient goes to the fake maps only: the real ones are constants, as
    the reference detaches them."""
    if len(real_feature_maps) != len(fake_feature_maps):
        raise ValueError(
            f'real_feature_maps has {len(real_feature_maps)} lists, '
            f'fake_feature_maps {len(fake_feature_maps)}')
    skip = int(bool(config.FEATURE_MATCHING_OMIT_FIRST))
    real, fake = [], []
    for index, (reals, fakes) in enumerate(
            zip(real_feature_maps, fake_feature_maps)):
        if len(reals) != len(fakes):
            raise ValueError(
                f'discriminator {index} has {len(reals)} real maps and '
                f'{len(fakes)} fake maps')
        if len(reals) > skip:
            _adv_lists(reals[skip:], fakes[skip:],
                       (f'real_feature_maps[{index}]',
                        f'fake_feature_maps[{index}]'))
        real.extend(reals[skip:])
        fake.extend(fakes[skip:])
    if not real:
        raise ValueError('no feature maps')
    pairs = [_adv_pair(r.detach(), f) for r, f in zip(real, fake)]
    return _multi_mean(
        (_lib.ADV_ABS_DIFF,) * len(pairs), [p[0] for p in pairs],
        [p[1] for p in pairs])[0]


def discriminator(real_outputs, fake_outputs):
    """Discriminator loss (loss.py:29-40) -> (total, real_losses,
    fake_losses): mean (1 - real)^2 and mean fake^2 per discriminator, or
    with ADVERSARIAL_HINGE_LOSS mean max(1 - real, 0) and mean max(1 + fake,
    0), in one launch set over both lists. The gradient of `total` goes to
    both lists; the per-discriminator losses are for logging and carry no
    gradient."""
    _adv_lists(real_outputs, fake_outputs, ('real_outputs', 'fake_outputs'))
    count = len(real_outputs)
    if config.ADVERSARIAL_HINGE_LOSS:
        ops = (_lib.ADV_HINGE_ONE_MINUS,) * count + \
            (_lib.ADV_HINGE_ONE_PLUS,) * count
    else:
        ops = (_lib.ADV_SQ_ONE_MINUS,) * count + (_lib.ADV_SQ,) * count
    total, losses = _multi_mean(
        ops, [_adv_single(t) for t in real_outputs] +
        [_adv_single(t) for t in fake_outputs])
    return total, losses[:count], losses[count:]


def generator(discriminator_outputs):
    """Generator adversarial loss (loss.py:43-53) -> (total, losses): mean
    (1 - output)^2 per discriminator, or with ADVERSARIAL_HINGE_LOSS mean
    max(1 - output, 0). The per-discriminator losses are for logging and
    carry no gradient."""
    if not len(discriminator_outputs):
        raise ValueError('discriminator_outputs is empty')
    for index, tensor in enumerate(discriminator_outputs):
        _adv_tensor(tensor, f'discriminator_outputs[{index}]')
    op = _lib.ADV_HINGE_ONE_MINUS if config.ADVERSARIAL_HINGE_LOSS else \
        _lib.ADV_SQ_ONE_MINUS
    return _multi_mean(
        (op,) * len(discriminator_outputs),
        [_adv_single(t) for t in discriminator_outputs])

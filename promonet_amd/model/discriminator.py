"""The spectrograms at the entrance of the spectral discriminators on the HIP
kernels (pm_disc_spec.h), differentiable in the audio.

API of the three `spectrogram` methods of `promonet.model.discriminator`
(promonet/model/discriminator.py): DiscriminatorR (:129-143),
DiscriminatorCMB (:175-192) and SpecDiscriminatorBase (:278-299). The conv
stacks behind them stay on torch. Neither direction syncs with the host, and
both capture into a graph on one stream.
"""
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


def _workspace(lib, sizes, flat, backward):
    size = lib.pm_disc_spec_workspace_bytes(
        sizes[0], *flat.shape, *sizes[1:], int(backward))
    return torch.empty(size, dtype=torch.uint8, device=flat.device)


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
    module, where it has them; a tensor that is not on a GPU goes to the
    original method."""
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

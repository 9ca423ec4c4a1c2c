"""A-weighted loudness on the HIP kernels.

API of `promonet.preprocess.loudness` (promonet/preprocess/loudness.py),
the editing utilities `limit` / `scale` / `shift` (:114-193) included.
"""
import ctypes

import numpy as np
import torch

import promonet_amd
from promonet_amd import _lib


def from_audio(audio, bands=1):
    """A-weighted loudness (loudness.py:17-55), computed on the GPU.

    audio (1, N) -> (bands, N // 256); `bands=None` keeps the 513 bins.
    Also accepts (B, N) and returns (B, bands, T): every utterance gets its
    own max - 80 dB floor, as separate reference calls would.
    """
    lib = _lib.lib()
    _lib.require_gpu(audio)
    flat = audio.to(torch.float32).contiguous()
    batch, samples = flat.shape
    frames = samples // promonet_amd.HOPSIZE
    bins = promonet_amd.WINDOW_SIZE // 2 + 1
    nbands = bins if bands is None else int(bands)
    if nbands > 16 and nbands != bins:
        raise ValueError('at most 16 loudness bands (or None for all bins)')
    weights = perceptual_weights_tensor(flat.device)
    device = flat.device
    with torch.cuda.device(device):
        size = lib.pm_loudness_scratch_bytes(batch, samples)
        scratch = torch.empty(max(size, 1), dtype=torch.uint8, device=device)
        out = torch.empty(batch, nbands, frames, device=device)
        _lib.check(lib.pm_loudness(
            _lib.ptr(flat), _lib.ptr(weights), _lib.ptr(out), batch,
            samples, nbands, promonet_amd.MIN_DB, scratch.data_ptr(),
            scratch.numel(), _lib.stream()))
    return out[0] if batch == 1 else out


def from_file(audio_file, bands=None, gpu=0):
    """loudness.py:58-60"""
    bands = promonet_amd.LOUDNESS_BANDS if bands is None else bands
    return from_audio(
        promonet_amd.load.audio(audio_file).to(f'cuda:{gpu}'), bands)


def from_file_to_file(audio_file, output_file, bands=None, gpu=0):
    """loudness.py:63-65"""
    torch.save(from_file(audio_file, bands, gpu).cpu(), output_file)


def from_files_to_files(audio_files, output_files, bands=None, gpu=0):
    """loudness.py:68-76"""
    for audio_file, output_file in zip(audio_files, output_files):
        from_file_to_file(audio_file, output_file, bands, gpu)


###############################################################################
# Loudness utilities
###############################################################################


def band_average(loudness, bands=None):
    """Average over frequency bands (loudness.py:84-111). Index arithmetic
    on an existing tensor; the fused path is `from_audio(audio, bands)`."""
    bands = promonet_amd.LOUDNESS_BANDS if bands is None else bands
    if bands == 1:
        return loudness.mean(dim=-2, keepdim=True)
    step = loudness.shape[-2] / bands
    return torch.stack(
        [
            loudness[..., int(b * step):int((b + 1) * step), :].mean(dim=-2)
            for b in range(int(bands))
        ],
        dim=-2)


def limit_tile():
    """(chunk, tile) of the limiter kernel: the steps one lane takes and the
    steps one workgroup pass covers (pm_limit.h). Needs no GPU."""
    chunk, tile = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().pm_limit_tile(
        ctypes.byref(chunk), ctypes.byref(tile)))
    return chunk.value, tile.value


def _rows(audio):
    """fp32 rows with unit element stride, and their row stride"""
    _lib.require_gpu(audio)
    if audio.dim() != 2:
        raise ValueError('audio must be (1, samples) or (batch, samples)')
    rows = audio.to(torch.float32)
    if rows.shape[1] > 1 and rows.stride(1) != 1 or (
            rows.shape[0] > 1 and rows.stride(0) < rows.shape[1]):
        rows = rows.contiguous()
    stride = rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]
    return rows, max(stride, rows.shape[1])


def _lengths(lengths, rows, device):
    """None, or a device int32 tensor of one length per row"""
    if lengths is None:
        return None
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.tensor(list(lengths), dtype=torch.int32)
    lengths = lengths.to(device=device, dtype=torch.int32).contiguous()
    if lengths.shape != (rows,):
        raise ValueError(f'{rows} rows, lengths of shape {tuple(lengths.shape)}')
    return lengths


def limit(audio, delay=40, attack_coef=.9, release_coef=.9995, threshold=.99,
          lengths=None):
    """The look-ahead limiter (loudness.py:114-141) on the GPU, bit for bit
    the reference's fp32 loop. audio (1, T) or (B, T), not modified; `lengths`
    (a list or a device tensor, read on the device only) makes the batch
    ragged: a row is limited over its own length and zero beyond it.

    Like the reference it does not hold the output under 1: a burst passes
    while the gain, smoothed by `attack_coef`, is still on its way down. After
    the first limiting event the gain comes to rest at 1 - 4 ulp, not at 1."""
    return limit_with_trace(audio, delay, attack_coef, release_coef,
                            threshold, lengths, trace=False)[0]


def limit_with_trace(audio, delay=40, attack_coef=.9, release_coef=.9995,
                     threshold=.99, lengths=None, trace=True):
    """`limit`, and what the kernel leaves for tests and diagnosis: (output,
    gain, counts). gain (B, T + delay - 1) holds g[0 .. length + delay - 2]
    of every row and zeros beyond; counts (B, 4) int32 = envelope steps and
    gain steps walked by one lane, chunks walked, tiles skipped as a whole."""
    lib = _lib.lib()
    rows, stride = _rows(audio)
    batch, samples = rows.shape
    device = rows.device
    delay = int(delay)
    lengths = _lengths(lengths, batch, device)
    with torch.cuda.device(device):
        out = torch.empty(batch, samples, device=device)
        gain = torch.empty(
            batch, samples + max(delay, 1) - 1, device=device
        ) if trace else None
        size = max(lib.pm_limit_workspace_bytes(batch), 16)
        workspace = torch.zeros(size // 4, dtype=torch.int32, device=device)
        _lib.check(lib.pm_limit(
            rows.data_ptr(), _lib.ptr(lengths, torch.int32), _lib.ptr(out),
            _lib.ptr(gain), batch, samples, stride, samples, delay,
            attack_coef, 1 - attack_coef, release_coef, threshold,
            workspace.data_ptr(), 4 * workspace.numel(), _lib.stream()))
    if samples == 0 and trace:
        gain.fill_(1.)
    return out, gain, workspace[:4 * batch].reshape(batch, 4)


def shift(audio, value, lengths=None, frame_lengths=None):
    """Shift loudness by `value` decibels (loudness.py:179-193) on the GPU.
    A Python scalar shifts every sample alike; a tensor (1, F) or (B, F) is a
    contour, converted to a gain 2^(value / 10) per frame and interpolated
    linearly to the audio's samples as torch.nn.functional.interpolate(mode=
    'linear', align_corners=False) does. With `lengths` / `frame_lengths`
    (lists or device tensors) each row interpolates its own frames to its own
    samples and is zero beyond them. audio (1, N) or (B, N); returns fp32."""
    lib = _lib.lib()
    rows, stride = _rows(audio)
    batch, samples = rows.shape
    device = rows.device
    if isinstance(value, torch.Tensor) and value.numel() > 1:
        _lib.require_gpu(value)
        if value.dim() != 2 or value.shape[0] not in (1, batch):
            raise ValueError('value must be a scalar, (1, frames) or '
                             '(batch, frames)')
        db = value.to(torch.float32).contiguous()
    elif isinstance(value, torch.Tensor):
        _lib.require_gpu(value)
        db = value.to(torch.float32).reshape(1, 1)
    else:
        db = torch.full((1, 1), float(value), device=device)
    frames = db.shape[1]
    lengths = _lengths(lengths, batch, device)
    frame_lengths = _lengths(frame_lengths, batch, device)
    with torch.cuda.device(device):
        out = torch.empty(batch, samples, device=device)
        _lib.check(lib.pm_loudness_shift(
            rows.data_ptr(), _lib.ptr(db), _lib.ptr(lengths, torch.int32),
            _lib.ptr(frame_lengths, torch.int32), _lib.ptr(out), batch,
            samples, stride, frames, frames if db.shape[0] > 1 else 0,
            samples, _lib.stream()))
    return out


def scale(audio, target_loudness, reference_gain=True):
    """Scale the audio to the target loudness (loudness.py:163-176) on the
    GPU: limit(shift(audio, gain)). audio (1, N) with the target (bands, T),
    or (B, N) with (B, bands, T), T = N // 256; full rows only.

    `reference_gain=True` keeps a quirk of the reference: it converts the
    difference in dB to a ratio and `shift` then converts that ratio as if it
    were dB a second time. `False` shifts by target - loudness dB once."""
    _lib.require_gpu(audio)
    _lib.require_gpu(target_loudness)
    target = target_loudness.to(torch.float32)
    if target.shape[-2] > 1:
        target = target.mean(dim=-2, keepdim=True)
    difference = target - from_audio(audio)
    if reference_gain:
        difference = promonet_amd.convert.db_to_ratio(difference)
    return limit(shift(audio, difference.reshape(audio.shape[0], -1)))


def normalize(loudness):
    """Normalize loudness to [-1., 1.] (loudness.py:144-146)"""
    return (loudness - promonet_amd.MIN_DB) / (
        promonet_amd.REF_DB - promonet_amd.MIN_DB)


def perceptual_weights():
    """A_weighting(fft_frequencies) - REF_DB, (513, 1) (loudness.py:149-160).
    `librosa.A_weighting` restated (IEC 61672, floor -80 dB): PARITY
    UNPINNED, librosa is absent from the build container."""
    freqs = np.linspace(
        0, promonet_amd.SAMPLE_RATE / 2, 1 + promonet_amd.WINDOW_SIZE // 2)
    f2 = freqs ** 2
    c = np.array([12194.217, 20.598997, 107.65265, 737.86223]) ** 2
    with np.errstate(divide='ignore'):
        weights = 2. + 20. * (
            np.log10(c[0]) + 2 * np.log10(f2) - np.log10(f2 + c[0]) -
            np.log10(f2 + c[1]) - .5 * np.log10(f2 + c[2]) -
            .5 * np.log10(f2 + c[3]))
    weights = np.maximum(-80., weights)
    return weights[:, None] - float(promonet_amd.REF_DB)


def perceptual_weights_tensor(device):
    cache = perceptual_weights_tensor.__dict__.setdefault('cache', {})
    if device not in cache:
        cache[device] = torch.from_numpy(
            perceptual_weights()[:, 0].astype(np.float32)).to(device)
    return cache[device]

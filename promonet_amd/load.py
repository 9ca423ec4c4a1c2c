"""Loading utilities on the hot path (reference: promonet/load.py)."""
import math

import numpy as np
import torch

import promonet_amd


def pitch_distribution(dataset=None, partition='train'):
    """The 256 ascending pitch-bin edges (Hz) of the default configuration.

    Reference: promonet/load.py:54-111 reads
    `assets/stats/{dataset}-{PITCH_BINS}{-loudness}{-pitch}{-viterbi}.pt`;
    the same values ship here as a .npy (the reference recomputes them from
    the training set when the file is missing - out of scope).
    """
    if not hasattr(pitch_distribution, 'distribution'):
        dataset = dataset or promonet_amd.TRAINING_DATASET
        key = ''
        if promonet_amd.AUGMENT_LOUDNESS:
            key += '-loudness'
        if promonet_amd.AUGMENT_PITCH:
            key += '-pitch'
        if promonet_amd.VITERBI_DECODE_PITCH:
            key += '-viterbi'
        file = (
            promonet_amd.ASSETS_DIR / 'stats' /
            f'{dataset}-{promonet_amd.PITCH_BINS}{key}.npy')
        if not file.exists():
            raise FileNotFoundError(
                f'{file}: pitch statistics for this configuration are not '
                'bundled')
        pitch_distribution.distribution = torch.from_numpy(np.load(file))
    return pitch_distribution.distribution.clone()


def audio(file, gpu=None):
    """Load mono audio at SAMPLE_RATE as (1, samples) float32
    (promonet/load.py:16-28: torchaudio.load + torchaudio.functional.resample
    + channel mean). torchaudio is not a dependency here: wav files are read
    with scipy, integer PCM is scaled by 2^(bits - 1) as torchaudio.load
    (normalize=True) does, and `resample` below restates torchaudio's
    windowed-sinc resampler (pinned against the published formula in
    tests/test_cpu_resample.py; parity with torchaudio itself is unpinned: it
    is not a dependency).

    With `gpu` the file is decoded on the host, uploaded at its native rate,
    resampled on the device (pm_resample) and then averaged over its channels,
    the reference's order; the result is a device tensor."""
    rate, data = decode(file)
    if gpu is None:
        data = resample(data, rate, promonet_amd.SAMPLE_RATE)
        return data.mean(dim=0, keepdim=True)
    device = torch.device(f'cuda:{gpu}')
    if int(rate) == promonet_amd.SAMPLE_RATE:
        # nothing to resample: the host mean, the bytes of the host path
        return data.mean(dim=0, keepdim=True).to(device)
    return mono(resample(data.to(device), rate, promonet_amd.SAMPLE_RATE))


def decode(file):
    """A wav file as (rate, (channels, samples) float32 CPU tensor); the
    tensor of a multi-channel file is a transposed view"""
    import scipy.io.wavfile
    rate, data = scipy.io.wavfile.read(file)
    if data.dtype.kind == 'i':
        data = data.astype(np.float32) / float(
            2 ** (8 * data.dtype.itemsize - 1))
    elif data.dtype.kind == 'u':
        data = (data.astype(np.float32) - 128.) / 128.
    data = torch.from_numpy(np.ascontiguousarray(data.astype(np.float32)))
    return rate, (data[None] if data.ndim == 1 else data.T)


def mono(channels):
    """The channel mean of resampled device audio (channels, samples) ->
    (1, samples). One function, one memory layout, for `audio` and the batched
    file loaders: their results are equal bit for bit."""
    return channels.contiguous().mean(dim=0, keepdim=True)


# Largest filter bank the device path uploads (floats). Every pair of
# standard rates stays under 0.3 M; a coprime pair such as 22 051 -> 22 050
# would need gigabytes.
RESAMPLE_BANK_MAX_FLOATS = 4 * 1024 * 1024


def resample_geometry(orig_freq, new_freq, lowpass_filter_width=6,
                      rolloff=.99):
    """(orig, new, width, base) of the polyphase bank: the rates over their
    gcd, the filter's half width in input samples and its cutoff"""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    gcd = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // gcd, new_freq // gcd
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    return orig, new, width, base


def resample_bank(orig_freq, new_freq, lowpass_filter_width=6, rolloff=.99,
                  max_floats=None):
    """The polyphase bank of torchaudio's 'sinc_interp_hann' resampler:
    (kernels float32 (new, 1, taps), orig, new, width), taps = 2 width +
    orig, built in float64. Output n = q new + p of the resampler is
    sum_k kernels[p, 0, k] x[q orig + k - width]. `max_floats` bounds
    new * taps (checked before anything is built)."""
    orig, new, width, base = resample_geometry(
        orig_freq, new_freq, lowpass_filter_width, rolloff)
    if max_floats is not None and new * (2 * width + orig) > max_floats:
        raise ValueError(
            f'resampling {int(orig_freq)} Hz -> {int(new_freq)} Hz needs a '
            f'bank of {new} filters x {2 * width + orig} taps = '
            f'{new * (2 * width + orig)} floats, above the limit of '
            f'{max_floats}: the rates share too small a divisor')
    index = torch.arange(
        -width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(
        0, -new, -1, dtype=torch.float64)[:, None, None] / new + index
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t)
    kernels = (kernels * window * (base / orig)).to(torch.float32)
    return kernels, orig, new, width


def resample_tile(orig_freq, new_freq, lowpass_filter_width=6, rolloff=.99):
    """Tile geometry of the device kernel for this rate pair, asked of the
    library (pm_resample_tile): (strides, outputs) = the input strides of
    `orig` samples and the strides * new output samples one workgroup takes.
    A sample's bits do not depend on it; tests place lengths around its
    edges."""
    orig, new, width, _ = resample_geometry(
        orig_freq, new_freq, lowpass_filter_width, rolloff)
    strides = promonet_amd._lib.lib().pm_resample_tile(orig, new, width)
    if strides < 0:
        promonet_amd._lib.check(strides)
    return strides, strides * new


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6,
             rolloff=.99, lengths=None):
    """torchaudio.functional.resample(waveform, orig_freq, new_freq) with its
    defaults ('sinc_interp_hann', lowpass_filter_width 6, rolloff 0.99):
    a polyphase bank of Hann-windowed sinc filters.

    A CPU tensor is filtered on the host by one strided conv1d. A device
    tensor (any strides, any floating type; cast to float32 as on the host)
    runs pm_resample on the current stream and stays on the device. The
    device bank is built and uploaded once per (rate pair, filter parameters,
    device); later calls copy nothing and can be captured in a graph.

    `lengths` (device path; a list or a tensor, one per flattened row) makes
    the batch ragged: row r is resampled as if it ended at lengths[r], the
    rest of its output row is zero, and (out, out_lengths) is returned with
    out_lengths = ceil(new lengths / orig), a list for a list and a tensor on
    the device of `lengths` otherwise. The lengths are never read back.
    (Equal rates return the input as it is, on either path.)"""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if waveform.is_cuda:
        return _resample_device(
            waveform, orig_freq, new_freq, lowpass_filter_width, rolloff,
            lengths)
    if lengths is not None:
        raise ValueError('lengths are supported for device tensors only')
    if orig_freq == new_freq:
        return waveform
    kernels, orig, new, width = resample_bank(
        orig_freq, new_freq, lowpass_filter_width, rolloff)
    shape = waveform.shape
    flat = waveform.reshape(-1, shape[-1]).to(torch.float32)
    length = flat.shape[-1]
    padded = torch.nn.functional.pad(flat, (width, width + orig))
    out = torch.nn.functional.conv1d(padded[:, None], kernels, stride=orig)
    out = out.transpose(1, 2).reshape(flat.shape[0], -1)
    target = int(math.ceil(new * length / orig))
    return out[..., :target].reshape(shape[:-1] + (target,))


_device_banks = {}


def _device_bank(orig_freq, new_freq, lowpass_filter_width, rolloff, device):
    """The transposed bank (taps, new) on `device`, uploaded once"""
    key = (orig_freq, new_freq, lowpass_filter_width, rolloff, str(device))
    if key not in _device_banks:
        kernels, orig, new, width = resample_bank(
            orig_freq, new_freq, lowpass_filter_width, rolloff,
            max_floats=RESAMPLE_BANK_MAX_FLOATS)
        _device_banks[key] = (
            kernels[:, 0].T.contiguous().to(device), orig, new, width)
    return _device_banks[key]


def _resample_device(waveform, orig_freq, new_freq, lowpass_filter_width,
                     rolloff, lengths):
    _lib = promonet_amd._lib
    shape = waveform.shape
    device = waveform.device
    samples = shape[-1]
    rows = math.prod(shape[:-1])
    flat = waveform.reshape(rows, samples).to(torch.float32)
    as_list = isinstance(lengths, (list, tuple))
    if lengths is not None:
        if as_list:
            lengths = torch.tensor(lengths, dtype=torch.int32)
        if lengths.numel() != rows:
            raise ValueError(
                f'{lengths.numel()} lengths for {rows} rows of audio')
        lengths = lengths.reshape(-1)
    if orig_freq == new_freq:
        out, orig, new = waveform, 1, 1
    else:
        bank, orig, new, width = _device_bank(
            orig_freq, new_freq, lowpass_filter_width, rolloff, device)
        target = (new * samples + orig - 1) // orig
        out = torch.empty(rows, target, dtype=torch.float32, device=device)
        if rows > 0 and target > 0:
            if flat.stride(1) != 1 or (rows > 1 and flat.stride(0) < samples):
                flat = flat.contiguous()
            device_lengths = None
            if lengths is not None:
                device_lengths = lengths.to(
                    device=device, dtype=torch.int32).contiguous()
            with torch.cuda.device(device):
                _lib.check(_lib.lib().pm_resample(
                    flat.data_ptr(),
                    _lib.ptr(device_lengths, torch.int32),
                    _lib.ptr(bank),
                    out.data_ptr(),
                    rows, samples, flat.stride(0) if rows > 1 else samples,
                    orig, new, width, target, target, _lib.stream()))
        out = out.reshape(shape[:-1] + (target,))
    if lengths is None:
        return out
    if as_list:
        out_lengths = [
            (new * min(max(int(item), 0), samples) + orig - 1) // orig
            for item in lengths.tolist()]
    else:
        out_lengths = (
            lengths.clamp(0, samples).to(torch.int64) * new + orig - 1
        ).div(orig, rounding_mode='floor')
    return out, out_lengths


def ppg(file, resample_length=None):
    """Load a PPG (40, T') and linearly resample to `resample_length` frames
    (promonet/load.py:172-188 delegates to ppgs.edit.grid; restated as
    align-corners-free linear interpolation on the frame grid)."""
    result = torch.load(file)
    if resample_length is not None and result.shape[-1] != resample_length:
        source = result.shape[-1]
        grid = torch.linspace(0., source - 1., resample_length)
        below = grid.floor().long().clamp(0, source - 1)
        above = (below + 1).clamp(0, source - 1)
        weight = (grid - below).to(result.dtype)
        result = (
            result[..., below] * (1 - weight) + result[..., above] * weight)
    return result


def features(prefix):
    """promonet/load.py:31-41"""
    viterbi = '-viterbi' if promonet_amd.VITERBI_DECODE_PITCH else ''
    return (
        torch.load(f'{prefix}-loudness.pt'),
        torch.load(f'{prefix}{viterbi}-pitch.pt'),
        torch.load(f'{prefix}{viterbi}-periodicity.pt'),
        torch.load(f'{prefix}-ppg.pt'))

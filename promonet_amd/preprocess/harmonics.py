"""Speech harmonic contours on the device.

API of `promonet.preprocess.harmonics` (promonet/preprocess/harmonics.py),
its default path: `features='stft'` and the 'viterbi' (or 'peak') decoder. A
high-pass biquad, a 4096-point STFT magnitude, one softmax and one Viterbi
decode per harmonic; every stage is a HIP kernel (pm_harmonics.h,
pm_viterbi.h). `features='lpc'` needs librosa and `'posteriorgram'` needs
penn: they raise.

Beyond the reference: `audio` may be a batch (B, samples), ragged with
`lengths=`; each row then equals its stand-alone call bit for bit.

Where this differs from the reference, on purpose:
- audio at another `sample_rate` is resampled to SAMPLE_RATE first
  (promonet_amd.load.resample) and filtered there; the reference filters at
  the original rate;
- a frame whose mask is empty or whose f0 is NaN gives NaN in the
  reference's softmax and an undefined path. Here its observation is a row
  of zeros (log-probabilities: it adds nothing to any path) and its output
  is NaN for that harmonic. Frames past a row's end are NaN too.
Parity with torchaudio (the biquad) and torbi (the decoder) is unpinned:
neither is a dependency. tests/harmonics_oracle.py restates both.
"""
import math

import torch

import promonet_amd
from promonet_amd import _lib

NUM_FFT = 4096
HARMONIC_WIDTH_RATIO = .8


###############################################################################
# Extract harmonics
###############################################################################


def from_audio(
    audio,
    sample_rate=None,
    pitch=None,
    features='stft',
    decoder='viterbi',
    max_harmonics=None,
    return_features=False,
    gpu=None,
    lengths=None,
    _debug=False
):
    """Compute speech harmonic contours (harmonics.py:20-77)

    Arguments
        audio
            shape=(1, samples) or (batch, samples)
        sample_rate
            The audio sampling rate; default SAMPLE_RATE
        pitch
            Optional pitch contour prior: (1, frames) / (frames,), or
            (batch, frames). It becomes harmonic 0.
        features
            'stft'. ('lpc' and 'posteriorgram' raise.)
        decoder
            One of ['peak', 'viterbi']
        max_harmonics
            The number of harmonics to compute; default MAX_HARMONICS
        return_features
            Whether to return the features used for analysis
        gpu
            The GPU index; None: the device of `audio`
        lengths
            Samples of each row of a ragged batch (list or tensor)

    Returns
        Speech harmonics, a device tensor; NaN where there are fewer
        shape=(max_harmonics, frames), or (batch, max_harmonics, frames) for
        batch > 1 or with `lengths`. With return_features also the features
        (states, frames) / (batch, states, frames).
    """
    if features == 'lpc':
        raise ValueError(
            "features='lpc' needs the third-party `librosa` package: only "
            "'stft' runs here")
    if features == 'posteriorgram':
        raise ValueError(
            "features='posteriorgram' needs the third-party `penn` package: "
            "only 'stft' runs here")
    if features != 'stft':
        raise ValueError(f'unknown features {features!r}')
    if decoder not in ('peak', 'viterbi'):
        raise ValueError(f'unknown decoder {decoder!r}')
    if max_harmonics is None:
        max_harmonics = promonet_amd.MAX_HARMONICS
    audio = _on_device(audio, gpu)
    if audio.ndim != 2:
        raise ValueError(
            f'audio must be (batch, samples), got {tuple(audio.shape)}')
    single = audio.shape[0] == 1 and lengths is None
    frames, frequencies, counts = stft(
        audio, sample_rate, lengths=lengths, _counts=True)
    if decoder == 'peak':
        harmonics = peak_pick(
            frames, frequencies, max_harmonics, lengths=counts)
        debug = {}
    else:
        if pitch is not None:
            pitch = _on_device(pitch, audio.device.index).to(torch.float32)
            pitch = pitch.reshape(-1, pitch.shape[-1])
        harmonics, debug = viterbi(
            frames, frequencies, pitch=pitch, max_harmonics=max_harmonics,
            lengths=counts, _debug=True)
    result = (harmonics[0] if single else harmonics,)
    if return_features:
        transposed = frames.transpose(1, 2)
        result += (transposed[0] if single else transposed,)
    if _debug:
        debug.update(frames=frames, frequencies=frequencies, counts=counts)
        result += (debug,)
    return result[0] if len(result) == 1 else result


def from_file(
    file,
    pitch_file=None,
    max_harmonics=None,
    return_features=False,
    gpu=None
):
    """Compute speech harmonic contours from audio file
    (harmonics.py:80-112)"""
    pitch = None if pitch_file is None else torch.load(pitch_file)
    return from_audio(
        promonet_amd.load.audio(file, gpu=gpu),
        pitch=pitch,
        max_harmonics=max_harmonics,
        return_features=return_features,
        gpu=gpu)


def from_file_to_file(
    file,
    output_file,
    pitch_file=None,
    output_feature_file=None,
    max_harmonics=None,
    gpu=None
):
    """Compute speech harmonic contours from audio file and save
    (harmonics.py:115-148)"""
    result = from_file(
        file,
        pitch_file=pitch_file,
        max_harmonics=max_harmonics,
        return_features=output_feature_file is not None,
        gpu=gpu)
    if output_feature_file is not None:
        torch.save(result[-1].cpu(), output_feature_file)
        result = result[0]
    torch.save(result.cpu(), output_file)


def from_files_to_files(
    files,
    output_files,
    pitch_files=None,
    output_feature_files=None,
    max_harmonics=None,
    gpu=None
):
    """Compute speech harmonic contours from audio files and save
    (harmonics.py:151-191)"""
    if pitch_files is None:
        pitch_files = [None] * len(files)
    if output_feature_files is None:
        output_feature_files = [None] * len(files)
    for file, output_file, pitch_file, output_feature_file in zip(
        files,
        output_files,
        pitch_files,
        output_feature_files
    ):
        from_file_to_file(
            file,
            output_file,
            pitch_file,
            output_feature_file,
            max_harmonics,
            gpu=gpu)


###############################################################################
# Decode
###############################################################################


def peak_pick(frames, frequencies, max_harmonics=None, lengths=None):
    """Decode harmonics via peak-picking (harmonics.py:199-212): per frame
    the first `max_harmonics` peaks of scipy.signal.find_peaks (no
    conditions) in ascending order, NaN beyond them. frames (T, S) ->
    (max_harmonics, T); (B, T, S) -> (B, max_harmonics, T). One kernel."""
    if max_harmonics is None:
        max_harmonics = promonet_amd.MAX_HARMONICS
    _lib.require_gpu(frames)
    single = frames.ndim == 2
    x = (frames[None] if single else frames).to(torch.float32).contiguous()
    device = x.device
    batch, count, states = x.shape
    frequencies = frequencies.to(device=device, dtype=torch.float32)
    out = torch.full(
        (batch, max_harmonics, count), float('nan'), device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_harmonics_peaks(
            _lib.ptr(x), _lib.ptr(frequencies.contiguous()),
            _lib.ptr(_row_counts(lengths, batch, device), torch.int32),
            _lib.ptr(out), batch, count, states, max_harmonics,
            _lib.stream()))
    return out[0] if single else out


def viterbi(
    frames,
    frequencies,
    pitch=None,
    max_harmonics=None,
    harmonic_width_ratio=HARMONIC_WIDTH_RATIO,
    gpu=None,
    lengths=None,
    _debug=False
):
    """Decode harmonics via Viterbi decoding (harmonics.py:215-297), one
    `promonet_amd.viterbi` decode per harmonic. frames (T, S) ->
    (max_harmonics, T); (B, T, S), ragged with `lengths` (frames of each
    row) -> (B, max_harmonics, T)."""
    if max_harmonics is None:
        max_harmonics = promonet_amd.MAX_HARMONICS
    frames = _on_device(frames, gpu)
    single = frames.ndim == 2
    x = (frames[None] if single else frames).to(torch.float32).contiguous()
    device = x.device
    batch, count, states = x.shape
    frequencies = frequencies.to(device=device, dtype=torch.float32)
    frequencies = frequencies.contiguous()
    transition, initial = decoder_model(frequencies)
    counts = _row_counts(lengths, batch, device)

    harmonics = torch.full(
        (batch, max_harmonics, count), float('nan'), device=device)
    debug = {
        'transition': transition, 'initial': initial, 'observations': [],
        'indices': [], 'valid': []}
    i = 0
    observed = None
    if pitch is not None:
        # Use the external pitch estimate for F0 (:248-264)
        pitch = pitch.to(device=device, dtype=torch.float32)
        harmonics[:, 0] = pitch.reshape(batch, count)
        i = 1
        if i < max_harmonics:
            observed = observation(
                x, frequencies, harmonics[:, 0].contiguous(),
                1. + harmonic_width_ratio, 1. + 1. / harmonic_width_ratio,
                counts)
    else:
        observed = observation(x, frequencies, lengths=counts)

    # Iteratively decode F1, F2, ... (:267-295)
    while i < max_harmonics:
        log_observation, valid = observed
        indices = promonet_amd.viterbi.from_probabilities(
            log_observation,
            batch_frames=counts,
            transition=transition,
            initial=initial,
            log_probs=True)
        harmonics[:, i] = torch.where(
            valid, frequencies[indices.to(torch.long)], float('nan'))
        if _debug:
            debug['observations'].append(log_observation)
            debug['indices'].append(indices)
            debug['valid'].append(valid)
        i += 1
        if i == max_harmonics:
            break
        observed = observation(
            x, frequencies, harmonics[:, 0].contiguous(),
            i + harmonic_width_ratio, i + 1. / harmonic_width_ratio, counts)
    harmonics = harmonics[0] if single else harmonics
    return (harmonics, debug) if _debug else harmonics


_models = {}


def decoder_model(frequencies):
    """(Transition, log initial) of harmonics.py:232-243 for these
    frequencies, built on their device with the reference's expressions and
    packed once per tensor"""
    key = (frequencies.data_ptr(), frequencies._version, frequencies.numel(),
           str(frequencies.device))
    entry = _models.get(key)
    if entry is not None and entry[0] is frequencies:
        return entry[1], entry[2]
    device = frequencies.device
    logfreq = torch.log2(frequencies)
    transition = 1. - 3.5 * torch.cdist(
        logfreq[None, :, None],
        logfreq[None, :, None],
        p=1.0
    )[0]
    transition[transition < 0.] = 0.
    transition /= transition.sum(dim=1)
    initial = torch.linspace(1., 0., len(logfreq), device=device)
    initial /= initial.sum()
    packed = promonet_amd.viterbi.Transition(transition)
    if len(_models) >= 4:
        _models.pop(next(iter(_models)))
    _models[key] = (frequencies, packed, torch.log(initial))
    return packed, _models[key][2]


def observation(frames, frequencies, f0=None, low=0., high=0., lengths=None):
    """One decode round's observation as log-probabilities, and the frames
    it is defined on: (log softmax (B, T, S), valid bool (B, T)). f0 None:
    round 0, log softmax(x + 0.5 arange(S, 0, -1)) (:228-229). Else every
    frame is masked to [searchsorted(frequencies, f0 low),
    searchsorted(frequencies, f0 high)) first (:252-264, :285-295); `low` and
    `high` are rounded to fp32 before the product, as torch rounds a Python
    scalar."""
    _lib.require_gpu(frames)
    device = frames.device
    batch, count, states = frames.shape
    out = torch.empty_like(frames)
    valid = torch.empty(batch, count, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_harmonics_observation(
            _lib.ptr(frames), _lib.ptr(f0), _lib.ptr(frequencies),
            _lib.ptr(_row_counts(lengths, batch, device), torch.int32),
            _lib.ptr(out),
            _lib.ptr(valid, torch.int32), batch, count, states,
            float(low), float(high), _lib.stream()))
    return out, valid.bool()


###############################################################################
# Preprocess
###############################################################################


def highpass_coefficients(sample_rate, cutoff, q=.707):
    """torchaudio.functional.highpass_biquad's coefficients (the RBJ
    cookbook high-pass), in float64 and normalised by a0:
    (b0, b1, b2, a1, a2)"""
    w0 = 2. * math.pi * cutoff / sample_rate
    alpha = math.sin(w0) / 2. / q
    b0 = (1. + math.cos(w0)) / 2.
    b1 = -1. - math.cos(w0)
    b2 = b0
    a0 = 1. + alpha
    a1 = -2. * math.cos(w0)
    a2 = 1. - alpha
    return b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0


def highpass(audio, sample_rate, cutoff, lengths=None):
    """torchaudio.functional.highpass_biquad(audio, sample_rate, cutoff)
    (Q = 0.707, clamped to [-1, 1] once at the end as lfilter does) of the
    rows of a device tensor (B, samples); zeros past a row's length."""
    _lib.require_gpu(audio)
    x = audio.to(torch.float32).contiguous()
    device = x.device
    rows, samples = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_harmonics_highpass(
            _lib.ptr(x), _lib.ptr(_row_counts(lengths, rows, device),
                                  torch.int32),
            _lib.ptr(out), rows, samples, samples, samples,
            *highpass_coefficients(sample_rate, cutoff), _lib.stream()))
    return out


_tables = {}


def _stft_tables(target_rate, fmin, device):
    """(frequencies, first bin, window, twiddle) on `device`, built once"""
    key = (target_rate, float(fmin), str(device))
    if key not in _tables:
        # STFT frequencies, cropped below fmin (:420-428)
        frequencies = torch.abs(torch.fft.fftfreq(
            NUM_FFT,
            1 / target_rate
        )[:NUM_FFT // 2 + 1])
        minidx = int(torch.searchsorted(frequencies, torch.tensor(fmin)))
        angle = 2. * math.pi * torch.arange(
            NUM_FFT // 2, dtype=torch.float64) / NUM_FFT
        twiddle = torch.stack([angle.cos(), -angle.sin()], dim=1)
        _tables[key] = (
            frequencies[minidx:].to(torch.float32).contiguous().to(device),
            minidx,
            torch.hann_window(NUM_FFT, dtype=torch.float32).to(device),
            twiddle.to(torch.float32).contiguous().to(device))
    return _tables[key]


def magnitude(audio, lengths, target_rate, fmin, frame_counts=None):
    """STFT magnitude of high-passed device audio (B, samples) at
    `target_rate` (:390-428): reflect padding, Hann window over 4096,
    center=False, sqrt(re^2 + im^2 + 1e-6), bins below fmin dropped.
    lengths: host list of each row's samples; frame_counts: the frames the
    reference expects of each row (samples at SAMPLE_RATE // HOPSIZE;
    default lengths // hop). Returns (frames (B, T, S), frequencies (S),
    row frame counts, device int32)."""
    device = audio.device
    rows, samples = audio.shape
    frequencies, minidx, window, twiddle = _stft_tables(
        target_rate, fmin, device)
    hopsize = int(
        promonet_amd.HOPSIZE * target_rate / promonet_amd.SAMPLE_RATE)
    if hopsize < 1:
        raise ValueError(f'no hop at {target_rate} Hz')
    geometry = []
    for row, length in enumerate(lengths):
        expected = (
            length // hopsize if frame_counts is None else frame_counts[row])
        size = (
            hopsize * (expected - (length // hopsize)) // 2 +
            (NUM_FFT - promonet_amd.HOPSIZE) // 2)
        if size < 0 or length <= size:
            raise ValueError(
                f'audio of {length} samples is too short: the reflect '
                f'padding of {size} samples a side needs at least '
                f'{max(size, 0) + 1}')
        count = max(0, 1 + (length + 2 * size - NUM_FFT) // hopsize)
        geometry.append([length, count, size])
    most = max(item[1] for item in geometry)
    states = NUM_FFT // 2 + 1 - minidx
    out = torch.empty(rows, most, states, device=device)
    geometry = torch.tensor(geometry, dtype=torch.int32).to(device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_harmonics_stft(
            _lib.ptr(audio), _lib.ptr(geometry, torch.int32),
            _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(out), rows,
            samples, most, states, minidx, hopsize, _lib.stream()))
    return out, frequencies, geometry[:, 1].contiguous()


def stft(
    audio,
    sample_rate=None,
    fmin=None,
    fmax=None,
    gpu=None,
    lengths=None,
    _counts=False
):
    """Compute short-time Fourier transform (harmonics.py:363-428): the
    high-pass at 1.33 fmin, the resampling to 2 fmax (the identity at the
    default fmax = SAMPLE_RATE // 2) and the magnitude of a 4096-point STFT
    above fmin. audio (1, samples) -> (frames (T, S), frequencies (S));
    (B, samples), ragged with `lengths` -> frames (B, T, S)."""
    sample_rate = int(sample_rate or promonet_amd.SAMPLE_RATE)
    fmin = promonet_amd.FMIN if fmin is None else fmin
    fmax = promonet_amd.SAMPLE_RATE // 2 if fmax is None else fmax
    audio = _on_device(audio, gpu).to(torch.float32)
    if audio.ndim != 2:
        raise ValueError(
            f'audio must be (batch, samples), got {tuple(audio.shape)}')
    single = audio.shape[0] == 1 and lengths is None
    rows = audio.shape[0]
    if lengths is None:
        lengths = [audio.shape[-1]] * rows
    elif isinstance(lengths, torch.Tensor):
        lengths = [int(item) for item in lengths.tolist()]
    else:
        lengths = [int(item) for item in lengths]
    if len(lengths) != rows:
        raise ValueError(f'{len(lengths)} lengths for {rows} rows of audio')
    lengths = [min(max(item, 0), audio.shape[-1]) for item in lengths]

    # Everything below runs at SAMPLE_RATE
    if sample_rate != promonet_amd.SAMPLE_RATE:
        audio, lengths = promonet_amd.load.resample(
            audio, sample_rate, promonet_amd.SAMPLE_RATE, lengths=lengths)
    padding = (NUM_FFT - promonet_amd.HOPSIZE) // 2
    for length in lengths:
        if length <= padding:
            raise ValueError(
                f'audio of {length} samples is too short for harmonic '
                f'analysis: the reflect padding needs at least '
                f'{padding + 1}')
    expected = [promonet_amd.convert.samples_to_frames(item)
                for item in lengths]

    # High-pass filter to remove low frequencies (:378-381)
    audio = highpass(
        audio, promonet_amd.SAMPLE_RATE, 1.33 * fmin, lengths=lengths)

    # Resample to remove upper harmonics (:383-388)
    target_rate = int(2 * fmax)
    if target_rate != promonet_amd.SAMPLE_RATE:
        audio, lengths = promonet_amd.load.resample(
            audio, promonet_amd.SAMPLE_RATE, target_rate, lengths=lengths)
        audio = audio.contiguous()

    frames, frequencies, counts = magnitude(
        audio, lengths, target_rate, fmin, expected)
    if _counts:
        return frames, frequencies, counts
    return (frames[0] if single else frames), frequencies


###############################################################################
# Utilities
###############################################################################


def _on_device(tensor, gpu):
    """`tensor` on cuda:`gpu`; with gpu None it must be there already"""
    if gpu is not None:
        return tensor.to(torch.device(f'cuda:{gpu}'))
    _lib.require_gpu(tensor)
    return tensor


def _row_counts(lengths, rows, device):
    """Per-row counts as a device int32 tensor, or None"""
    if lengths is None:
        return None
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.tensor(list(lengths), dtype=torch.int32)
    if lengths.numel() != rows:
        raise ValueError(f'{lengths.numel()} lengths for {rows} rows')
    return lengths.reshape(-1).to(
        device=device, dtype=torch.int32).contiguous()

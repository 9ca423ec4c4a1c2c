"""Speech harmonic contours on the device.

API of `promonet.preprocess.harmonics` (promonet/preprocess/harmonics.py):
`features='stft'` (the default) or `'lpc'`, and the 'viterbi' (or 'peak')
decoder. 'stft': a high-pass biquad, a 4096-point STFT magnitude, one softmax
and one Viterbi decode per harmonic. 'lpc' (`lpc_coefficients`, :305-330):
Hamming-windowed 1024-sample frames, Burg's order-24 predictor and log10 of
the all-pole response at 512 frequencies, one kernel, one wave a frame: the
spectral envelope, whose peaks are the formants. Every stage is a HIP kernel
(pm_harmonics.h, pm_lpc.h, pm_viterbi.h). `'posteriorgram'` needs penn: it
raises; so does 'lpc' for a tensor that is not on a device (the reference's
host path needs librosa).

Beyond the reference: `audio` may be a batch (B, samples), ragged with
`lengths=`; each row then equals its stand-alone call bit for bit.

Where this differs from the reference, on purpose:
- audio at another `sample_rate` is resampled to SAMPLE_RATE first
  (promonet_amd.load.resample) and filtered there; the reference filters at
  the original rate;
- a frame whose mask is empty or whose f0 is NaN gives NaN in the
  reference's softmax and an undefined path. Here its observation is a row
  of zeros (log-probabilities: it adds nothing to any path) and its output
  is NaN for that harmonic. Frames past a row's end are NaN too;
- 'lpc' with the 'viterbi' decoder decodes bins 1 to 511 only. The
  reference's frequencies start at 0 Hz, log2 gives -inf, cdist gives NaN at
  [0, 0] and the column-wise normalisation spreads it over all of column 0:
  its decoder's transition matrix holds NaN and the path is undefined.
  Without bin 0 the matrix is finite (band of at most 167 of 511 states).
  The 'peak' decoder and `return_features` keep all 512 bins: bin 0 can
  never be a peak;
- Burg's denominator is recomputed as sum(f^2 + b^2) at every order, not
  updated as librosa does: equal in exact arithmetic, and the update cancels
  in fp32. The target is the float64 recursion.
Parity with torchaudio (the biquad), torbi (the decoder) and librosa (Burg's
recursion, `librosa.lpc`) is unpinned: none is a dependency.
tests/harmonics_oracle.py and tests/lpc_oracle.py restate them from their
published behaviour.
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
            'stft' or 'lpc'. ('posteriorgram' raises; so does 'lpc' for a
            tensor that is not on a device when `gpu` is None.)
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
    if features == 'lpc' and gpu is None and \
            isinstance(audio, torch.Tensor) and not audio.is_cuda:
        raise ValueError(
            "features='lpc' on the CPU needs the third-party `librosa` "
            "package; pass a device tensor or gpu=")
    if features == 'posteriorgram':
        raise ValueError(
            "features='posteriorgram' needs the third-party `penn` package: "
            "only 'stft' and 'lpc' run here")
    if features not in ('stft', 'lpc'):
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
    if features == 'lpc':
        frames, frequencies, counts = lpc_coefficients(
            audio, sample_rate, lengths=lengths, _counts=True)
    else:
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
        decoded, states = frames, frequencies
        if features == 'lpc':
            # 0 Hz makes the decoder's transition matrix NaN: see above
            decoded = frames[..., 1:]
            states = _lpc_tables(frames.device)[1]
        harmonics, debug = viterbi(
            decoded, states, pitch=pitch, max_harmonics=max_harmonics,
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
    gpu=None,
    features='stft'
):
    """Compute speech harmonic contours from audio file
    (harmonics.py:80-112)"""
    pitch = None if pitch_file is None else torch.load(pitch_file)
    return from_audio(
        promonet_amd.load.audio(file, gpu=gpu),
        pitch=pitch,
        features=features,
        max_harmonics=max_harmonics,
        return_features=return_features,
        gpu=gpu)


def from_file_to_file(
    file,
    output_file,
    pitch_file=None,
    output_feature_file=None,
    max_harmonics=None,
    gpu=None,
    features='stft'
):
    """Compute speech harmonic contours from audio file and save
    (harmonics.py:115-148)"""
    result = from_file(
        file,
        pitch_file=pitch_file,
        max_harmonics=max_harmonics,
        return_features=output_feature_file is not None,
        gpu=gpu,
        features=features)
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


LPC_BINS = 512

_lpc = {}


def _lpc_tables(device):
    """(frequencies (512), frequencies[1:], Hamming window (1024), table
    (1024, 4) = the float64 (cos, sin)(2 pi m / 1024) as float heads and
    float tails) on `device`, built once"""
    key = str(device)
    if key not in _lpc:
        # Real FFT frequencies in Hz (:320-322): spaced rate / 1023
        frequencies = promonet_amd.SAMPLE_RATE * torch.linspace(
            0., 1., promonet_amd.NUM_FFT)
        frequencies = frequencies[0:len(frequencies) // 2]
        angle = 2. * math.pi * torch.arange(
            promonet_amd.WINDOW_SIZE, dtype=torch.float64
        ) / promonet_amd.WINDOW_SIZE
        exact = torch.stack([angle.cos(), angle.sin()], dim=1)
        head = exact.to(torch.float32)
        tail = (exact - head.to(torch.float64)).to(torch.float32)
        table = torch.cat([head, tail], dim=1)
        _lpc[key] = (
            frequencies.contiguous().to(device),
            frequencies[1:].contiguous().to(device),
            torch.hamming_window(
                promonet_amd.WINDOW_SIZE, dtype=torch.float32).to(device),
            table.contiguous().to(device))
    return _lpc[key]


def lpc_frames(samples):
    """Frames of `samples` samples (an int or an integer tensor): the unfold
    of the zero-padded audio (:307-315)"""
    padding = promonet_amd.WINDOW_SIZE - promonet_amd.HOPSIZE
    if isinstance(samples, torch.Tensor):
        count = (samples + (padding - promonet_amd.WINDOW_SIZE)).div(
            promonet_amd.HOPSIZE, rounding_mode='floor') + 1
        return count.clamp(min=0)
    return max(
        0,
        (samples + padding - promonet_amd.WINDOW_SIZE) // promonet_amd.HOPSIZE
        + 1)


def lpc(audio, lengths=None, order=None, return_coefficients=False):
    """One launch of pm_harmonics_lpc on device audio (B, samples) at
    SAMPLE_RATE: log10 |H| (B, T, 512) of Burg's predictor of `order`
    (default SAMPLE_RATE / 1000 + 2 = 24) of every Hamming-windowed frame,
    T = lpc_frames(samples), and with return_coefficients the predictors
    (B, T, order + 1). lengths: device int32 (B) or None; it is read on the
    device only, frames past a row's count are zeros, and the launch can be
    captured in a graph."""
    _lib.require_gpu(audio)
    if audio.ndim != 2:
        raise ValueError(
            f'audio must be (batch, samples), got {tuple(audio.shape)}')
    if order is None:
        order = int(promonet_amd.SAMPLE_RATE / 1000 + 2)
    x = audio.to(torch.float32)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    device = x.device
    rows, samples = x.shape
    if lengths is not None and lengths.numel() != rows:
        raise ValueError(f'{lengths.numel()} lengths for {rows} rows')
    count = lpc_frames(samples)
    _, _, window, table = _lpc_tables(device)
    out = torch.empty(rows, count, LPC_BINS, device=device)
    coefficients = None
    if return_coefficients:
        coefficients = torch.empty(rows, count, order + 1, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_harmonics_lpc(
            x.data_ptr(), _lib.ptr(lengths, torch.int32), _lib.ptr(window),
            _lib.ptr(table), _lib.ptr(out), _lib.ptr(coefficients), rows,
            x.stride(0) if rows > 1 else samples, samples, count, order,
            _lib.stream()))
    return (out, coefficients) if return_coefficients else out


def lpc_coefficients(
    audio,
    sample_rate=None,
    lengths=None,
    gpu=None,
    return_coefficients=False,
    _counts=False
):
    """Compute linear predictive coding features (harmonics.py:305-330):
    log10 of the all-pole response of Burg's order-24 predictor of every
    frame, and the frequencies (512,) it is evaluated at. audio (1, samples)
    -> frames (T, 512); (B, samples), or ragged with `lengths` (a list or a
    tensor, samples of each row, never read back) -> (B, T, 512), zeros past
    a row's frames. Audio at another `sample_rate` is resampled to
    SAMPLE_RATE first, this module's convention: the order is always 24.
    With return_coefficients also the predictors (..., T, 25). Burg's
    recursion restates librosa.lpc; parity with librosa is unpinned."""
    sample_rate = int(sample_rate or promonet_amd.SAMPLE_RATE)
    audio = _on_device(audio, gpu).to(torch.float32)
    if audio.ndim != 2:
        raise ValueError(
            f'audio must be (batch, samples), got {tuple(audio.shape)}')
    device = audio.device
    rows = audio.shape[0]
    single = rows == 1 and lengths is None
    if lengths is not None:
        lengths = _row_counts(lengths, rows, device)
    if sample_rate != promonet_amd.SAMPLE_RATE:
        if lengths is None:
            audio = promonet_amd.load.resample(
                audio, sample_rate, promonet_amd.SAMPLE_RATE)
        else:
            audio, lengths = promonet_amd.load.resample(
                audio, sample_rate, promonet_amd.SAMPLE_RATE, lengths=lengths)
            lengths = lengths.to(torch.int32)
    result = lpc(audio, lengths, return_coefficients=return_coefficients)
    frames, coefficients = result if return_coefficients else (result, None)
    frequencies = _lpc_tables(device)[0]
    if _counts:
        samples = audio.shape[-1]
        if lengths is None:
            counts = torch.full(
                (rows,), lpc_frames(samples), dtype=torch.int32, device=device)
        else:
            counts = lpc_frames(lengths.clamp(0, samples)).to(torch.int32)
        return frames, frequencies, counts
    if single:
        frames = frames[0]
        coefficients = coefficients[0] if return_coefficients else None
    if return_coefficients:
        return frames, frequencies, coefficients
    return frames, frequencies


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

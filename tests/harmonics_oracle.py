"""CPU restatement of promonet/preprocess/harmonics.py's default path
(features='stft', decoder='viterbi' or 'peak') and of the decoder it calls.
Not a test: the oracle of test_cpu_harmonics.py, test_gpu_viterbi.py and
test_gpu_harmonics.py. It shares no code with promonet_amd.

torchaudio (the biquad) and torbi (the decoder) are not dependencies: both
are restated from their published behaviour, parity unpinned.
"""
import itertools
import math

import numpy as np
import torch

SAMPLE_RATE = 22050
HOPSIZE = 256
FMIN = 50.
NUM_FFT = 4096
BIN = SAMPLE_RATE / NUM_FFT


###############################################################################
# High-pass (harmonics.py:378-381: torchaudio.functional.highpass_biquad)
###############################################################################


def highpass_coefficients(sample_rate=SAMPLE_RATE, cutoff=1.33 * FMIN,
                          q=.707):
    """The RBJ high-pass of torchaudio.functional.highpass_biquad, float64,
    normalised by a0 as torchaudio.functional.biquad does"""
    w0 = 2 * math.pi * cutoff / sample_rate
    alpha = math.sin(w0) / 2 / q
    b0 = (1 + math.cos(w0)) / 2
    b1 = -1 - math.cos(w0)
    b2 = b0
    a0 = 1 + alpha
    a1 = -2 * math.cos(w0)
    a2 = 1 - alpha
    return np.array([b0, b1, b2, a1, a2], dtype=np.float64) / a0


def biquad(x, coefficients=None, dtype=np.float64, clamp=True):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] of a
    1-D array, every product and sum rounded to `dtype`, in that order;
    clamped to [-1, 1] once at the end (torchaudio.functional.lfilter's
    default)"""
    if coefficients is None:
        coefficients = highpass_coefficients()
    b0, b1, b2, a1, a2 = (dtype(c) for c in coefficients)
    x = np.asarray(x).astype(dtype)
    y = np.zeros(len(x), dtype=dtype)
    x1 = x2 = y1 = y2 = dtype(0)
    for n in range(len(x)):
        x0 = x[n]
        y0 = b0 * x0 + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        y[n] = y0
        x2, x1, y2, y1 = x1, x0, y1, y0
    return np.clip(y, -1, 1) if clamp else y


###############################################################################
# STFT (harmonics.py:390-428)
###############################################################################


def frequencies():
    """(frequencies above FMIN float32, first bin) (:420-428)"""
    result = torch.abs(torch.fft.fftfreq(
        NUM_FFT, 1 / SAMPLE_RATE)[:NUM_FFT // 2 + 1])
    minidx = int(torch.searchsorted(result, torch.tensor(FMIN)))
    return result[minidx:], minidx


def stft(filtered):
    """float64 magnitudes (frames, states) of high-passed audio (samples,)
    at SAMPLE_RATE, and per frame sum_n |w_n x_n| (the scale of a
    transform's rounding error)"""
    audio = torch.as_tensor(filtered, dtype=torch.float64)[None]
    frames = audio.shape[-1] // HOPSIZE
    size = (
        HOPSIZE * (frames - (audio.shape[-1] // HOPSIZE)) // 2 +
        (NUM_FFT - HOPSIZE) // 2)
    audio = torch.nn.functional.pad(audio[None], (size, size), 'reflect')[0]
    window = torch.hann_window(NUM_FFT, dtype=torch.float64)
    result = torch.stft(
        audio,
        NUM_FFT,
        hop_length=HOPSIZE,
        window=window,
        center=False,
        normalized=False,
        onesided=True,
        return_complex=True)
    result = torch.view_as_real(result)
    spectrogram = torch.sqrt(result.pow(2).sum(-1) + 1e-6)
    _, minidx = frequencies()
    scale = (audio[0].unfold(0, NUM_FFT, HOPSIZE) * window).abs().sum(-1)
    return spectrogram[0][minidx:].T.contiguous(), scale


###############################################################################
# Observation (harmonics.py:228-229, :252-264, :285-295)
###############################################################################


def observation(frames, freqs, f0=None, low=None, high=None,
                dtype=torch.float32):
    """(log softmax (T, S) in `dtype`, valid (T,)) of one decode round.
    f0 None: round 0 with its bias. The mask indices always come from the
    fp32 product, as in the reference. A frame whose mask is empty or whose
    f0 is NaN is all zeros and not valid (the defined deviation)."""
    x = frames.to(dtype)
    count, states = x.shape
    valid = torch.ones(count, dtype=torch.bool)
    if f0 is None:
        x = x + (.5 * torch.arange(states, 0, -1)).to(dtype)
    else:
        f0 = f0.to(torch.float32)
        lo = torch.searchsorted(freqs, f0 * low)
        hi = torch.searchsorted(freqs, f0 * high)
        index = torch.arange(states)[None]
        inside = (index >= lo[:, None]) & (index < hi[:, None])
        x = torch.where(inside, x, -float('inf'))
        valid = (lo < hi) & ~torch.isnan(f0)
        x[~valid] = 0.
    result = torch.log(torch.softmax(x, dim=1))
    result[~valid] = 0.
    return result, valid


###############################################################################
# Viterbi (the decoder of harmonics.py:270-276)
###############################################################################


def viterbi(observation, transition, initial, length=None):
    """Indices (T,) int32 of the best path through fp32 log-probabilities
    observation (T, S), transition (S, S) [next, previous], initial (S);
    zeros from `length` on. One fp32 add per sum, d + A first, then + B.
    numpy.argmax returns the FIRST maximum (documented), also among all
    -inf."""
    B = np.asarray(observation, dtype=np.float32)
    A = np.asarray(transition, dtype=np.float32)
    p = np.asarray(initial, dtype=np.float32)
    total, states = B.shape
    length = total if length is None else max(0, min(int(length), total))
    out = np.zeros(total, dtype=np.int32)
    if length == 0:
        return out
    rows = np.arange(states)
    pointers = np.zeros((length, states), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        d = B[0] + p
        for t in range(1, length):
            candidates = d[None, :] + A
            best = np.argmax(candidates, axis=1)
            pointers[t] = best
            d = B[t] + candidates[rows, best]
    state = int(np.argmax(d))
    out[length - 1] = state
    for t in range(length - 1, 0, -1):
        state = int(pointers[t, state])
        out[t - 1] = state
    return out


def path_score(path, observation, transition, initial):
    """The fp32 score of one path under the recurrence above"""
    B = np.asarray(observation, dtype=np.float32)
    A = np.asarray(transition, dtype=np.float32)
    d = np.float32(B[0, path[0]] + np.float32(initial[path[0]]))
    for t in range(1, len(path)):
        d = np.float32(B[t, path[t]] + np.float32(d + A[path[t], path[t - 1]]))
    return d


def brute_force(observation, transition, initial):
    """The best score over all S^T paths"""
    total, states = np.asarray(observation).shape
    return max(
        path_score(path, observation, transition, initial)
        for path in itertools.product(range(states), repeat=total))


def decoder_model(freqs):
    """(transition, initial) probabilities of harmonics.py:232-243"""
    logfreq = torch.log2(freqs)
    transition = 1. - 3.5 * torch.cdist(
        logfreq[None, :, None],
        logfreq[None, :, None],
        p=1.0
    )[0]
    transition[transition < 0.] = 0.
    transition /= transition.sum(dim=1)
    initial = torch.linspace(1., 0., len(logfreq))
    initial /= initial.sum()
    return transition, initial


def decode(frames, freqs, pitch=None, max_harmonics=3, ratio=.8):
    """harmonics.py:215-297 on features (T, S): (max_harmonics, T)"""
    transition, initial = decoder_model(freqs)
    with np.errstate(divide='ignore'):
        log_transition = torch.log(transition).numpy()
        log_initial = torch.log(initial).numpy()
    harmonics = torch.full((max_harmonics, len(frames)), float('nan'))
    i = 0
    if pitch is not None:
        harmonics[0] = pitch.reshape(-1)
        i = 1
        x, valid = observation(
            frames, freqs, harmonics[0], 1. + ratio, 1. + 1. / ratio)
    else:
        x, valid = observation(frames, freqs)
    while i < max_harmonics:
        indices = torch.from_numpy(
            viterbi(x.numpy(), log_transition, log_initial)).long()
        harmonics[i] = torch.where(valid, freqs[indices], float('nan'))
        i += 1
        if i == max_harmonics:
            break
        x, valid = observation(
            frames, freqs, harmonics[0], i + ratio, i + 1. / ratio)
    return harmonics


###############################################################################
# Peak picking (harmonics.py:199-212)
###############################################################################


def find_peaks(x):
    """scipy.signal.find_peaks(x)[0] with no conditions: samples strictly
    above both neighbours; a plateau counts once, at (left + right) // 2"""
    peaks = []
    i, last = 1, len(x) - 1
    while i < last:
        if x[i - 1] < x[i]:
            ahead = i + 1
            while ahead < last and x[ahead] == x[i]:
                ahead += 1
            if x[ahead] < x[i]:
                peaks.append((i + ahead - 1) // 2)
                i = ahead
        i += 1
    return np.array(peaks, dtype=np.int64)


def peak_pick(frames, freqs, max_harmonics=3):
    try:
        from scipy.signal import find_peaks as find
        peaks = [find(np.asarray(frame))[0] for frame in frames]
    except ImportError:
        peaks = [find_peaks(np.asarray(frame)) for frame in frames]
    harmonics = torch.full((max_harmonics, len(frames)), float('nan'))
    for i, peak in enumerate(peaks):
        for j, p in enumerate(sorted(peak)[:max_harmonics]):
            harmonics[j, i] = freqs[p]
    return harmonics


###############################################################################
# End to end
###############################################################################


def from_audio(audio, pitch=None, max_harmonics=3):
    """Harmonics (max_harmonics, frames) of audio (samples,) at SAMPLE_RATE:
    the float64 high-pass and STFT rounded to fp32 features, the fp32
    observation and the decode"""
    filtered = biquad(np.asarray(audio, dtype=np.float32)).astype(np.float32)
    features, _ = stft(filtered)
    freqs, _ = frequencies()
    return decode(features.to(torch.float32), freqs, pitch, max_harmonics)


def synthetic_voice(samples=22150, glide=.3, seed=0):
    """Harmonics 1-5 of f0 = 110 * 2^(glide t) Hz at amplitude 0.2 / k plus
    noise of 0.003: (audio float32 (samples,), f0 at every sample float64)"""
    t = np.arange(samples) / SAMPLE_RATE
    f0 = 110. * 2. ** (glide * t)
    phase = 2 * np.pi * np.cumsum(f0) / SAMPLE_RATE
    audio = sum(.2 / k * np.sin(k * phase) for k in range(1, 6))
    audio = audio + .003 * np.random.RandomState(seed).randn(samples)
    return audio.astype(np.float32), f0


def check_contours(harmonics, f0):
    """The worst distance (Hz) of contour k from (k + 1) f0 at the frame
    centres 256 j + 128, over frames 8 .. T - 9"""
    harmonics = np.asarray(harmonics, dtype=np.float64)
    count = harmonics.shape[-1]
    centres = HOPSIZE * np.arange(count) + HOPSIZE // 2
    worst = 0.
    for k in range(harmonics.shape[0]):
        error = np.abs(harmonics[k] - (k + 1) * f0[centres])[8:count - 8]
        assert not np.isnan(error).any()
        worst = max(worst, float(error.max()))
    return worst

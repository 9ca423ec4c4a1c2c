"""CPU restatement of promonet/preprocess/harmonics.py:305-330
(`lpc_coefficients`): zero padding, Hamming-windowed frames, Burg's linear
predictor, the all-pole response and log10 |H|. Not a test: the oracle of
test_cpu_lpc.py and test_gpu_lpc.py. It shares no code with promonet_amd.

librosa is not a dependency: `burg` restates `librosa.lpc` from its published
algorithm (float32 in, float32 arithmetic), parity unpinned. The float64
evaluation of the same recursion is what the device is held to; the float32
one is the yardstick (what the reference's own arithmetic loses).
"""
import numpy as np
import torch

SAMPLE_RATE = 22050
HOPSIZE = 256
WINDOW_SIZE = 1024
NUM_FFT = 1024
BINS = NUM_FFT // 2
PADDING = (WINDOW_SIZE - HOPSIZE) // 2
ORDER = int(SAMPLE_RATE / 1000 + 2)


def frame_count(samples):
    """Frames of `samples` samples of audio: the unfold of the padded signal"""
    return max(0, (samples + 2 * PADDING - WINDOW_SIZE) // HOPSIZE + 1)


def frequencies():
    """(512,) float32 (:321-322): spaced sample_rate / 1023, not the FFT's
    grid"""
    result = SAMPLE_RATE * torch.linspace(0., 1., NUM_FFT)
    return result[0:len(result) // 2]


def frames(audio, dtype=np.float64):
    """(T, 1024) windowed frames of float32 audio (samples,) (:307-318). The
    window is torch.hamming_window's float32 one in both precisions; float64
    takes the exact product of the two float32 factors."""
    audio = np.asarray(audio, dtype=np.float32)
    padded = np.concatenate([
        np.zeros(PADDING, np.float32), audio, np.zeros(PADDING, np.float32)])
    count = frame_count(len(audio))
    window = torch.hamming_window(WINDOW_SIZE).numpy().astype(dtype)
    index = HOPSIZE * np.arange(count)[:, None] + np.arange(WINDOW_SIZE)[None]
    return padded[index].astype(dtype).reshape(count, WINDOW_SIZE) * window


def total(values):
    """The sum of a 1-D array in its dtype by a fixed pairwise tree (halves
    added elementwise until one value is left): the same bits on every host,
    which numpy's own reductions do not promise"""
    size = 1
    while size < len(values):
        size *= 2
    work = np.zeros(size, dtype=values.dtype)
    work[:len(values)] = values
    while size > 1:
        size //= 2
        work = work[:size] + work[size:]
    return work[0]


def burg(y, order, dtype=np.float64, direct=False, history=None):
    """Burg's predictor a (order + 1,), a[0] = 1, of one frame: librosa.lpc's
    recursion, every operation in `dtype`.

    direct: recompute the denominator as sum(f^2 + b^2) every order instead
    of updating it (equal in exact arithmetic). history: a list that receives
    (denominator used, direct sum) of every order."""
    y = np.asarray(y).astype(dtype)
    tiny = dtype(np.finfo(np.float32).tiny)
    two = dtype(2)
    a = np.zeros(order + 1, dtype=dtype)
    a[0] = 1
    f, b = y[1:].copy(), y[:-1].copy()
    den = total(f * f) + total(b * b)
    for i in range(order):
        if direct:
            den = total(f * f) + total(b * b)
        if history is not None:
            history.append((den, total(f * f) + total(b * b)))
        r = dtype(-two * total(b * f) / (den + tiny))
        previous = a.copy()
        for j in range(1, i + 2):
            a[j] = previous[j] + r * previous[i - j + 1]
        forward = f + r * b
        backward = b + r * f
        den = (dtype(1) - r * r) * den - backward[-1] ** 2 - forward[0] ** 2
        f, b = forward[1:], backward[:-1]
    return a


def response(a, bins=BINS):
    """|H_k| = |1 / sum_j a[j] e^(-i pi j k / bins)|, k < bins, in float64:
    scipy.signal.freqz([1], a, worN=bins)"""
    a = np.asarray(a, dtype=np.float64)
    angle = np.pi * np.outer(np.arange(bins), np.arange(len(a))) / bins
    return 1. / np.abs(np.exp(-1j * angle) @ a)


def features(audio, dtype=np.float64, order=ORDER, direct=False):
    """(log10 |H| (T, 512) float64, coefficients (T, order + 1) float64) of
    float32 audio (samples,): the Burg recursion in `dtype`, the response in
    float64 either way"""
    windowed = frames(audio, dtype)
    coefficients = np.zeros((len(windowed), order + 1))
    for t, frame in enumerate(windowed):
        coefficients[t] = burg(frame, order, dtype, direct)
    result = np.zeros((len(windowed), BINS))
    for t, a in enumerate(coefficients):
        result[t] = np.log10(response(a))
    return result, coefficients


###############################################################################
# Signals
###############################################################################


def resonator(centres, bandwidths):
    """The all-pole denominator (1 + 2 len(centres),) with a pole pair at
    every centre frequency (Hz) of the given -3 dB bandwidth (Hz)"""
    a = np.ones(1)
    for centre, bandwidth in zip(centres, bandwidths):
        radius = np.exp(-np.pi * bandwidth / SAMPLE_RATE)
        theta = 2 * np.pi * centre / SAMPLE_RATE
        a = np.convolve(a, [1., -2. * radius * np.cos(theta), radius ** 2])
    return a


def autoregressive(a, samples, seed, warmup=4096):
    """Unit-variance white noise through 1 / A(z), float64, after `warmup`
    samples of run-in"""
    noise = np.random.RandomState(seed).randn(samples + warmup)
    out = np.zeros(samples + warmup)
    order = len(a) - 1
    for n in range(samples + warmup):
        value = noise[n]
        for j in range(1, min(order, n) + 1):
            value -= a[j] * out[n - j]
        out[n] = value
    return out[warmup:]


def resonant(centres, bandwidths, floor_db, samples, seed):
    """A noise-driven resonant signal of peak 0.5 plus white noise `floor_db`
    dB under the peak (None: no floor), float32 (samples,)"""
    signal = autoregressive(resonator(centres, bandwidths), samples, seed)
    signal *= .5 / np.abs(signal).max()
    if floor_db is not None:
        floor = np.random.RandomState(seed + 1000).randn(samples)
        signal = signal + .5 * 10. ** (-floor_db / 20.) * floor
    return signal.astype(np.float32)


SAMPLES = 2048      # 8 frames

# the gated cases of test_gpu_lpc.py: noise-driven, no clean periodic input
# (there the reference's own float32 recursion is off by 0.1 to 12)
CASES = {
    'white': lambda: (.1 * np.random.RandomState(0).randn(SAMPLES)).astype(
        np.float32),
    'three resonances, 40 dB floor': lambda: resonant(
        (700., 1800., 3200.), (90., 110., 150.), 40., SAMPLES, 1),
    'two wide resonances': lambda: resonant(
        (900., 2600.), (400., 600.), None, SAMPLES, 2),
    'four resonances, 40 dB floor': lambda: resonant(
        (500., 1500., 2500., 3500.), (60., 80., 100., 120.), 40., SAMPLES, 3),
}


def case(name):
    return CASES[name]()
